// san_flanger.cpp — s2r_flanger_reference of csrc/s2r_rules.cpp under ASan + UBSan (tests/test_flanger_native.py) at the edges of its
// shapes — H = 33 and 4096, frames 0, 1, 31, 32, 33, H - 1, H, H + 1, no output buffer — every buffer allocated at exactly the size
// s2r.h states, the answers that need no model, and refusals that touch nothing.  Built with -ffp-contract=off.  Prints "flanger ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "s2r.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "san_flanger.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

// a heap block of exactly n floats (n == 0: a pointer that is not null and must not be touched)
struct Buf {
    float *p;
    size_t n;
    explicit Buf(size_t n_, float fill = 0.0f) : p(new float[n_]), n(n_) { for (size_t i = 0; i < n; i++) p[i] = fill; }
    ~Buf() { delete[] p; }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    float &operator[](size_t i) { return p[i]; }
};

uint32_t rng_state = 2468u;
float noise() {                                  // in (-1, 1), never 0
    rng_state = rng_state * 1664525u + 1013904223u;
    return ((float)(rng_state >> 8) + 0.5f) / 8388608.0f - 1.0f;
}
void fill_noise(Buf &b, float scale = 1.0f) { for (size_t i = 0; i < b.n; i++) b[i] = noise() * scale; }

const uint32_t kFrames[] = {0u, 1u, 31u, 32u, 33u};

// depth 0, a whole base B: d = B, f = 0, tap[n] = w[n - B].  With feedback = cross = 0 and dry 0, wet 1 the output is the line B
// frames late and the line is x (x + 0: the noise has no zero, so on bits); with feedback 1 the line is the recursion w[n] = x[n] +
// w[n - B], restated here
void plain_comb() {
    const uint32_t bases[] = {32u, 4095u};
    for (uint32_t B : bases) {
        const uint32_t H = B + 1u;
        CHECK(s2r_flanger_history_frames((float)B, 0.0f) == H);
        std::vector<uint32_t> frames(kFrames, kFrames + 5);
        frames.push_back(H - 1u); frames.push_back(H); frames.push_back(H + 1u);
        for (uint32_t N : frames)
            for (int fed = 0; fed < 2; fed++) {
                Buf x(2u * (size_t)N), hist(2u * (size_t)H), out(2u * (size_t)N), hist2(2u * (size_t)H);
                fill_noise(x, 0.25f); fill_noise(hist, 0.25f);
                std::vector<float> w(hist.p, hist.p + hist.n);   // the line: the history, then the call's
                for (size_t i = 0; i < hist.n; i++) hist2[i] = hist[i];
                uint32_t phase = 0xfffffff0u, phase2 = phase;
                const float fb = fed ? 1.0f : 0.0f;
                CHECK(s2r_flanger_reference((float)B, 0.0f, 7u, 0x80000000u, fb, 0.0f, 0.0f, 1.0f, N ? x.p : nullptr, N, hist.p, &phase, N ? out.p : nullptr) == S2R_OK);
                for (size_t n = 0; n < N; n++)
                    for (size_t c = 0; c < 2; c++) {
                        const float tap = w[2 * (H + n - B) + c];
                        CHECK(out[2 * n + c] == tap);
                        const float p = fb * tap;
                        const float s = p + 0.0f * w[2 * (H + n - B) + (1 - c)];
                        w.push_back(x[2 * n + c] + s);
                    }
                for (size_t i = 0; i < hist.n; i++) CHECK(hist[i] == w[w.size() - hist.n + i]);      // the last H of (history, w)
                CHECK(phase == 0xfffffff0u + 7u * N);
                // no output buffer: the state moves on all the same
                CHECK(s2r_flanger_reference((float)B, 0.0f, 7u, 0x80000000u, fb, 0.0f, 0.0f, 1.0f, N ? x.p : nullptr, N, hist2.p, &phase2, nullptr) == S2R_OK);
                for (size_t i = 0; i < hist.n; i++) CHECK(hist2[i] == hist[i]);
                CHECK(phase2 == phase);
            }
    }
}

// the whole depth at H = 33 (32 + 0.5) and H = 4096 (32 + 4063), every phase of the triangle met by a fast LFO, feedback and cross at
// the edge of their sum: the taps reach the oldest frame and never past it; |w| <= |x| + |tap| keeps everything finite here
void swept() {
    const float shapes[][2] = {{32.0f, 0.5f}, {32.0f, 4063.0f}, {4094.5f, 0.5f}, {2000.3f, 2094.6f}};
    for (const float *sh : shapes) {
        const uint32_t H = s2r_flanger_history_frames(sh[0], sh[1]);
        CHECK(H >= 33u && H <= 4096u);
        std::vector<uint32_t> frames(kFrames, kFrames + 5);
        frames.push_back(H - 1u); frames.push_back(H); frames.push_back(H + 1u);
        for (uint32_t N : frames) {
            Buf x(2u * (size_t)N), hist(2u * (size_t)H), out(2u * (size_t)N);
            fill_noise(x, 0.01f); fill_noise(hist, 0.01f);
            uint32_t phase = 0x80000000u;                        // m == 1 at frame 0: i = H - 1
            CHECK(s2r_flanger_reference(sh[0], sh[1], 0x01000193u, 0x40000000u, -0.5f, 0.5f, 0.5f, 0.125f, N ? x.p : nullptr, N, hist.p, &phase, N ? out.p : nullptr) == S2R_OK);
            for (size_t i = 0; i < out.n; i++) CHECK(std::isfinite(out[i]));
            for (size_t i = 0; i < hist.n; i++) CHECK(std::isfinite(hist[i]));
            CHECK(phase == 0x80000000u + 0x01000193u * N);
            phase = 0x80000000u;
            CHECK(s2r_flanger_reference(sh[0], sh[1], 0u, 0u, 1.0f, 0.0f, 0.0f, 1.0f, N ? x.p : nullptr, N, hist.p, &phase, N ? out.p : nullptr) == S2R_OK);
            CHECK(phase == 0x80000000u);
        }
    }
}

void refusals() {
    Buf one(66, 1.0f), x(2, 1.0f), out(2, 1.0f);
    uint32_t phase = 3u;
#define REFUSED(base, depth, fb, cr, dry, wet) CHECK(s2r_flanger_reference(base, depth, 0, 0, fb, cr, dry, wet, x.p, 1, one.p, &phase, out.p) == S2R_ERR_PATCH_RANGE)
    REFUSED(31.999f, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f);
    REFUSED(1.0f, 40.0f, 0.0f, 0.0f, 1.0f, 1.0f);
    REFUSED(32.0f, -1.0f, 0.0f, 0.0f, 1.0f, 1.0f);
    REFUSED(NAN, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f);
    REFUSED(32.0f, INFINITY, 0.0f, 0.0f, 1.0f, 1.0f);
    REFUSED(std::nextafterf(4095.0f, 5000.0f), 0.0f, 0.0f, 0.0f, 1.0f, 1.0f);
    REFUSED(32.0f, 0.0f, 0.5f, std::nextafterf(0.5f, 1.0f), 1.0f, 1.0f);
    REFUSED(32.0f, 0.0f, -1.5f, 0.0f, 1.0f, 1.0f);
    REFUSED(32.0f, 0.0f, 0.0f, NAN, 1.0f, 1.0f);
    REFUSED(32.0f, 0.0f, 0.0f, 0.0f, 1.5f, 1.0f);
    REFUSED(32.0f, 0.0f, 0.0f, 0.0f, 1.0f, -0.5f);
#undef REFUSED
    CHECK(s2r_flanger_reference(32.0f, 0.0f, 0, 0, 0.0f, 0.0f, 1.0f, 1.0f, x.p, 1, nullptr, &phase, out.p) == S2R_ERR_INVALID);
    CHECK(s2r_flanger_reference(32.0f, 0.0f, 0, 0, 0.0f, 0.0f, 1.0f, 1.0f, x.p, 1, one.p, nullptr, out.p) == S2R_ERR_INVALID);
    CHECK(s2r_flanger_reference(32.0f, 0.0f, 0, 0, 0.0f, 0.0f, 1.0f, 1.0f, nullptr, 1, one.p, &phase, out.p) == S2R_ERR_INVALID);
    for (size_t i = 0; i < one.n; i++) CHECK(one[i] == 1.0f);
    CHECK(out[0] == 1.0f && out[1] == 1.0f && phase == 3u);
    CHECK(s2r_flanger_history_frames(31.0f, 1.0f) == 0u && s2r_flanger_history_frames(4095.0f, 1.0f) == 0u && s2r_flanger_history_frames(NAN, 0.0f) == 0u);
}

}  // namespace

int main() {
    plain_comb();
    swept();
    refusals();
    std::printf("flanger ok\n");
    return 0;
}
