// san_chorus.cpp — s2r_chorus_reference of csrc/s2r_rules.cpp under ASan + UBSan (tests/test_chorus_native.py) at the edges of its
// shapes — H = 2 and 4096, no frames, one, H - 1, H, H + 1, no output buffer — every buffer allocated at exactly the size s2r.h
// states, and the answer that needs no model.  Built with -ffp-contract=off.  Prints "chorus ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "s2r.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "san_chorus.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

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

uint32_t rng_state = 1357u;
float noise() {                                  // in (-1, 1), never 0
    rng_state = rng_state * 1664525u + 1013904223u;
    return ((float)(rng_state >> 8) + 0.5f) / 8388608.0f - 1.0f;
}
void fill_noise(Buf &b) { for (size_t i = 0; i < b.n; i++) b[i] = noise(); }

// V = 1, depth 0, a whole base B, dry 0, wet 1: d = B, f = 0, tap = a + 0 * (bb - a): the stream B frames late, as VALUES (a -0.0
// may come out +0.0, by the rule; the noise has no zero)
void plain_delay() {
    const uint32_t bases[] = {1u, 2u, 63u, 4095u};
    for (uint32_t B : bases) {
        const uint32_t H = B + 1u;
        CHECK(s2r_chorus_history_frames((float)B, 0.0f) == H);
        const uint32_t frames[] = {0u, 1u, H - 1u, H, H + 1u};
        for (uint32_t N : frames) {
            Buf x(2u * (size_t)N), hist(2u * (size_t)H), out(2u * (size_t)N), hist2(2u * (size_t)H);
            fill_noise(x); fill_noise(hist);
            std::vector<float> all(hist.p, hist.p + hist.n);         // the stream: the history, then x
            for (size_t i = 0; i < hist.n; i++) hist2[i] = hist[i];
            uint32_t phase = 0xfffffff0u, phase2 = phase;
            CHECK(s2r_chorus_reference(1, (float)B, 0.0f, 7u, 0x80000000u, 0.0f, 1.0f, N ? x.p : nullptr, N, hist.p, &phase, N ? out.p : nullptr) == S2R_OK);
            for (size_t i = 0; i < x.n; i++) all.push_back(x[i]);
            for (size_t n = 0; n < N; n++)
                for (size_t c = 0; c < 2; c++) CHECK(out[2 * n + c] == all[2 * (H + n - B) + c]);
            for (size_t i = 0; i < hist.n; i++) CHECK(hist[i] == all[all.size() - hist.n + i]);      // the last H of (history, x)
            CHECK(phase == 0xfffffff0u + 7u * N);
            // no output buffer: the state moves on all the same
            CHECK(s2r_chorus_reference(1, (float)B, 0.0f, 7u, 0x80000000u, 0.0f, 1.0f, N ? x.p : nullptr, N, hist2.p, &phase2, nullptr) == S2R_OK);
            for (size_t i = 0; i < hist.n; i++) CHECK(hist2[i] == hist[i]);
            CHECK(phase2 == phase);
        }
    }
}

// the whole depth at H = 2 (1 + 0.5) and H = 4096 (1 + 4094), eight voices, every phase of the triangle met by a fast LFO: the taps
// reach the oldest frame and never past it
void swept() {
    const float shapes[][2] = {{1.0f, 0.5f}, {1.0f, 4094.0f}, {4094.5f, 0.5f}, {2000.3f, 2094.6f}};
    for (const float *sh : shapes) {
        const uint32_t H = s2r_chorus_history_frames(sh[0], sh[1]);
        CHECK(H >= 2u && H <= 4096u);
        const uint32_t frames[] = {0u, 1u, H - 1u, H, H + 1u};
        for (uint32_t N : frames) {
            Buf x(2u * (size_t)N), hist(2u * (size_t)H), out(2u * (size_t)N);
            fill_noise(x); fill_noise(hist);
            uint32_t phase = 0x80000000u;                        // m == 1 at frame 0: i = H - 1
            CHECK(s2r_chorus_reference(8, sh[0], sh[1], 0x01000193u, 0x40000000u, 0.5f, 0.125f, N ? x.p : nullptr, N, hist.p, &phase, N ? out.p : nullptr) == S2R_OK);
            for (size_t i = 0; i < out.n; i++) CHECK(std::isfinite(out[i]) && std::fabs(out[i]) <= 0.5f + 0.125f * 8.0f);
            if (N) for (size_t i = 0; i < 2; i++) CHECK(hist[hist.n - 2 + i] == x[x.n - 2 + i]);
            phase = 0x80000000u;
            CHECK(s2r_chorus_reference(1, sh[0], sh[1], 0u, 0u, 0.0f, 1.0f, N ? x.p : nullptr, N, hist.p, &phase, N ? out.p : nullptr) == S2R_OK);
            CHECK(phase == 0x80000000u);
        }
    }
}

void refusals() {
    Buf one(4, 1.0f);
    uint32_t phase = 3u;
    CHECK(s2r_chorus_reference(0, 1.0f, 0.0f, 0, 0, 1.0f, 1.0f, one.p, 1, one.p, &phase, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_chorus_reference(9, 1.0f, 0.0f, 0, 0, 1.0f, 1.0f, one.p, 1, one.p, &phase, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_chorus_reference(1, 0.5f, 0.0f, 0, 0, 1.0f, 1.0f, one.p, 1, one.p, &phase, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_chorus_reference(1, 1.0f, -1.0f, 0, 0, 1.0f, 1.0f, one.p, 1, one.p, &phase, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_chorus_reference(1, NAN, 0.0f, 0, 0, 1.0f, 1.0f, one.p, 1, one.p, &phase, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_chorus_reference(1, 1.0f, INFINITY, 0, 0, 1.0f, 1.0f, one.p, 1, one.p, &phase, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_chorus_reference(1, std::nextafterf(4095.0f, 5000.0f), 0.0f, 0, 0, 1.0f, 1.0f, one.p, 1, one.p, &phase, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_chorus_reference(1, 1.0f, 0.0f, 0, 0, 1.5f, 1.0f, one.p, 1, one.p, &phase, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_chorus_reference(1, 1.0f, 0.0f, 0, 0, 1.0f, -0.5f, one.p, 1, one.p, &phase, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_chorus_reference(1, 1.0f, 0.0f, 0, 0, 1.0f, 1.0f, one.p, 1, nullptr, &phase, one.p) == S2R_ERR_INVALID);
    CHECK(s2r_chorus_reference(1, 1.0f, 0.0f, 0, 0, 1.0f, 1.0f, one.p, 1, one.p, nullptr, one.p) == S2R_ERR_INVALID);
    CHECK(s2r_chorus_reference(1, 1.0f, 0.0f, 0, 0, 1.0f, 1.0f, nullptr, 1, one.p, &phase, one.p) == S2R_ERR_INVALID);
    CHECK(one[0] == 1.0f && one[3] == 1.0f && phase == 3u);
    CHECK(s2r_chorus_history_frames(0.5f, 0.0f) == 0u && s2r_chorus_history_frames(4095.0f, 1.0f) == 0u && s2r_chorus_history_frames(NAN, 0.0f) == 0u);
}

}  // namespace

int main() {
    plain_delay();
    swept();
    refusals();
    std::printf("chorus ok\n");
    return 0;
}
