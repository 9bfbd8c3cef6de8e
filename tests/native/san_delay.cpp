// san_delay.cpp — s2r_delay_reference of csrc/s2r_rules.cpp under ASan + UBSan (tests/test_delay_native.py) at the edges of its
// shapes — D = 1, no frames, fewer frames than D, a frame count that is no multiple of D, no output buffer — every buffer allocated
// at exactly the size s2r.h states, and the answers that need no model.  Built with -ffp-contract=off.  Prints "delay ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "s2r.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "san_delay.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

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
void fill_noise(Buf &b) { for (size_t i = 0; i < b.n; i++) b[i] = noise(); }

void shapes() {
    const uint32_t delays[] = {1u, 2u, 5u, 64u, 1000u};
    for (uint32_t D : delays) {
        const uint32_t frames[] = {0u, 1u, D - 1u, D, D + 1u, 3u * D + 2u};
        for (uint32_t N : frames) {
            Buf x(2u * (size_t)N), hist(2u * (size_t)D), out(2u * (size_t)N), hist2(2u * (size_t)D);
            fill_noise(x); fill_noise(hist);
            std::vector<float> all(hist.p, hist.p + hist.n);         // the stream: the history, then x
            for (size_t i = 0; i < hist.n; i++) hist2[i] = hist[i];
            // feedback 0, cross 0, dry 0, wet 1: the line is the input, and the output the stream D frames late (values: 0 * x gives up no
            // more than the sign of a zero, and the noise has none)
            CHECK(s2r_delay_reference(D, 0.0f, 0.0f, 0.0f, 1.0f, N ? x.p : nullptr, N, hist.p, N ? out.p : nullptr) == S2R_OK);
            for (size_t i = 0; i < x.n; i++) all.push_back(x[i]);
            for (size_t i = 0; i < out.n; i++) CHECK(out[i] == all[i]);
            for (size_t i = 0; i < hist.n; i++) CHECK(hist[i] == all[all.size() - hist.n + i]);      // the last D of (history, W)
            // no output buffer: the history moves on all the same
            CHECK(s2r_delay_reference(D, 0.0f, 0.0f, 0.0f, 1.0f, N ? x.p : nullptr, N, hist2.p, nullptr) == S2R_OK);
            for (size_t i = 0; i < hist.n; i++) CHECK(hist2[i] == hist[i]);
            // feedback and cross at the limit of their sum, from the history the pass above left
            CHECK(s2r_delay_reference(D, -0.5f, 0.5f, 0.25f, 1.0f, N ? x.p : nullptr, N, hist.p, N ? out.p : nullptr) == S2R_OK);
            for (size_t i = 0; i < out.n; i++) CHECK(std::isfinite(out[i]));
            for (size_t i = 0; i < hist.n; i++) CHECK(std::isfinite(hist[i]));
        }
    }
    // the longest delay, fewer frames than it
    {
        Buf x(2u * 3u, 0.5f), hist(2u * (size_t)S2R_MAX_DELAY_FRAMES, 0.25f), out(2u * 3u);
        hist[0] = 1.0f; hist[hist.n - 1] = 2.0f;
        CHECK(s2r_delay_reference(S2R_MAX_DELAY_FRAMES, 1.0f, 0.0f, 1.0f, 1.0f, x.p, 3, hist.p, out.p) == S2R_OK);
        CHECK(out[0] == 1.5f && out[1] == 0.75f && out[5] == 0.75f);
        CHECK(hist[hist.n - 6] == 1.5f && hist[hist.n - 1] == 0.75f && hist[hist.n - 7] == 2.0f && hist[0] == 0.25f);
    }
}

void refusals() {
    Buf one(2, 1.0f);
    CHECK(s2r_delay_reference(0, 0.0f, 0.0f, 1.0f, 1.0f, one.p, 1, one.p, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_delay_reference(S2R_MAX_DELAY_FRAMES + 1u, 0.0f, 0.0f, 1.0f, 1.0f, one.p, 1, one.p, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_delay_reference(1, 0.75f, 0.5f, 1.0f, 1.0f, one.p, 1, one.p, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_delay_reference(1, 0.6f, -0.4f, 1.0f, 1.0f, one.p, 1, one.p, one.p) == S2R_ERR_PATCH_RANGE);       // 1 + 2^-25 in double
    CHECK(s2r_delay_reference(1, NAN, 0.0f, 1.0f, 1.0f, one.p, 1, one.p, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_delay_reference(1, 0.0f, 0.0f, 1.5f, 1.0f, one.p, 1, one.p, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_delay_reference(1, 0.0f, 0.0f, 1.0f, -0.5f, one.p, 1, one.p, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_delay_reference(1, 0.5f, 0.5f, 1.0f, 1.0f, one.p, 1, nullptr, one.p) == S2R_ERR_INVALID);
    CHECK(s2r_delay_reference(1, 0.5f, 0.5f, 1.0f, 1.0f, nullptr, 1, one.p, one.p) == S2R_ERR_INVALID);
    CHECK(one[0] == 1.0f && one[1] == 1.0f);
}

}  // namespace

int main() {
    shapes();
    refusals();
    std::printf("delay ok\n");
    return 0;
}
