// san_eq.cpp — s2r_eq_reference and s2r_eq_design of csrc/s2r_rules.cpp under ASan + UBSan (tests/test_eq_native.py) at the edges of
// their shapes — 1 to S2R_EQ_MAX_BANDS bands; no frames, one, two, five, a thousand; no output buffer — every buffer allocated at
// exactly the size s2r.h states, and the answers that need no model.  Built with -ffp-contract=off.  Prints "eq ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "s2r.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "san_eq.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

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
bool same_bits(const float *a, const float *b, size_t n) { return n == 0 || std::memcmp(a, b, n * sizeof(float)) == 0; }

const int kKinds[6] = {S2R_EQ_PEAK, S2R_EQ_LOW_SHELF, S2R_EQ_HIGHPASS, S2R_EQ_HIGH_SHELF, S2R_EQ_LOWPASS, S2R_EQ_PEAK};

void design(Buf &c, uint32_t bands) {
    for (uint32_t k = 0; k < bands; k++)
        CHECK(s2r_eq_design(kKinds[k], 150.0 * (k + 1) * (k + 1), k % 2 ? -9.0 : 6.0, 0.7 + k, 48000.0, c.p + 5 * k) == S2R_OK);
}

// every shape on exact buffers; one call equals two, on bits; a null output moves the state on all the same
void shapes() {
    const uint32_t frames[] = {0u, 1u, 2u, 5u, 1000u};
    for (uint32_t bands = 1; bands <= S2R_EQ_MAX_BANDS; bands++) {
        Buf c(5u * bands);
        design(c, bands);
        for (uint32_t N : frames) {
            Buf x(2u * (size_t)N), out(2u * (size_t)N), st(4u * bands), st2(4u * bands), st3(4u * bands);
            fill_noise(x); fill_noise(st);
            for (size_t i = 0; i < st.n; i++) st3[i] = st2[i] = st[i];
            CHECK(s2r_eq_reference(bands, c.p, N ? x.p : nullptr, N, st.p, N ? out.p : nullptr) == S2R_OK);
            for (size_t i = 0; i < out.n; i++) CHECK(std::isfinite(out[i]));
            CHECK(s2r_eq_reference(bands, c.p, N ? x.p : nullptr, N, st2.p, nullptr) == S2R_OK);
            CHECK(same_bits(st.p, st2.p, st.n));
            if (N == 0) { CHECK(same_bits(st.p, st3.p, st.n)); continue; }
            const uint32_t cut = N / 2u;                 // (0 for one frame: an empty first call)
            Buf a(2u * (size_t)cut), b(2u * (size_t)(N - cut)), xa(2u * (size_t)cut), xb(2u * (size_t)(N - cut));
            for (size_t i = 0; i < xa.n; i++) xa[i] = x[i];
            for (size_t i = 0; i < xb.n; i++) xb[i] = x[xa.n + i];
            CHECK(s2r_eq_reference(bands, c.p, cut ? xa.p : nullptr, cut, st3.p, cut ? a.p : nullptr) == S2R_OK);
            CHECK(s2r_eq_reference(bands, c.p, xb.p, N - cut, st3.p, b.p) == S2R_OK);
            CHECK(same_bits(a.p, out.p, a.n) && same_bits(b.p, out.p + a.n, b.n) && same_bits(st3.p, st.p, st.n));
        }
    }
}

// no model: a band (g, 0, 0, 0, 0) from a zero state is a gain, as values; two of them in a row are the two products in order; and a
// pure two-frame delay (0, 0, 1, 0, 0) is the stream two frames late with the state (x[N - 1], x[N - 2]) per channel
void plain_answers() {
    const uint32_t N = 33;
    Buf x(2u * N), out(2u * N), c(10), st(8);
    fill_noise(x);
    c[0] = 0.5f; c[5] = -3.0f;
    CHECK(s2r_eq_reference(2, c.p, x.p, N, st.p, out.p) == S2R_OK);
    for (size_t i = 0; i < x.n; i++) { const float h = 0.5f * x[i]; CHECK(out[i] == -3.0f * h); }
    for (size_t i = 0; i < st.n; i++) CHECK(st[i] == 0.0f);
    Buf d(5), sd(4);
    d[2] = 1.0f;
    CHECK(s2r_eq_reference(1, d.p, x.p, N, sd.p, out.p) == S2R_OK);
    for (size_t n = 0; n < N; n++)
        for (size_t ch = 0; ch < 2; ch++) CHECK(out[2 * n + ch] == (n >= 2 ? x[2 * (n - 2) + ch] : 0.0f));
    // s1 is what leaves at the next frame, s2 the frame after: x[N - 2] and x[N - 1]
    CHECK(sd[0] == x[2 * (N - 2)] && sd[1] == x[2 * (N - 2) + 1] && sd[2] == x[2 * (N - 1)] && sd[3] == x[2 * (N - 1) + 1]);
}

// a refusal touches nothing: a band on the triangle's edge, a coefficient that is not finite, no bands, too many
void refusals() {
    Buf x(6), out(6, 9.0f), st(16, 0.25f), c(5u * (S2R_EQ_MAX_BANDS + 1u));
    fill_noise(x);
    for (uint32_t k = 0; k <= S2R_EQ_MAX_BANDS; k++) c[5 * k] = 1.0f;
    CHECK(s2r_eq_reference(0, c.p, x.p, 3, st.p, out.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_eq_reference(S2R_EQ_MAX_BANDS + 1u, c.p, x.p, 3, st.p, out.p) == S2R_ERR_PATCH_RANGE);
    c[4] = 1.0f;
    CHECK(s2r_eq_reference(1, c.p, x.p, 3, st.p, out.p) == S2R_ERR_PATCH_RANGE);
    c[4] = 0.5f; c[3] = 1.5f;
    CHECK(s2r_eq_reference(1, c.p, x.p, 3, st.p, out.p) == S2R_ERR_PATCH_RANGE);
    c[3] = 0.0f; c[5 * 3 + 1] = INFINITY;
    CHECK(s2r_eq_reference(4, c.p, x.p, 3, st.p, out.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_eq_reference(3, c.p, x.p, 3, st.p, out.p) == S2R_OK);          // (the band that is not finite is the fourth)
    Buf st2(16, 0.25f), out2(6, 9.0f);
    CHECK(s2r_eq_reference(3, c.p, nullptr, 3, st2.p, out2.p) == S2R_ERR_INVALID);
    CHECK(s2r_eq_reference(3, nullptr, x.p, 3, st2.p, out2.p) == S2R_ERR_INVALID);
    CHECK(s2r_eq_reference(3, c.p, x.p, 3, nullptr, out2.p) == S2R_ERR_INVALID);
    for (size_t i = 0; i < st2.n; i++) CHECK(st2[i] == 0.25f);
    for (size_t i = 0; i < out2.n; i++) CHECK(out2[i] == 9.0f);
    float five[5] = {9.0f, 9.0f, 9.0f, 9.0f, 9.0f};
    CHECK(s2r_eq_design(S2R_EQ_PEAK, 24000.0, 0.0, 1.0, 48000.0, five) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_eq_design(7, 1000.0, 0.0, 1.0, 48000.0, five) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_eq_design(S2R_EQ_PEAK, 1000.0, 0.0, 1.0, 48000.0, nullptr) == S2R_ERR_INVALID);
    for (float v : five) CHECK(v == 9.0f);
    CHECK(s2r_eq_design(S2R_EQ_PEAK, 1000.0, 0.0, 1.0, 48000.0, five) == S2R_OK);
    CHECK(five[0] == 1.0f && five[1] == five[3] && five[2] == five[4]);
}

}  // namespace

int main() {
    shapes();
    plain_answers();
    refusals();
    std::printf("eq ok\n");
    return 0;
}
