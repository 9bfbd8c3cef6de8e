// san_dyn.cpp — s2r_dynamics_reference, s2r_dynamics_curve and s2r_dynamics_coef of csrc/s2r_rules.cpp under ASan + UBSan
// (tests/test_dyn_native.py) at the edges of their shapes — no frames, one, two, five, a thousand; self-keyed and keyed by another
// buffer; no output buffer, no meter — every buffer allocated at exactly the size s2r.h states, and the answers that need no model.
// Built with -ffp-contract=off.  Prints "dyn ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "s2r.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "san_dyn.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

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
bool same_bits(const float *a, const float *b, size_t n) { return n == 0 || std::memcmp(a, b, n * sizeof(float)) == 0; }
float level(uint32_t j) { return std::ldexp(1.0f + (float)(j % 16u) / 16.0f, -24 + (int)(j / 16u)); }

// every shape on exact buffers; one call equals two, on bits; null outputs move the gain on all the same
void shapes() {
    const uint32_t frames[] = {0u, 1u, 2u, 5u, 1000u};
    Buf curve(S2R_DYN_CURVE_POINTS);
    CHECK(s2r_dynamics_curve(-20.0, 4.0, 6.0, 3.0, curve.p) == S2R_OK);
    const float a_att = s2r_dynamics_coef(1.0, 48000.0), a_rel = s2r_dynamics_coef(100.0, 48000.0);
    CHECK(a_att > 0.97f && a_att < 0.98f && a_rel > a_att && a_rel < 1.0f && s2r_dynamics_coef(0.0, 48000.0) == 0.0f);
    for (int cross = 0; cross < 2; cross++)
        for (uint32_t N : frames) {
            Buf x(2u * (size_t)N), key(2u * (size_t)N), out(2u * (size_t)N), y(1, curve[0]), y2(1, curve[0]), y3(1, curve[0]), mn(1, 9.0f), mn2(1, 9.0f);
            fill_noise(x); fill_noise(key);
            const float *k = cross ? (N ? key.p : nullptr) : nullptr;
            CHECK(s2r_dynamics_reference(curve.p, a_att, a_rel, k, N ? x.p : nullptr, N, y.p, N ? out.p : nullptr, mn.p) == S2R_OK);
            for (size_t i = 0; i < out.n; i++) CHECK(std::isfinite(out[i]));
            CHECK(y[0] >= 0.0f && (N ? mn[0] <= curve[0] && mn[0] >= 0.0f : mn[0] == 9.0f));
            CHECK(s2r_dynamics_reference(curve.p, a_att, a_rel, k, N ? x.p : nullptr, N, y2.p, nullptr, nullptr) == S2R_OK);
            CHECK(same_bits(y.p, y2.p, 1));
            if (N == 0) { CHECK(y[0] == curve[0]); continue; }
            const uint32_t cut = N / 2u;                 // (0 for one frame: an empty first call)
            Buf a(2u * (size_t)cut), b(2u * (size_t)(N - cut)), xa(2u * (size_t)cut), xb(2u * (size_t)(N - cut)), ka(2u * (size_t)cut), kb(2u * (size_t)(N - cut));
            for (size_t i = 0; i < xa.n; i++) { xa[i] = x[i]; ka[i] = key[i]; }
            for (size_t i = 0; i < xb.n; i++) { xb[i] = x[xa.n + i]; kb[i] = key[xa.n + i]; }
            CHECK(s2r_dynamics_reference(curve.p, a_att, a_rel, cross && cut ? ka.p : nullptr, cut ? xa.p : nullptr, cut, y3.p, cut ? a.p : nullptr, mn2.p) == S2R_OK);
            CHECK(s2r_dynamics_reference(curve.p, a_att, a_rel, cross ? kb.p : nullptr, xb.p, N - cut, y3.p, b.p, mn2.p) == S2R_OK);
            CHECK(same_bits(a.p, out.p, a.n) && same_bits(b.p, out.p + a.n, b.n) && same_bits(y3.p, y.p, 1));
        }
}

// no model: a constant curve is a gain whatever the key and the coefficients; with zero coefficients a key at breakpoint j reads
// curve[j]; in place (out == x) is the same
void plain_answers() {
    const uint32_t N = 33;
    Buf x(2u * N), out(2u * N), half(S2R_DYN_CURVE_POINTS, 0.5f), y(1, 0.5f), mn(1);
    fill_noise(x);
    CHECK(s2r_dynamics_reference(half.p, 0.9f, 0.99f, nullptr, x.p, N, y.p, out.p, mn.p) == S2R_OK);
    for (size_t i = 0; i < x.n; i++) CHECK(out[i] == 0.5f * x[i]);
    CHECK(y[0] == 0.5f && mn[0] == 0.5f);
    Buf ramp(S2R_DYN_CURVE_POINTS), key(2u * S2R_DYN_CURVE_POINTS), ones(2u * S2R_DYN_CURVE_POINTS, 1.0f), got(2u * S2R_DYN_CURVE_POINTS), y2(1, 0.0f);
    for (uint32_t j = 0; j < S2R_DYN_CURVE_POINTS; j++) { ramp[j] = 256.0f - 0.4375f * (float)j; key[2u * j + (j & 1u)] = (j & 2u) ? -level(j) : level(j); }
    CHECK(s2r_dynamics_reference(ramp.p, 0.0f, 0.0f, key.p, ones.p, S2R_DYN_CURVE_POINTS, y2.p, got.p, mn.p) == S2R_OK);
    for (uint32_t j = 0; j < S2R_DYN_CURVE_POINTS; j++) CHECK(got[2u * j] == ramp[j] && got[2u * j + 1u] == ramp[j]);
    CHECK(y2[0] == ramp[S2R_DYN_CURVE_POINTS - 1u] && mn[0] == ramp[S2R_DYN_CURVE_POINTS - 1u]);
    Buf in_place(2u * N), y3(1, 0.5f), y4(1, 0.5f);
    for (size_t i = 0; i < x.n; i++) in_place[i] = x[i];
    CHECK(s2r_dynamics_reference(ramp.p, 0.5f, 0.75f, nullptr, x.p, N, y3.p, out.p, nullptr) == S2R_OK);
    CHECK(s2r_dynamics_reference(ramp.p, 0.5f, 0.75f, nullptr, in_place.p, N, y4.p, in_place.p, nullptr) == S2R_OK);
    CHECK(same_bits(in_place.p, out.p, out.n) && same_bits(y3.p, y4.p, 1));
}

// a refusal touches nothing
void refusals() {
    Buf x(6), out(6, 9.0f), y(1, 0.25f), mn(1, 9.0f), curve(S2R_DYN_CURVE_POINTS, 1.0f);
    fill_noise(x);
    CHECK(s2r_dynamics_reference(curve.p, 1.0f, 0.5f, nullptr, x.p, 3, y.p, out.p, mn.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_dynamics_reference(curve.p, 0.5f, -0.25f, nullptr, x.p, 3, y.p, out.p, mn.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_dynamics_reference(curve.p, NAN, 0.5f, nullptr, x.p, 3, y.p, out.p, mn.p) == S2R_ERR_PATCH_RANGE);
    curve[512] = 257.0f;
    CHECK(s2r_dynamics_reference(curve.p, 0.5f, 0.5f, nullptr, x.p, 3, y.p, out.p, mn.p) == S2R_ERR_PATCH_RANGE);
    curve[512] = 256.0f; curve[0] = -1.0f;
    CHECK(s2r_dynamics_reference(curve.p, 0.5f, 0.5f, nullptr, x.p, 3, y.p, out.p, mn.p) == S2R_ERR_PATCH_RANGE);
    curve[0] = INFINITY;
    CHECK(s2r_dynamics_reference(curve.p, 0.5f, 0.5f, nullptr, x.p, 3, y.p, out.p, mn.p) == S2R_ERR_PATCH_RANGE);
    curve[0] = 0.0f;
    Buf bad(1, -1.0f);
    CHECK(s2r_dynamics_reference(curve.p, 0.5f, 0.5f, nullptr, x.p, 3, bad.p, out.p, mn.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_dynamics_reference(nullptr, 0.5f, 0.5f, nullptr, x.p, 3, y.p, out.p, mn.p) == S2R_ERR_INVALID);
    CHECK(s2r_dynamics_reference(curve.p, 0.5f, 0.5f, nullptr, nullptr, 3, y.p, out.p, mn.p) == S2R_ERR_INVALID);
    CHECK(s2r_dynamics_reference(curve.p, 0.5f, 0.5f, nullptr, x.p, 3, nullptr, out.p, mn.p) == S2R_ERR_INVALID);
    CHECK(y[0] == 0.25f && mn[0] == 9.0f && bad[0] == -1.0f);
    for (size_t i = 0; i < out.n; i++) CHECK(out[i] == 9.0f);
    CHECK(s2r_dynamics_reference(curve.p, 0.5f, 0.5f, nullptr, x.p, 3, y.p, out.p, mn.p) == S2R_OK);
    Buf table(S2R_DYN_CURVE_POINTS, 9.0f);
    CHECK(s2r_dynamics_curve(-20.0, 0.5, 0.0, 0.0, table.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_dynamics_curve(-20.0, 4.0, -1.0, 0.0, table.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_dynamics_curve(-20.0, 4.0, 0.0, 60.0, table.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_dynamics_curve((double)NAN, 4.0, 0.0, 0.0, table.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_dynamics_curve(-20.0, 4.0, 0.0, 0.0, nullptr) == S2R_ERR_INVALID);
    for (size_t i = 0; i < table.n; i++) CHECK(table[i] == 9.0f);
    CHECK(s2r_dynamics_curve(-20.0, (double)INFINITY, 0.0, 0.0, table.p) == S2R_OK);
    CHECK(table[0] == 1.0f && table[512] < 0.0004f && table[512] > 0.0003f);     // 0.1 / 256
    CHECK(std::isnan(s2r_dynamics_coef(-1.0, 48000.0)) && std::isnan(s2r_dynamics_coef(1.0, 0.0)));
}

}  // namespace

int main() {
    shapes();
    plain_answers();
    refusals();
    std::printf("dyn ok\n");
    return 0;
}
