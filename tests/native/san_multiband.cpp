// san_multiband.cpp — s2r_multiband_reference and s2r_multiband_design of csrc/s2r_rules.cpp under ASan + UBSan
// (tests/test_multiband_native.py) at 1 .. 4 bands and calls of 0, 1, 9 and 500 frames, every buffer allocated at exactly the size
// s2r.h states — lp and hp [B - 1][5], ap [B - 2][5], curves [B][513], state [S2R_MULTIBAND_STATE(B)], bands [B][frames][2], minima [B],
// arrays of no rows as NULL —, the answers that need no model (a stream in one call and in several leaves the same bits; unit curves
// leave gains of exactly 1), and refusals that touch nothing.  Built with -ffp-contract=off.  Prints "multiband ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "s2r.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "san_multiband.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

// a heap block of exactly n floats; n == 0: null, as s2r.h accepts for an array of no rows
struct Buf {
    float *p;
    size_t n;
    explicit Buf(size_t n_, float fill = 0.0f) : p(n_ ? new float[n_] : nullptr), n(n_) { for (size_t i = 0; i < n; i++) p[i] = fill; }
    ~Buf() { delete[] p; }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    float &operator[](size_t i) { return p[i]; }
};

uint32_t rng_state = 24680u;
float noise() {                                  // in (-1, 1), never 0
    rng_state = rng_state * 1664525u + 1013904223u;
    return ((float)(rng_state >> 8) + 0.5f) / 8388608.0f - 1.0f;
}
bool same_bits(const float *a, const float *b, size_t n) { return n == 0 || std::memcmp(a, b, n * sizeof(float)) == 0; }

const double kSplits[3] = {200.0, 1500.0, 6000.0};
const uint32_t kCalls[] = {0, 1, 9, 500};

// the crossover of B bands in blocks of exactly their sizes
struct Rows {
    Buf lp, hp, ap;
    explicit Rows(uint32_t B) : lp((size_t)(B - 1u) * 5u, 9.0f), hp((size_t)(B - 1u) * 5u, 9.0f), ap(B >= 2u ? (size_t)(B - 2u) * 5u : 0u, 9.0f) {
        CHECK(s2r_multiband_design(48000.0, B > 1u ? kSplits : nullptr, B - 1u, lp.p, hp.p, ap.p) == S2R_OK);
        for (size_t i = 0; i < lp.n; i++) CHECK(std::isfinite(lp[i]) && lp[i] != 9.0f && std::isfinite(hp[i]) && hp[i] != 9.0f);
        for (size_t i = 0; i < ap.n; i++) CHECK(std::isfinite(ap[i]) && ap[i] != 9.0f);
    }
};

void initial(Buf &state, uint32_t B, Buf &curves) {
    for (size_t i = 0; i < state.n; i++) state[i] = 0.0f;
    for (uint32_t j = 0; j < B; j++) state[state.n - B + j] = curves[(size_t)j * S2R_DYN_CURVE_POINTS];
}

void shapes() {
    for (uint32_t B = 1; B <= S2R_MULTIBAND_MAX_BANDS; B++) {
        const uint32_t N = 510;
        Rows r(B);
        Buf curves((size_t)B * S2R_DYN_CURVE_POINTS), att(B), rel(B);
        for (uint32_t j = 0; j < B; j++) {
            CHECK(s2r_dynamics_curve(-30.0 + 3.0 * j, 4.0, 6.0, 0.0, curves.p + (size_t)j * S2R_DYN_CURVE_POINTS) == S2R_OK);
            att[j] = s2r_dynamics_coef(1.0 + j, 48000.0); rel[j] = s2r_dynamics_coef(40.0, 48000.0);
        }
        Buf x((size_t)N * 2u);
        for (size_t i = 0; i < x.n; i++) x[i] = 0.8f * noise();
        Buf state(S2R_MULTIBAND_STATE(B)), out((size_t)N * 2u, 7.0f), bands((size_t)B * N * 2u, 7.0f), mn(B, 7.0f);
        const size_t sizes[4] = {1, 18, 39, 64};                 // 4 S(B) + B
        CHECK(state.n == sizes[B - 1u]);
        initial(state, B, curves);
        CHECK(s2r_multiband_reference(B, r.lp.p, r.hp.p, r.ap.p, curves.p, att.p, rel.p, x.p, N, state.p, out.p, bands.p, mn.p) == S2R_OK);
        for (size_t i = 0; i < out.n; i++) CHECK(std::isfinite(out[i]) && out[i] != 7.0f);
        for (size_t i = 0; i < bands.n; i++) CHECK(std::isfinite(bands[i]) && bands[i] != 7.0f);
        for (uint32_t j = 0; j < B; j++) CHECK(mn[j] > 0.0f && mn[j] < 1.0f && state[state.n - B + j] >= mn[j]);
        // the calls in a row from the initial state, on blocks of their own sizes, with null optional outputs in between
        Buf state2(S2R_MULTIBAND_STATE(B));
        initial(state2, B, curves);
        uint32_t at = 0;
        for (uint32_t frames : kCalls) {
            Buf seg((size_t)frames * 2u), o((size_t)frames * 2u, 7.0f), bd((size_t)B * frames * 2u, 7.0f), m(B, 7.0f);
            for (size_t i = 0; i < seg.n; i++) seg[i] = x[(size_t)at * 2u + i];
            CHECK(s2r_multiband_reference(B, r.lp.p, r.hp.p, r.ap.p, curves.p, att.p, rel.p, seg.p, frames, state2.p, o.p, frames == 9u ? nullptr : bd.p,
                                          frames == 1u ? nullptr : m.p) == S2R_OK);
            CHECK(same_bits(o.p, out.p + (size_t)at * 2u, o.n));
            if (frames != 9u)
                for (uint32_t j = 0; j < B; j++) CHECK(same_bits(bd.p + (size_t)j * frames * 2u, bands.p + ((size_t)j * N + at) * 2u, (size_t)frames * 2u));
            if (frames == 0u) for (uint32_t j = 0; j < B; j++) CHECK(m[j] == 7.0f);         // no frames: the minima are not written
            at += frames;
        }
        CHECK(at == N && same_bits(state.p, state2.p, state.n));
        // unit curves and no retention: every gain exactly 1
        Buf unit((size_t)B * S2R_DYN_CURVE_POINTS, 1.0f), zero(B), state3(S2R_MULTIBAND_STATE(B)), mn3(B, 7.0f);
        initial(state3, B, unit);
        CHECK(s2r_multiband_reference(B, r.lp.p, r.hp.p, r.ap.p, unit.p, zero.p, zero.p, x.p, N, state3.p, nullptr, nullptr, mn3.p) == S2R_OK);
        for (uint32_t j = 0; j < B; j++) CHECK(mn3[j] == 1.0f && state3[state3.n - B + j] == 1.0f);
    }
}

void refusals() {
    const uint32_t B = 3;
    Rows r(B);
    Buf curves((size_t)B * S2R_DYN_CURVE_POINTS, 0.5f), att(B, 0.5f), rel(B, 0.25f), x(8, 0.5f), state(S2R_MULTIBAND_STATE(B), 0.125f), out(8, 7.0f), mn(B, 7.0f);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    auto run = [&](uint32_t n_bands) { return s2r_multiband_reference(n_bands, r.lp.p, r.hp.p, r.ap.p, curves.p, att.p, rel.p, x.p, 4, state.p, out.p, nullptr, mn.p); };
    CHECK(run(0) == S2R_ERR_PATCH_RANGE && run(5) == S2R_ERR_PATCH_RANGE);
    { const float keep = r.hp[4]; r.hp[4] = 1.0f; CHECK(run(B) == S2R_ERR_PATCH_RANGE); r.hp[4] = keep; }
    { const float keep = r.ap[0]; r.ap[0] = nan; CHECK(run(B) == S2R_ERR_PATCH_RANGE); r.ap[0] = keep; }
    { curves[2u * S2R_DYN_CURVE_POINTS + 512u] = 300.0f; CHECK(run(B) == S2R_ERR_PATCH_RANGE); curves[2u * S2R_DYN_CURVE_POINTS + 512u] = 0.5f; }
    { att[2] = 1.0f; CHECK(run(B) == S2R_ERR_PATCH_RANGE); att[2] = 0.5f; }
    { state[state.n - 1u] = -1.0f; CHECK(run(B) == S2R_ERR_PATCH_RANGE); state[state.n - 1u] = 0.125f; }
    CHECK(s2r_multiband_reference(B, nullptr, r.hp.p, r.ap.p, curves.p, att.p, rel.p, x.p, 4, state.p, out.p, nullptr, mn.p) == S2R_ERR_INVALID);
    CHECK(s2r_multiband_reference(B, r.lp.p, r.hp.p, nullptr, curves.p, att.p, rel.p, x.p, 4, state.p, out.p, nullptr, mn.p) == S2R_ERR_INVALID);
    CHECK(s2r_multiband_reference(B, r.lp.p, r.hp.p, r.ap.p, curves.p, att.p, rel.p, nullptr, 4, state.p, out.p, nullptr, mn.p) == S2R_ERR_INVALID);
    CHECK(s2r_multiband_reference(B, r.lp.p, r.hp.p, r.ap.p, curves.p, att.p, rel.p, x.p, 4, nullptr, out.p, nullptr, mn.p) == S2R_ERR_INVALID);
    for (size_t i = 0; i < state.n; i++) CHECK(state[i] == 0.125f);
    for (size_t i = 0; i < out.n; i++) CHECK(out[i] == 7.0f);
    for (size_t i = 0; i < mn.n; i++) CHECK(mn[i] == 7.0f);
    CHECK(run(B) == S2R_OK);
    // the design: frequencies out of order or out of range, too many splits, null rows; what it refuses it leaves alone
    Buf lp(15, 3.0f), hp(15, 3.0f), ap(10, 3.0f);
    const double down[2] = {900.0, 300.0}, edge[1] = {24000.0}, four[4] = {100.0, 200.0, 300.0, 400.0}, bad[1] = {std::numeric_limits<double>::quiet_NaN()};
    CHECK(s2r_multiband_design(48000.0, down, 2, lp.p, hp.p, ap.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_multiband_design(48000.0, edge, 1, lp.p, hp.p, ap.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_multiband_design(48000.0, four, 4, lp.p, hp.p, ap.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_multiband_design(48000.0, bad, 1, lp.p, hp.p, ap.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_multiband_design(0.0, kSplits, 1, lp.p, hp.p, ap.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_multiband_design(48000.0, kSplits, 2, lp.p, hp.p, nullptr) == S2R_ERR_INVALID);
    CHECK(s2r_multiband_design(48000.0, nullptr, 1, lp.p, hp.p, ap.p) == S2R_ERR_INVALID);
    for (size_t i = 0; i < lp.n; i++) CHECK(lp[i] == 3.0f && hp[i] == 3.0f);
    for (size_t i = 0; i < ap.n; i++) CHECK(ap[i] == 3.0f);
    CHECK(s2r_multiband_design(48000.0, nullptr, 0, nullptr, nullptr, nullptr) == S2R_OK);
}

}  // namespace

int main() {
    shapes();
    refusals();
    std::printf("multiband ok\n");
    return 0;
}
