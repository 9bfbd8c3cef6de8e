// san_limiter_tp.cpp — s2r_limiter_tp_reference of csrc/s2r_rules.cpp under ASan + UBSan (tests/test_limiter_tp_native.py) at the edges
// of its shapes — the pairs (1, 0), (48, 0) and (1024, 4096); calls of 0, 1, 9 and 1000 frames —, every buffer allocated at exactly the
// size s2r.h states, the answers that need no model (the ceiling holds; the delay of L + 8 in every bit; a stream in one call and in
// several leaves the same bits), and refusals that touch nothing.  Built with -ffp-contract=off.  Prints "limiter tp ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "s2r.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "san_limiter_tp.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

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

uint32_t rng_state = 13579u;
float noise() {                                  // in (-1, 1), never 0
    rng_state = rng_state * 1664525u + 1013904223u;
    return ((float)(rng_state >> 8) + 0.5f) / 8388608.0f - 1.0f;
}
void fill_noise(Buf &b, float amp) { for (size_t i = 0; i < b.n; i++) b[i] = amp * noise(); }
bool same_bits(const float *a, const float *b, size_t n) { return n == 0 || std::memcmp(a, b, n * sizeof(float)) == 0; }

struct Pair { uint32_t L, H; };
const Pair kPairs[] = {{1, 0}, {48, 0}, {1024, 4096}};
const uint32_t kCalls[] = {0, 1, 9, 1000};

// every pair: the four calls in a row from the initial state against the same 1010 frames in one call; the ceiling holds
void shapes() {
    for (const Pair &pr : kPairs) {
        const uint32_t L = pr.L, H = pr.H, G = 2u * L + H, X = L + S2R_LIMITER_TP_HISTORY, N = 1010;
        const float c = 0.25f;
        Buf x((size_t)N * 2u);
        fill_noise(x, 0.9f);
        Buf xh((size_t)X * 2u), gh(G, 1.0f), y((size_t)N * 2u, 7.0f), gain(N, 7.0f);
        CHECK(s2r_limiter_tp_reference(x.p, N, c, L, H, xh.p, gh.p, y.p, gain.p) == S2R_OK);
        size_t limited = 0;
        for (uint32_t n = 0; n < N; n++) {
            CHECK(gain[n] > 0.0f && gain[n] <= 1.0f && std::fabs(y[2u * n]) <= c && std::fabs(y[2u * n + 1u]) <= c);
            limited += gain[n] < 1.0f;
        }
        CHECK(limited > N / 4u);
        if (N >= X) CHECK(same_bits(xh.p, x.p + (size_t)(N - X) * 2u, (size_t)X * 2u));       // the call's last L + 16 frames
        Buf xh2((size_t)X * 2u), gh2(G, 1.0f);
        uint32_t at = 0;
        for (uint32_t frames : kCalls) {
            Buf seg((size_t)frames * 2u), ys((size_t)frames * 2u, 7.0f), gs(frames, 7.0f);
            for (size_t i = 0; i < seg.n; i++) seg[i] = x[(size_t)at * 2u + i];
            CHECK(s2r_limiter_tp_reference(seg.p, frames, c, L, H, xh2.p, gh2.p, ys.p, gs.p) == S2R_OK);
            CHECK(same_bits(ys.p, y.p + (size_t)at * 2u, ys.n) && same_bits(gs.p, gain.p + at, gs.n));
            at += frames;
        }
        CHECK(at == N && same_bits(xh.p, xh2.p, xh.n) && same_bits(gh.p, gh2.p, gh.n));
        // the outputs may be null, and y may be x
        Buf xh3((size_t)X * 2u), gh3(G, 1.0f), xh4((size_t)X * 2u), gh4(G, 1.0f);
        CHECK(s2r_limiter_tp_reference(x.p, N, c, L, H, xh3.p, gh3.p, nullptr, nullptr) == S2R_OK && same_bits(xh.p, xh3.p, xh.n) && same_bits(gh.p, gh3.p, gh.n));
        Buf in_place((size_t)N * 2u);
        for (size_t i = 0; i < x.n; i++) in_place[i] = x[i];
        CHECK(s2r_limiter_tp_reference(in_place.p, N, c, L, H, xh4.p, gh4.p, in_place.p, nullptr) == S2R_OK && same_bits(in_place.p, y.p, y.n));
    }
}

// under a ceiling the interpolation never exceeds: the input L + 8 frames late in every bit, behind +0.0, the gains exactly 1
void delay() {
    for (const Pair &pr : kPairs) {
        const uint32_t L = pr.L, H = pr.H, G = 2u * L + H, X = L + S2R_LIMITER_TP_HISTORY, D = L + S2R_LIMITER_TP_LATENCY, N = 1200;
        Buf x((size_t)N * 2u), xh((size_t)X * 2u), gh(G, 1.0f), y((size_t)N * 2u, 7.0f), gain(N, 7.0f);
        fill_noise(x, 0.9f);
        CHECK(s2r_limiter_tp_reference(x.p, N, 16.0f, L, H, xh.p, gh.p, y.p, gain.p) == S2R_OK);
        for (uint32_t n = 0; n < N; n++) CHECK(gain[n] == 1.0f);
        for (size_t i = 0; i < (size_t)(D < N ? D : N) * 2u; i++) CHECK(y[i] == 0.0f && !std::signbit(y[i]));
        if (N > D) CHECK(same_bits(y.p + (size_t)D * 2u, x.p, (size_t)(N - D) * 2u));
        for (size_t i = 0; i < gh.n; i++) CHECK(gh[i] == 1.0f);
    }
}

// refusals touch nothing
void refusals() {
    Buf x((size_t)4 * 2u, 0.5f), xh((size_t)(4 + S2R_LIMITER_TP_HISTORY) * 2u, 0.125f), gh(9, 0.75f), y((size_t)4 * 2u, 7.0f), gain(4, 7.0f);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (float c : {nan, inf, -0.25f, 0.0f, std::ldexp(1.0f, -21), std::ldexp(1.0f, 21)})
        CHECK(s2r_limiter_tp_reference(x.p, 4, c, 4, 1, xh.p, gh.p, y.p, gain.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_limiter_tp_reference(x.p, 4, 0.25f, 0, 1, xh.p, gh.p, y.p, gain.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_limiter_tp_reference(x.p, 4, 0.25f, 1025, 1, xh.p, gh.p, y.p, gain.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_limiter_tp_reference(x.p, 4, 0.25f, 4, 4097, xh.p, gh.p, y.p, gain.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_limiter_tp_reference(nullptr, 4, 0.25f, 4, 1, xh.p, gh.p, y.p, gain.p) == S2R_ERR_INVALID);
    CHECK(s2r_limiter_tp_reference(x.p, 4, 0.25f, 4, 1, nullptr, gh.p, y.p, gain.p) == S2R_ERR_INVALID);
    CHECK(s2r_limiter_tp_reference(x.p, 4, 0.25f, 4, 1, xh.p, nullptr, y.p, gain.p) == S2R_ERR_INVALID);
    CHECK(s2r_limiter_tp_reference(nullptr, 0, 0.25f, 4, 1, xh.p, gh.p, nullptr, nullptr) == S2R_OK);          // no frames: nothing moves
    for (size_t i = 0; i < xh.n; i++) CHECK(xh[i] == 0.125f);
    for (size_t i = 0; i < gh.n; i++) CHECK(gh[i] == 0.75f);
    for (size_t i = 0; i < y.n; i++) CHECK(y[i] == 7.0f);
    for (size_t i = 0; i < gain.n; i++) CHECK(gain[i] == 7.0f);
}

}  // namespace

int main() {
    shapes();
    delay();
    refusals();
    std::printf("limiter tp ok\n");
    return 0;
}
