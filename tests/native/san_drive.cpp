// san_drive.cpp — s2r_drive_reference, s2r_drive_taps and s2r_drive_curve of csrc/s2r_rules.cpp under ASan + UBSan
// (tests/test_drive_native.py) at the edges of their shapes — no frames, one, 31, 32, 33, a thousand; every curve kind, a table of
// huge entries, pre at both ends; no output buffer; in place — every buffer allocated at exactly the size s2r.h states, the answers
// that need no model, and the range checks.  Built with -ffp-contract=off.  Prints "drive ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "s2r.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "san_drive.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

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
void fill_noise(Buf &b, float scale = 1.0f) { for (size_t i = 0; i < b.n; i++) b[i] = noise() * scale; }
bool same_bits(const float *a, const float *b, size_t n) { return n == 0 || std::memcmp(a, b, n * sizeof(float)) == 0; }

constexpr size_t kHist = 2u * S2R_DRIVE_HISTORY, kPoints = S2R_DRIVE_CURVE_POINTS;

// every shape on exact buffers; one call equals two, on bits; a null output moves the history on all the same
void shapes() {
    const uint32_t frames[] = {0u, 1u, 31u, 32u, 33u, 1000u};
    const float pres[] = {0.0f, 0.75f, 3.0f, 1024.0f};
    for (uint32_t kind = 0; kind <= 5u; kind++) {
        Buf curve(kPoints);
        if (kind < 5u) CHECK(s2r_drive_curve(kind, 2.5, curve.p) == S2R_OK);
        else { fill_noise(curve, 3.0e38f); }                     // finite, and as large as a table may be
        for (size_t i = 0; i < kPoints; i++) CHECK(std::isfinite(curve[i]));
        for (uint32_t N : frames)
            for (float pre : pres) {
                Buf x(2u * (size_t)N), out(2u * (size_t)N), h(kHist), h2(kHist), h3(kHist), before(kHist);
                fill_noise(x); fill_noise(h, 0.25f);
                std::memcpy(h2.p, h.p, kHist * sizeof(float)); std::memcpy(h3.p, h.p, kHist * sizeof(float)); std::memcpy(before.p, h.p, kHist * sizeof(float));
                CHECK(s2r_drive_reference(curve.p, pre, 0.5f, 0.75f, N ? x.p : nullptr, N, h.p, N ? out.p : nullptr) == S2R_OK);
                for (size_t i = 0; i < kHist; i++) CHECK(std::isfinite(h[i]));
                CHECK(s2r_drive_reference(curve.p, pre, 0.5f, 0.75f, N ? x.p : nullptr, N, h2.p, nullptr) == S2R_OK);
                CHECK(same_bits(h.p, h2.p, kHist));
                if (N == 0) { CHECK(same_bits(h.p, before.p, kHist)); continue; }
                // the history is the last 32 frames of history ++ call
                for (size_t k = 0; k < S2R_DRIVE_HISTORY; k++)
                    for (size_t c = 0; c < 2u; c++) {
                        const size_t at = (size_t)N + k;         // entry of history ++ call
                        const float want = at < S2R_DRIVE_HISTORY ? before[2u * at + c] : x[2u * (at - S2R_DRIVE_HISTORY) + c];
                        CHECK(same_bits(&h[2u * k + c], &want, 1));
                    }
                const uint32_t cut = N / 2u;                 // (0 for one frame: an empty first call)
                Buf a(2u * (size_t)cut), b(2u * (size_t)(N - cut)), xa(2u * (size_t)cut), xb(2u * (size_t)(N - cut));
                for (size_t i = 0; i < xa.n; i++) xa[i] = x[i];
                for (size_t i = 0; i < xb.n; i++) xb[i] = x[xa.n + i];
                CHECK(s2r_drive_reference(curve.p, pre, 0.5f, 0.75f, cut ? xa.p : nullptr, cut, h3.p, cut ? a.p : nullptr) == S2R_OK);
                CHECK(s2r_drive_reference(curve.p, pre, 0.5f, 0.75f, xb.p, N - cut, h3.p, b.p) == S2R_OK);
                CHECK(same_bits(a.p, out.p, a.n) && same_bits(b.p, out.p + a.n, b.n) && same_bits(h3.p, h.p, kHist));
            }
    }
}

// no model: wet 0 and dry 1 give the input 16 frames late; in place is the same; the taps are symmetric and sum to one
void plain_answers() {
    const uint32_t N = 200;
    Buf lin(kPoints), x(2u * N), out(2u * N), h(kHist), all(kHist + 2u * N);
    CHECK(s2r_drive_curve(S2R_DRIVE_LINEAR, 0.0, lin.p) == S2R_OK);
    CHECK(lin[0] == -1.0f && lin[512] == 0.0f && lin[1024] == 1.0f && lin[513] == 1.0f / 512.0f);
    fill_noise(x); fill_noise(h, 0.25f);
    std::memcpy(all.p, h.p, kHist * sizeof(float)); std::memcpy(all.p + kHist, x.p, x.n * sizeof(float));
    CHECK(s2r_drive_reference(lin.p, 4.0f, 1.0f, 0.0f, x.p, N, h.p, out.p) == S2R_OK);
    for (size_t i = 0; i < out.n; i++) CHECK(out[i] == all[i + 2u * (S2R_DRIVE_HISTORY - S2R_DRIVE_LATENCY)]);
    Buf in_place(2u * N), h2(kHist), h3(kHist), out2(2u * N);
    std::memcpy(h2.p, all.p, kHist * sizeof(float)); std::memcpy(h3.p, all.p, kHist * sizeof(float));
    for (size_t i = 0; i < x.n; i++) in_place[i] = x[i];
    CHECK(s2r_drive_reference(lin.p, 4.0f, 0.5f, 0.5f, x.p, N, h2.p, out2.p) == S2R_OK);
    CHECK(s2r_drive_reference(lin.p, 4.0f, 0.5f, 0.5f, in_place.p, N, h3.p, in_place.p) == S2R_OK);
    CHECK(same_bits(in_place.p, out2.p, out2.n) && same_bits(h3.p, h2.p, kHist));
    Buf taps(S2R_DRIVE_TAPS);
    CHECK(s2r_drive_taps(taps.p) == S2R_OK && s2r_drive_taps(nullptr) == S2R_ERR_INVALID);
    double sum = 0.0;
    for (size_t k = 0; k < S2R_DRIVE_TAPS; k++) { CHECK(same_bits(&taps[k], &taps[S2R_DRIVE_TAPS - 1u - k], 1)); sum += (double)taps[k]; }
    CHECK(std::fabs(sum - 1.0) <= 65.0 * std::ldexp(1.0, -24));
}

// a refusal touches nothing
void refusals() {
    Buf lin(kPoints), x(6), out(6, 9.0f), h(kHist, 0.25f), t(kPoints, 9.0f);
    CHECK(s2r_drive_curve(S2R_DRIVE_LINEAR, 1.0, lin.p) == S2R_OK);
    fill_noise(x);
    const float good[3] = {1.0f, 0.5f, 0.5f};
    const float wrong[3][3] = {{-0.5f, 1024.5f, NAN}, {-0.5f, 1.5f, NAN}, {-0.5f, 1.5f, INFINITY}};
    for (int k = 0; k < 3; k++)
        for (float v : wrong[k]) {
            float l[3];
            std::memcpy(l, good, sizeof l);
            l[k] = v;
            CHECK(s2r_drive_reference(lin.p, l[0], l[1], l[2], x.p, 3, h.p, out.p) == S2R_ERR_PATCH_RANGE);
        }
    for (size_t at : {(size_t)0, (size_t)512, kPoints - 1u})
        for (float v : {(float)NAN, (float)INFINITY, -(float)INFINITY}) {
            Buf bad(kPoints);
            std::memcpy(bad.p, lin.p, kPoints * sizeof(float));
            bad[at] = v;
            CHECK(s2r_drive_reference(bad.p, 1.0f, 0.5f, 0.5f, x.p, 3, h.p, out.p) == S2R_ERR_PATCH_RANGE);
        }
    Buf inf(kHist, 0.25f);
    inf[kHist - 1u] = INFINITY;
    CHECK(s2r_drive_reference(lin.p, 1.0f, 0.5f, 0.5f, x.p, 3, inf.p, out.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_drive_reference(nullptr, 1.0f, 0.5f, 0.5f, x.p, 3, h.p, out.p) == S2R_ERR_INVALID);
    CHECK(s2r_drive_reference(lin.p, 1.0f, 0.5f, 0.5f, nullptr, 3, h.p, out.p) == S2R_ERR_INVALID);
    CHECK(s2r_drive_reference(lin.p, 1.0f, 0.5f, 0.5f, x.p, 3, nullptr, out.p) == S2R_ERR_INVALID);
    for (size_t i = 0; i < kHist; i++) CHECK(h[i] == 0.25f);
    for (size_t i = 0; i < out.n; i++) CHECK(out[i] == 9.0f);
    CHECK(s2r_drive_reference(lin.p, 1.0f, 0.5f, 0.5f, x.p, 3, h.p, out.p) == S2R_OK);
    // the designed curves
    for (uint32_t kind : {5u, 99u}) CHECK(s2r_drive_curve(kind, 1.0, t.p) == S2R_ERR_PATCH_RANGE);
    for (uint32_t kind = S2R_DRIVE_TANH; kind <= S2R_DRIVE_FOLD; kind++) {
        for (double a : {0.0, -1.0, 0.015, 64.5, (double)NAN, (double)INFINITY}) CHECK(s2r_drive_curve(kind, a, t.p) == S2R_ERR_PATCH_RANGE);
        CHECK(s2r_drive_curve(kind, 1.0, nullptr) == S2R_ERR_INVALID);
    }
    for (size_t i = 0; i < kPoints; i++) CHECK(t[i] == 9.0f);
    for (uint32_t kind = S2R_DRIVE_TANH; kind <= S2R_DRIVE_FOLD; kind++)
        for (double a : {S2R_DRIVE_MIN_AMOUNT, S2R_DRIVE_MAX_AMOUNT}) {
            CHECK(s2r_drive_curve(kind, a, t.p) == S2R_OK);
            for (size_t i = 0; i < kPoints; i++) CHECK(t[i] >= -1.0f && t[i] <= 1.0f);
            CHECK(t[512] == 0.0f);
        }
}

}  // namespace

int main() {
    shapes();
    plain_answers();
    refusals();
    std::printf("drive ok\n");
    return 0;
}
