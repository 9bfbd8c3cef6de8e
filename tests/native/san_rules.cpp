// san_rules.cpp — the handle-free rule functions of csrc/s2r_rules.cpp under ASan + UBSan (tests/test_rules_native.py): the three
// references at the edges of their ranges, every buffer allocated at exactly the size s2r.h states, and a few answers that need
// no model.  Built with -ffp-contract=off, so the sums written here round as the rules' do.  Prints "rules ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "s2r.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "san_rules.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

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

uint32_t rng_state = 12345u;
float noise() {                                  // in (-1, 1), never 0
    rng_state = rng_state * 1664525u + 1013904223u;
    return ((float)(rng_state >> 8) + 0.5f) / 8388608.0f - 1.0f;
}
void fill_noise(Buf &b, float scale = 1.0f) { for (size_t i = 0; i < b.n; i++) b[i] = noise() * scale; }

void reverb() {
    const uint32_t taps[] = {1u, S2R_IR_SEGMENT, S2R_IR_SEGMENT + 1u};
    const uint32_t frames[] = {0u, 1u, 300u};
    for (uint32_t K : taps)
        for (uint32_t N : frames) {
            Buf ir(K), line(K - 1u + N), out(N);
            fill_noise(ir); fill_noise(line);
            CHECK(s2r_reverb_reference(ir.p, K, line.p, N, 0.25f, 1.0f, N ? out.p : nullptr) == S2R_OK);
            for (uint32_t i = 0; i < N; i++) CHECK(std::isfinite(out[i]));
            // one tap of 1.0, dry 0, wet 1: the input, behind however much history the response asks for
            for (uint32_t k = 0; k < K; k++) ir[k] = k == 0 ? 1.0f : 0.0f;
            CHECK(s2r_reverb_reference(ir.p, K, line.p, N, 0.0f, 1.0f, N ? out.p : nullptr) == S2R_OK);
            for (uint32_t i = 0; i < N; i++) CHECK(out[i] == line[K - 1u + i]);
        }
    Buf one(1, 1.0f);
    CHECK(s2r_reverb_reference(one.p, 0, one.p, 1, 0.0f, 1.0f, one.p) == S2R_ERR_INVALID);
    CHECK(s2r_reverb_reference(one.p, 1, one.p, 1, 1.5f, 1.0f, one.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_reverb_reference(one.p, 1, one.p, 1, 0.0f, 1.0f, nullptr) == S2R_ERR_INVALID);
}

void master() {
    const uint32_t buses[] = {1u, S2R_MAX_BUSES};
    const uint32_t frames[] = {0u, 1u, 257u};
    for (uint32_t nb : buses)
        for (uint32_t N : frames) {
            const size_t ch = ((size_t)nb + 1u) * 2u;
            Buf stems((size_t)nb * N * 2u), r0(nb), r1(nb), lr(2u * (size_t)N), peak(ch), energy(ch);
            fill_noise(stems);
            for (uint32_t b = 0; b < nb; b++) { r0[b] = (float)(b + 1u) / (float)(2u * S2R_MAX_BUSES); r1[b] = 1.0f - r0[b]; }
            CHECK(s2r_master_reference(stems.p, nb, N, r0.p, r1.p, 0.25f, 1.0f, lr.p, peak.p, energy.p) == S2R_OK);
            for (size_t i = 0; i < lr.n; i++) CHECK(std::isfinite(lr[i]));
            for (size_t i = 0; i < ch; i++) CHECK(peak[i] >= 0.0f && energy[i] >= 0.0f && (N == 0 ? peak[i] == 0.0f : peak[i] > 0.0f));
            // every optional output null, one at a time and together
            CHECK(s2r_master_reference(stems.p, nb, N, r0.p, r1.p, 0.25f, 1.0f, nullptr, peak.p, nullptr) == S2R_OK);
            CHECK(s2r_master_reference(stems.p, nb, N, r0.p, r1.p, 0.25f, 1.0f, lr.p, nullptr, energy.p) == S2R_OK);
            CHECK(s2r_master_reference(stems.p, nb, N, r0.p, r1.p, 0.25f, 1.0f, nullptr, nullptr, nullptr) == S2R_OK);
            // returns and fader at 1: the sum in bus order from +0.0
            for (uint32_t b = 0; b < nb; b++) r0[b] = r1[b] = 1.0f;
            CHECK(s2r_master_reference(stems.p, nb, N, r0.p, r1.p, 1.0f, 1.0f, lr.p, nullptr, nullptr) == S2R_OK);
            for (size_t i = 0; i < 2u * (size_t)N; i++) {
                float t = 0.0f;
                for (uint32_t b = 0; b < nb; b++) t = t + stems[(size_t)b * N * 2u + i];
                CHECK(lr[i] == t);
            }
        }
    Buf one(2, 1.0f);
    CHECK(s2r_master_reference(one.p, 0, 1, one.p, one.p, 1.0f, 1.0f, one.p, nullptr, nullptr) == S2R_ERR_INVALID);
    CHECK(s2r_master_reference(one.p, S2R_MAX_BUSES + 1u, 1, one.p, one.p, 1.0f, 1.0f, one.p, nullptr, nullptr) == S2R_ERR_INVALID);
    CHECK(s2r_master_reference(one.p, 1, 1, one.p, one.p, 1.0f, 1.5f, one.p, nullptr, nullptr) == S2R_ERR_PATCH_RANGE);
}

void limiter() {
    const uint32_t looks[] = {1u, S2R_LIMITER_MAX_LOOKAHEAD}, holds[] = {0u, S2R_LIMITER_MAX_HOLD};
    const uint32_t frames[] = {0u, 1u, 300u};
    for (uint32_t L : looks)
        for (uint32_t H : holds) {
            const size_t G = 2u * (size_t)L + H;
            // over the ceiling, call after call from the state the last one left
            Buf xh(2u * (size_t)L), gh(G, 1.0f);
            for (uint32_t N : frames) {
                Buf x(2u * (size_t)N), y(2u * (size_t)N), gain(N);
                fill_noise(x);
                CHECK(s2r_limiter_reference(x.p, N, 0.25f, L, H, xh.p, gh.p, y.p, gain.p) == S2R_OK);
                for (size_t i = 0; i < y.n; i++) CHECK(std::fabs(y[i]) <= 0.25f);
                for (size_t i = 0; i < gain.n; i++) CHECK(gain[i] > 0.0f && gain[i] <= 1.0f);
                CHECK(s2r_limiter_reference(x.p, N, 0.25f, L, H, xh.p, gh.p, nullptr, gain.p) == S2R_OK);
                CHECK(s2r_limiter_reference(x.p, N, 0.25f, L, H, xh.p, gh.p, y.p, nullptr) == S2R_OK);
                CHECK(s2r_limiter_reference(N ? x.p : nullptr, N, 0.25f, L, H, xh.p, gh.p, nullptr, nullptr) == S2R_OK);
            }
            // under the ceiling, from the initial state: the input L frames late behind +0.0, every gain 1, the last L frames kept
            Buf xh0(2u * (size_t)L), gh0(G, 1.0f);
            size_t at = 0;
            std::vector<float> all;
            for (uint32_t N : frames) {
                Buf x(2u * (size_t)N), y(2u * (size_t)N), gain(N);
                fill_noise(x, 0.5f);
                CHECK(s2r_limiter_reference(x.p, N, 1.0f, L, H, xh0.p, gh0.p, y.p, gain.p) == S2R_OK);
                for (size_t i = 0; i < x.n; i++) all.push_back(x[i]);
                for (size_t i = 0; i < y.n; i++) {
                    const size_t j = at + i;
                    CHECK(gain[i / 2u] == 1.0f && y[i] == (j < 2u * (size_t)L ? 0.0f : all[j - 2u * (size_t)L]));
                }
                at += y.n;
            }
            for (size_t i = 0; i < xh0.n; i++) {
                const size_t back = xh0.n - i;           // floats before the end of the stream
                CHECK(xh0[i] == (back <= all.size() ? all[all.size() - back] : 0.0f));
            }
            for (size_t i = 0; i < gh0.n; i++) CHECK(gh0[i] == 1.0f);
        }
    Buf one(8, 1.0f);
    CHECK(s2r_limiter_reference(one.p, 1, 0.25f, 0, 0, one.p, one.p, nullptr, nullptr) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_limiter_reference(one.p, 1, 0.25f, S2R_LIMITER_MAX_LOOKAHEAD + 1u, 0, one.p, one.p, nullptr, nullptr) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_limiter_reference(one.p, 1, 0.25f, 1, S2R_LIMITER_MAX_HOLD + 1u, one.p, one.p, nullptr, nullptr) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_limiter_reference(one.p, 1, 0.25f, 1, 0, nullptr, one.p, nullptr, nullptr) == S2R_ERR_INVALID);
}

// the gains of the mixer: the ends of their ranges, null outputs
void gains() {
    float l = -1.0f, r = -1.0f;
    s2r_pan_gains(-1.0f, &l, &r); CHECK(l == 1.0f && r == 0.0f);
    s2r_pan_gains(1.0f, &l, nullptr); CHECK(l == 0.0f);
    s2r_pan_gains(0.0f, nullptr, &r); CHECK(r == std::sqrt(0.5f));
    s2r_pan_gains(0.0f, nullptr, nullptr);
    CHECK(s2r_voice_pan(1.0f, 1.0f, 127) == 1.0f && s2r_voice_pan(-1.0f, 1.0f, 0) == -1.0f && s2r_voice_pan(0.25f, 0.5f, 64) == 0.25f);
    CHECK(s2r_voice_gain(0.5f, 0.0f, 0.0f) == 0.5f && s2r_voice_gain(1.0f, 1.0f, 0.0f) == 0.0f && s2r_voice_gain(1.0f, 1.0f, NAN) == 1.0f);
    CHECK(s2r_send_gain(0.5f, 0.5f) == 0.25f);
    s2r_fader_gains(0.0f, 0.5f, 1.0f, 0.0f, &l, &r); CHECK(l == std::sqrt(0.5f) * 0.5f && r == l);
    s2r_fader_gains(0.5f, 1.0f, 0.5f, 2.0f, &l, nullptr); CHECK(l == 0.0f);
    s2r_fader_gains(0.5f, 1.0f, 0.5f, -2.0f, nullptr, &r); CHECK(r == 0.0f);
}

}  // namespace

int main() {
    reverb();
    master();
    limiter();
    gains();
    std::printf("rules ok\n");
    return 0;
}
