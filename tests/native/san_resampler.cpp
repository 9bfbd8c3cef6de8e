// san_resampler.cpp — s2r_resampler_reference, s2r_resampler_count and s2r_resampler_design of csrc/s2r_rules.cpp under ASan + UBSan
// (tests/test_resampler_native.py) at the edges of their shapes — 1/1, 2/1, 1/2, 4/1, 1/4, 2/3, 147/160, 160/147, 147/320 and both ends of
// the table budget; T 4; calls of 0, 1, T - 2, T - 1, T and 1000 frames; 0, 3 and 8 buses; ph at 0 and at M - 1 —, every buffer allocated
// at exactly the size s2r.h states (the outputs at exactly the call's count), the answers that need no model, and refusals that touch
// nothing.  Built with -ffp-contract=off.  Prints "resampler ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "s2r.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "san_resampler.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

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

uint32_t rng_state = 24680u;
float noise() {                                  // in (-1, 1), never 0
    rng_state = rng_state * 1664525u + 1013904223u;
    return ((float)(rng_state >> 8) + 0.5f) / 8388608.0f - 1.0f;
}
void fill_noise(Buf &b, float amp) { for (size_t i = 0; i < b.n; i++) b[i] = amp * noise(); }
bool same_bits(const float *a, const float *b, size_t n) { return n == 0 || std::memcmp(a, b, n * sizeof(float)) == 0; }

struct Shape { uint32_t L, M, T; };
const Shape kShapes[] = {{1, 1, 4}, {2, 1, 32}, {1, 2, 64}, {4, 1, 8}, {1, 4, 16}, {2, 3, 48}, {147, 160, 32}, {160, 147, 32}, {147, 320, 64},
                         {192, 175, 128}, {320, 147, 76}};

// every shape: a stream in one call and the same stream in two calls leave the same outputs, state and ph; the count is
// s2r_resampler_count's; the history of a call of T - 1 frames or more is the call's last frames, newest first
void shapes() {
    for (const Shape &sh : kShapes) {
        const uint32_t L = sh.L, M = sh.M, T = sh.T, H = T - 1u;
        Buf table((size_t)L * T);
        CHECK(s2r_resampler_design(L, M, T, 10.0, 0.9, table.p) == S2R_OK);
        for (uint32_t p = 0; p < L; p++) {
            double sum = 0.0;
            for (uint32_t k = 0; k < T; k++) { CHECK(std::isfinite(table[(size_t)p * T + k]) && std::fabs(table[(size_t)p * T + k]) <= 4.0f); sum += table[(size_t)p * T + k]; }
            CHECK(std::fabs(sum - 1.0) < 1e-5);
        }
        for (uint32_t nb : {0u, 3u, 8u})
            for (uint32_t frames : {0u, 1u, T - 2u, T - 1u, T, 1000u})
                for (uint32_t ph0 : {0u, M - 1u}) {
                    if (frames == 1000u && nb == 3u) continue;   // (the long call: fewer shapes)
                    Buf stems((size_t)nb * frames * 2u), master((size_t)frames * 2u);
                    fill_noise(stems, 0.5f); fill_noise(master, 0.5f);
                    Buf st((size_t)S2R_RESAMPLER_STATE(T)), st2((size_t)S2R_RESAMPLER_STATE(T));
                    fill_noise(st, 0.7f);
                    for (size_t i = 0; i < st.n; i++) st2[i] = st[i];
                    size_t want = 99, made = 99;
                    CHECK(s2r_resampler_count(L, M, ph0, frames, &want) == S2R_OK && want <= S2R_RESAMPLER_MAX_OUT(frames, L, M));
                    Buf out((size_t)S2R_RESAMPLER_PROGRAMMES * want * 2u, 7.0f);
                    uint32_t ph = ph0;
                    CHECK(s2r_resampler_reference(L, M, T, table.p, nb ? stems.p : nullptr, nb, master.p, frames, st.p, &ph, out.p, want, &made) == S2R_OK);
                    CHECK(made == want && ph < M && (uint64_t)ph == (uint64_t)ph0 + (uint64_t)want * M - (uint64_t)frames * L);
                    if (frames >= H)
                        for (uint32_t j = 0; j < H; j++) CHECK(st[(size_t)16 * H + j] == master[(size_t)(frames - 1u - j) * 2u] && st[(size_t)17 * H + j] == master[(size_t)(frames - 1u - j) * 2u + 1u]);
                    // the same stream in two calls: the halves of every programme, gathered
                    const uint32_t fa = frames / 2u, fb = frames - fa;
                    Buf stems_a((size_t)nb * fa * 2u), stems_b((size_t)nb * fb * 2u);
                    for (uint32_t b = 0; b < nb; b++) {
                        for (size_t i = 0; i < (size_t)fa * 2u; i++) stems_a[(size_t)b * fa * 2u + i] = stems[(size_t)b * frames * 2u + i];
                        for (size_t i = 0; i < (size_t)fb * 2u; i++) stems_b[(size_t)b * fb * 2u + i] = stems[(size_t)b * frames * 2u + (size_t)fa * 2u + i];
                    }
                    size_t na = 99, nb2 = 99, got_a = 99, got_b = 99;
                    uint32_t ph2 = ph0;
                    CHECK(s2r_resampler_count(L, M, ph2, fa, &na) == S2R_OK);
                    Buf out_a((size_t)S2R_RESAMPLER_PROGRAMMES * na * 2u, 7.0f);
                    CHECK(s2r_resampler_reference(L, M, T, table.p, nb ? stems_a.p : nullptr, nb, master.p, fa, st2.p, &ph2, out_a.p, na, &got_a) == S2R_OK && got_a == na);
                    CHECK(s2r_resampler_count(L, M, ph2, fb, &nb2) == S2R_OK && na + nb2 == want);
                    Buf out_b((size_t)S2R_RESAMPLER_PROGRAMMES * nb2 * 2u, 7.0f);
                    CHECK(s2r_resampler_reference(L, M, T, table.p, nb ? stems_b.p : nullptr, nb, master.p + (size_t)fa * 2u, fb, st2.p, &ph2, out_b.p, nb2, &got_b) == S2R_OK && got_b == nb2);
                    CHECK(ph2 == ph && same_bits(st.p, st2.p, st.n));
                    for (uint32_t p = 0; p < S2R_RESAMPLER_PROGRAMMES; p++) {
                        CHECK(same_bits(out.p + (size_t)p * want * 2u, out_a.p + (size_t)p * na * 2u, na * 2u));
                        CHECK(same_bits(out.p + ((size_t)p * want + na) * 2u, out_b.p + (size_t)p * nb2 * 2u, nb2 * 2u));
                    }
                }
    }
}

// the identity table at 1/1 returns the input's bits; 4/1 makes four frames of one; 1/4 fed single frames mostly makes none
void answers() {
    const float id[4] = {1.0f, 0.0f, 0.0f, 0.0f};
    Buf stems((size_t)8 * 300 * 2u), master((size_t)300 * 2u), st((size_t)S2R_RESAMPLER_STATE(4)), out((size_t)9 * 300 * 2u, 7.0f);
    fill_noise(stems, 1.0f); fill_noise(master, 1.0f);
    uint32_t ph = 0;
    size_t made = 0;
    CHECK(s2r_resampler_reference(1, 1, 4, id, stems.p, 8, master.p, 300, st.p, &ph, out.p, 300, &made) == S2R_OK && made == 300 && ph == 0);
    CHECK(same_bits(out.p, stems.p, stems.n) && same_bits(out.p + (size_t)8 * 300 * 2u, master.p, master.n));
    Buf t4((size_t)4 * 8), st4((size_t)S2R_RESAMPLER_STATE(8)), one(2, 0.25f), four((size_t)9 * 4 * 2u, 7.0f);
    CHECK(s2r_resampler_design(4, 1, 8, 8.0, 0.9, t4.p) == S2R_OK);
    CHECK(s2r_resampler_reference(4, 1, 8, t4.p, nullptr, 0, one.p, 1, st4.p, &ph, four.p, 4, &made) == S2R_OK && made == 4 && ph == 0);
    for (size_t i = 0; i < (size_t)8 * 4 * 2u; i++) CHECK(four[i] == 0.0f && !std::signbit(four[i]));       // the buses: fed +0.0
    Buf t14((size_t)16), st14((size_t)S2R_RESAMPLER_STATE(16)), o14((size_t)9 * 2u, 7.0f);
    CHECK(s2r_resampler_design(1, 4, 16, 8.0, 0.9, t14.p) == S2R_OK);
    size_t total = 0, empty = 0;
    for (uint32_t f = 0; f < 41; f++) {
        one[0] = noise(); one[1] = noise();
        CHECK(s2r_resampler_reference(1, 4, 16, t14.p, nullptr, 0, one.p, 1, st14.p, &ph, o14.p, 1, &made) == S2R_OK && made <= 1 && ph < 4);
        total += made; empty += made == 0;
    }
    CHECK(total == 11 && empty == 30);
    // NaN and infinities pass through as the operations have them, and nothing else is touched by them
    Buf bad((size_t)20 * 2u), stb((size_t)S2R_RESAMPLER_STATE(4)), ob((size_t)9 * 20 * 2u);
    bad[10] = std::numeric_limits<float>::quiet_NaN(); bad[21] = std::numeric_limits<float>::infinity();
    ph = 0;
    CHECK(s2r_resampler_reference(1, 1, 4, id, nullptr, 0, bad.p, 20, stb.p, &ph, ob.p, 20, &made) == S2R_OK && made == 20);
    CHECK(std::isnan(ob[(size_t)8 * 20 * 2u + 10]) && std::isinf(ob[(size_t)8 * 20 * 2u + 21]) && std::isnan(ob[(size_t)8 * 20 * 2u + 23]) && ob[(size_t)8 * 20 * 2u + 30] == 0.0f);
}

// refusals touch nothing
void refusals() {
    Buf table((size_t)2 * 4, 0.25f), master((size_t)10 * 2u, 0.5f), st((size_t)S2R_RESAMPLER_STATE(4), 0.125f), out((size_t)9 * 7 * 2u, 7.0f);
    uint32_t ph = 1;
    size_t made = 77;
    const Shape bad[] = {{0, 1, 4}, {1, 0, 4}, {321, 320, 4}, {320, 321, 4}, {2, 4, 4}, {5, 1, 4}, {1, 5, 4}, {2, 3, 0}, {2, 3, 6}, {2, 3, 132}, {193, 175, 128}, {320, 147, 80}};
    for (const Shape &sh : bad) {
        CHECK(s2r_resampler_reference(sh.L, sh.M, sh.T, table.p, nullptr, 0, master.p, 10, st.p, &ph, out.p, 7, &made) == S2R_ERR_PATCH_RANGE);
        CHECK(s2r_resampler_design(sh.L, sh.M, sh.T, 10.0, 0.9, table.p) == S2R_ERR_PATCH_RANGE);
    }
    CHECK(s2r_resampler_count(2, 4, 0, 10, &made) == S2R_ERR_PATCH_RANGE && s2r_resampler_count(2, 3, 3, 10, &made) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_resampler_count(2, 3, 1, 10, nullptr) == S2R_ERR_INVALID);
    CHECK(s2r_resampler_reference(2, 3, 4, table.p, nullptr, 9, master.p, 10, st.p, &ph, out.p, 7, &made) == S2R_ERR_PATCH_RANGE);
    ph = 3;
    CHECK(s2r_resampler_reference(2, 3, 4, table.p, nullptr, 0, master.p, 10, st.p, &ph, out.p, 7, &made) == S2R_ERR_PATCH_RANGE);
    ph = 1;
    table[5] = 4.5f;
    CHECK(s2r_resampler_reference(2, 3, 4, table.p, nullptr, 0, master.p, 10, st.p, &ph, out.p, 7, &made) == S2R_ERR_PATCH_RANGE);
    table[5] = std::numeric_limits<float>::quiet_NaN();
    CHECK(s2r_resampler_reference(2, 3, 4, table.p, nullptr, 0, master.p, 10, st.p, &ph, out.p, 7, &made) == S2R_ERR_PATCH_RANGE);
    table[5] = 0.25f;
    CHECK(s2r_resampler_reference(2, 3, 4, nullptr, nullptr, 0, master.p, 10, st.p, &ph, out.p, 7, &made) == S2R_ERR_INVALID);
    CHECK(s2r_resampler_reference(2, 3, 4, table.p, nullptr, 0, nullptr, 10, st.p, &ph, out.p, 7, &made) == S2R_ERR_INVALID);
    CHECK(s2r_resampler_reference(2, 3, 4, table.p, nullptr, 2, master.p, 10, st.p, &ph, out.p, 7, &made) == S2R_ERR_INVALID);
    CHECK(s2r_resampler_reference(2, 3, 4, table.p, nullptr, 0, master.p, 10, nullptr, &ph, out.p, 7, &made) == S2R_ERR_INVALID);
    CHECK(s2r_resampler_reference(2, 3, 4, table.p, nullptr, 0, master.p, 10, st.p, nullptr, out.p, 7, &made) == S2R_ERR_INVALID);
    CHECK(s2r_resampler_reference(2, 3, 4, table.p, nullptr, 0, master.p, 10, st.p, &ph, out.p, 7, nullptr) == S2R_ERR_INVALID);
    CHECK(s2r_resampler_reference(2, 3, 4, table.p, nullptr, 0, master.p, 10, st.p, &ph, nullptr, 7, &made) == S2R_ERR_INVALID);
    CHECK(s2r_resampler_reference(2, 3, 4, table.p, nullptr, 0, master.p, 10, st.p, &ph, out.p, 6, &made) == S2R_ERR_INVALID);      // 10 frames at 2/3 from ph 1: 7 frames
    CHECK(s2r_resampler_design(2, 3, 4, -1.0, 0.9, table.p) == S2R_ERR_PATCH_RANGE && s2r_resampler_design(2, 3, 4, 21.0, 0.9, table.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_resampler_design(2, 3, 4, 10.0, 0.0, table.p) == S2R_ERR_PATCH_RANGE && s2r_resampler_design(2, 3, 4, 10.0, 1.5, table.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_resampler_design(2, 3, 4, std::nan(""), 0.9, table.p) == S2R_ERR_PATCH_RANGE && s2r_resampler_design(2, 3, 4, 10.0, 0.9, nullptr) == S2R_ERR_INVALID);
    CHECK(ph == 1 && made == 77);
    for (size_t i = 0; i < table.n; i++) CHECK(table[i] == 0.25f);
    for (size_t i = 0; i < st.n; i++) CHECK(st[i] == 0.125f);
    for (size_t i = 0; i < out.n; i++) CHECK(out[i] == 7.0f);
    CHECK(s2r_resampler_reference(2, 3, 4, table.p, nullptr, 0, master.p, 10, st.p, &ph, out.p, 7, &made) == S2R_OK && made == 7);
}

}  // namespace

int main() {
    shapes();
    answers();
    refusals();
    std::printf("resampler ok\n");
    return 0;
}
