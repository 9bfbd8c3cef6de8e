// san_loudness.cpp — s2r_loudness_reference, s2r_loudness_readings and s2r_loudness_design of csrc/s2r_rules.cpp under ASan + UBSan
// (tests/test_loudness_native.py) at the edges of their shapes — hops 16, 17, 48 and 4800; calls of 0, 1, 15, 16, 17 frames and of many
// hops; 0, 2 and 8 buses; fewer than 4 and fewer than 30 hop rows —, every buffer allocated at exactly the size s2r.h states, the
// answers that need no model, and refusals that touch nothing.  Built with -ffp-contract=off.  Prints "loudness ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "s2r.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "san_loudness.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

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

uint32_t rng_state = 97531u;
float noise() {                                  // in (-1, 1), never 0
    rng_state = rng_state * 1664525u + 1013904223u;
    return ((float)(rng_state >> 8) + 0.5f) / 8388608.0f - 1.0f;
}
void fill_noise(Buf &b, float scale = 1.0f) { for (size_t i = 0; i < b.n; i++) b[i] = noise() * scale; }

constexpr size_t CH = S2R_LOUDNESS_CHANNELS, ST = S2R_LOUDNESS_STATE;

// every shape: the rows buffer holds exactly the rows the call completes, the position moves by the frames, a stream in one call and
// the same stream in two calls leave the same rows and state, a bus past the call's stays on zeros
void shapes() {
    Buf c(10);
    CHECK(s2r_loudness_design(48000.0, c.p) == S2R_OK);
    const uint32_t hops[] = {16u, 17u, 48u, 4800u}, calls[] = {0u, 1u, 15u, 16u, 17u, 9601u}, buses[] = {0u, 2u, 8u};
    for (uint32_t hop : hops)
        for (uint32_t N : calls)
            for (uint32_t nb : buses)
                for (uint32_t pos0 : {0u, hop - 1u}) {
                    Buf stems(2u * (size_t)nb * N), master(2u * (size_t)N), state(ST), state2(ST);
                    fill_noise(stems, 0.25f); fill_noise(master, 0.5f); fill_noise(state, 0.01f);
                    for (size_t q = 0; q < CH; q++) state[72 + q] = std::fabs(state[72 + q]);       // a partial sum of squares is not negative
                    for (size_t i = 0; i < ST; i++) state2[i] = state[i];
                    const size_t made = ((size_t)pos0 + N) / hop;
                    Buf rows(made * CH, -1.0f), rows2(made * CH, -1.0f);
                    uint32_t pos = pos0, pos2 = pos0;
                    size_t n_rows = 99, n1 = 99, n2 = 99;
                    float tp[2] = {-1.0f, -1.0f};
                    CHECK(s2r_loudness_reference(c.p, hop, nb && N ? stems.p : nullptr, nb, N ? master.p : nullptr, N, state.p, &pos, made ? rows.p : nullptr,
                                                 rows.n, &n_rows, tp) == S2R_OK);
                    CHECK(n_rows == made && pos == (pos0 + N) % hop);
                    for (size_t i = 0; i < rows.n; i++) CHECK(rows[i] >= 0.0f && std::isfinite(rows[i]));
                    for (size_t i = 0; i < ST; i++) CHECK(std::isfinite(state[i]));
                    float peak[2] = {0.0f, 0.0f};
                    for (size_t n = 0; n < N; n++) for (size_t ch = 0; ch < 2; ch++) peak[ch] = std::fmax(peak[ch], std::fabs(master[2 * n + ch]));
                    CHECK(tp[0] >= peak[0] && tp[1] >= peak[1]);         // the samples themselves are among the maximum's values
                    // the master's last 16 frames of history followed by call
                    for (size_t k = 0; k < 16 && N >= 16; k++) for (size_t ch = 0; ch < 2; ch++) CHECK(state[90 + 2 * k + ch] == master[2 * (N - 16 + k) + ch]);
                    // the same stream cut at N / 3: the true peak may not be NULL-checked away, the rows arrive in two parts
                    const uint32_t Na = N / 3u, Nb = N - Na;
                    const size_t made_a = ((size_t)pos0 + Na) / hop;
                    // (stems are bus-major per call: the two calls' stems are gathered into buffers of their own)
                    Buf sa(2u * (size_t)nb * Na), sb(2u * (size_t)nb * Nb);
                    for (uint32_t b = 0; b < nb; b++) {
                        for (size_t i = 0; i < 2u * (size_t)Na; i++) sa[2u * (size_t)b * Na + i] = stems[2u * (size_t)b * N + i];
                        for (size_t i = 0; i < 2u * (size_t)Nb; i++) sb[2u * (size_t)b * Nb + i] = stems[2u * (size_t)b * N + 2u * (size_t)Na + i];
                    }
                    CHECK(s2r_loudness_reference(c.p, hop, nb && Na ? sa.p : nullptr, nb, Na ? master.p : nullptr, Na, state2.p, &pos2, made_a ? rows2.p : nullptr,
                                                 made_a * CH, &n1, nullptr) == S2R_OK);
                    CHECK(n1 == made_a);
                    CHECK(s2r_loudness_reference(c.p, hop, nb && Nb ? sb.p : nullptr, nb, Nb ? master.p + 2u * (size_t)Na : nullptr, Nb, state2.p, &pos2,
                                                 made - made_a ? rows2.p + made_a * CH : nullptr, (made - made_a) * CH, &n2, nullptr) == S2R_OK);
                    CHECK(n1 + n2 == made && pos2 == pos);
                    for (size_t i = 0; i < rows.n; i++) CHECK(rows2[i] == rows[i]);
                    for (size_t i = 0; i < ST; i++) CHECK(state2[i] == state[i]);
                }
    // a bus past the call's runs on zeros from a zero state: its sums are +0.0, its filters stay +0.0
    Buf stems(2u * 2u * 64u), master(2u * 64u), state(ST), rows(4 * CH, -1.0f);
    fill_noise(stems); fill_noise(master);
    uint32_t pos = 0; size_t n_rows = 0;
    CHECK(s2r_loudness_reference(c.p, 16u, stems.p, 2u, master.p, 64u, state.p, &pos, rows.p, rows.n, &n_rows, nullptr) == S2R_OK && n_rows == 4);
    for (size_t r = 0; r < 4; r++) for (size_t q = 0; q < CH; q++) CHECK((q >= 4 && q < 16) ? rows[r * CH + q] == 0.0f : rows[r * CH + q] > 0.0f);
    for (size_t q = 4; q < 16; q++) for (size_t i = 0; i < 4; i++) CHECK(state[4 * q + i] == 0.0f && !std::signbit(state[4 * q + i]));
}

// rows of a constant mean square: every block has the same loudness, and the three readings are it as soon as there are hops enough
void readings() {
    const uint32_t hop = 4800;
    for (size_t n_hops : {(size_t)0, (size_t)1, (size_t)3, (size_t)4, (size_t)29, (size_t)30, (size_t)64}) {
        Buf rows(n_hops * CH);
        for (size_t i = 0; i < n_hops; i++) { rows[i * CH + 16] = 0.25f * hop; rows[i * CH + 17] = 0.25f * hop; rows[i * CH + 2] = 1e-9f; }
        double out[3] = {1.0, 1.0, 1.0};
        CHECK(s2r_loudness_readings(n_hops ? rows.p : nullptr, n_hops, hop, 8u, out) == S2R_OK);
        const double want = -0.691 + 10.0 * std::log10(0.5);
        CHECK(n_hops >= 4 ? std::fabs(out[0] - want) < 1e-12 : out[0] == -INFINITY);
        CHECK(n_hops >= 30 ? std::fabs(out[1] - want) < 1e-12 : out[1] == -INFINITY);
        CHECK(n_hops >= 4 ? std::fabs(out[2] - want) < 1e-12 : out[2] == -INFINITY);
        CHECK(s2r_loudness_readings(n_hops ? rows.p : nullptr, n_hops, hop, 1u, out) == S2R_OK);      // below the absolute gate
        CHECK(out[2] == -INFINITY && (n_hops >= 4 ? out[0] < -70.0 && std::isfinite(out[0]) : out[0] == -INFINITY));
        CHECK(s2r_loudness_readings(n_hops ? rows.p : nullptr, n_hops, hop, 0u, out) == S2R_OK);      // silence
        CHECK(out[0] == -INFINITY && out[1] == -INFINITY && out[2] == -INFINITY);
    }
}

void refusals() {
    Buf c(10), bad(10), state(ST, 1.0f), master(2, 1.0f), stems(2, 1.0f), rows(CH, 1.0f);
    CHECK(s2r_loudness_design(48000.0, c.p) == S2R_OK);
    for (size_t i = 0; i < 10; i++) bad[i] = c[i];
    bad[7] = NAN;
    uint32_t pos = 15; size_t n_rows = 77; float tp[2] = {5.0f, 5.0f};
#define REF(cp, hop, st, nb, ms, N, sp, pp, rp, cap, np) s2r_loudness_reference(cp, hop, st, nb, ms, N, sp, pp, rp, cap, np, tp)
    CHECK(REF(c.p, 15u, stems.p, 1u, master.p, 1u, state.p, &pos, rows.p, rows.n, &n_rows) == S2R_ERR_PATCH_RANGE);
    CHECK(REF(c.p, (1u << 20) + 1u, stems.p, 1u, master.p, 1u, state.p, &pos, rows.p, rows.n, &n_rows) == S2R_ERR_PATCH_RANGE);
    CHECK(REF(bad.p, 16u, stems.p, 1u, master.p, 1u, state.p, &pos, rows.p, rows.n, &n_rows) == S2R_ERR_PATCH_RANGE);
    CHECK(REF(c.p, 16u, stems.p, 9u, master.p, 1u, state.p, &pos, rows.p, rows.n, &n_rows) == S2R_ERR_PATCH_RANGE);
    pos = 16;
    CHECK(REF(c.p, 16u, stems.p, 1u, master.p, 1u, state.p, &pos, rows.p, rows.n, &n_rows) == S2R_ERR_PATCH_RANGE);
    pos = 15;
    CHECK(REF(nullptr, 16u, stems.p, 1u, master.p, 1u, state.p, &pos, rows.p, rows.n, &n_rows) == S2R_ERR_INVALID);
    CHECK(REF(c.p, 16u, nullptr, 1u, master.p, 1u, state.p, &pos, rows.p, rows.n, &n_rows) == S2R_ERR_INVALID);
    CHECK(REF(c.p, 16u, stems.p, 1u, nullptr, 1u, state.p, &pos, rows.p, rows.n, &n_rows) == S2R_ERR_INVALID);
    CHECK(REF(c.p, 16u, stems.p, 1u, master.p, 1u, nullptr, &pos, rows.p, rows.n, &n_rows) == S2R_ERR_INVALID);
    CHECK(REF(c.p, 16u, stems.p, 1u, master.p, 1u, state.p, nullptr, rows.p, rows.n, &n_rows) == S2R_ERR_INVALID);
    CHECK(REF(c.p, 16u, stems.p, 1u, master.p, 1u, state.p, &pos, rows.p, rows.n, nullptr) == S2R_ERR_INVALID);
    CHECK(REF(c.p, 16u, stems.p, 1u, master.p, 1u, state.p, &pos, rows.p, CH - 1, &n_rows) == S2R_ERR_INVALID);      // the call completes a hop
    CHECK(REF(c.p, 16u, stems.p, 1u, master.p, 1u, state.p, &pos, nullptr, CH, &n_rows) == S2R_ERR_INVALID);
#undef REF
    for (size_t i = 0; i < ST; i++) CHECK(state[i] == 1.0f);
    for (size_t i = 0; i < CH; i++) CHECK(rows[i] == 1.0f);
    CHECK(pos == 15 && n_rows == 77 && tp[0] == 5.0f && tp[1] == 5.0f);
    double out[3] = {2.0, 2.0, 2.0};
    CHECK(s2r_loudness_readings(rows.p, 1, 15u, 0u, out) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_loudness_readings(rows.p, 1, 16u, 9u, out) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_loudness_readings(nullptr, 1, 16u, 0u, out) == S2R_ERR_INVALID);
    CHECK(s2r_loudness_readings(rows.p, 1, 16u, 0u, nullptr) == S2R_ERR_INVALID);
    CHECK(out[0] == 2.0 && out[1] == 2.0 && out[2] == 2.0);
    CHECK(s2r_loudness_design(NAN, bad.p) == S2R_ERR_PATCH_RANGE && s2r_loudness_design(7999.0, bad.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_loudness_design(768001.0, bad.p) == S2R_ERR_PATCH_RANGE && s2r_loudness_design(INFINITY, bad.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_loudness_design(48000.0, nullptr) == S2R_ERR_INVALID);
    CHECK(std::isnan(bad[7]) && bad[0] == c[0]);
    for (double sr : {8000.0, 44100.0, 768000.0}) {
        CHECK(s2r_loudness_design(sr, bad.p) == S2R_OK);
        for (size_t i = 0; i < 10; i++) CHECK(std::isfinite(bad[i]));
        for (size_t k = 0; k < 2; k++) CHECK(std::fabs((double)bad[5 * k + 4]) < 1.0 && std::fabs((double)bad[5 * k + 3]) < 1.0 + (double)bad[5 * k + 4]);     // stable
    }
}

}  // namespace

int main() {
    shapes();
    readings();
    refusals();
    std::printf("loudness ok\n");
    return 0;
}
