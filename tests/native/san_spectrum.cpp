// san_spectrum.cpp — s2r_spectrum_reference, s2r_spectrum_readings, s2r_spectrum_band_readings, s2r_spectrum_window and
// s2r_spectrum_twiddles of csrc/s2r_rules.cpp under ASan + UBSan (tests/test_spectrum_native.py) at the edges of their shapes — sizes
// 256, 512 and 8192; hops of N / 8, N and past N; calls of 0, 1, hop - 1, hop and many hops of frames, from the start of a hop and from
// its last frame; 0, 2 and 8 buses —, every buffer allocated at exactly the size s2r.h states, the answers that need no model, and
// refusals that touch nothing.  Built with -ffp-contract=off.  Prints "spectrum ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "s2r.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "san_spectrum.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

// a heap block of exactly n elements (n == 0: a pointer that is not null and must not be touched)
template <class T> struct BufT {
    T *p;
    size_t n;
    explicit BufT(size_t n_, T fill = T(0)) : p(new T[n_]), n(n_) { for (size_t i = 0; i < n; i++) p[i] = fill; }
    ~BufT() { delete[] p; }
    BufT(const BufT &) = delete;
    BufT &operator=(const BufT &) = delete;
    T &operator[](size_t i) { return p[i]; }
};
using Buf = BufT<float>;
using DBuf = BufT<double>;

uint32_t rng_state = 24680u;
float noise() {                                  // in (-1, 1), never 0
    rng_state = rng_state * 1664525u + 1013904223u;
    return ((float)(rng_state >> 8) + 0.5f) / 8388608.0f - 1.0f;
}
void fill_noise(Buf &b) { for (size_t i = 0; i < b.n; i++) b[i] = noise(); }

// every shape: the rows buffer holds exactly the rows the call completes, the position moves by the frames, a stream in one call and
// the same stream in two calls leave the same rows and state, a bus past the call's reads +0.0
void shapes() {
    for (uint32_t n : {256u, 512u, 8192u}) {
        const size_t row = S2R_SPECTRUM_ROW(n), bins = n / 2u + 1u;
        Buf w(n), tw(n);
        CHECK(s2r_spectrum_window(S2R_WINDOW_BLACKMAN_HARRIS, n, w.p) == S2R_OK);
        CHECK(s2r_spectrum_twiddles(n, tw.p) == S2R_OK);
        CHECK(tw[0] == 1.0f && tw[1] == 0.0f && tw[2 * (n / 4u)] == 0.0f && tw[2 * (n / 4u) + 1] == -1.0f);
        for (uint32_t hop : {n / 8u, n, n + 5u})
            for (uint32_t nb : {0u, 2u, 8u})
                for (uint32_t pos0 : {0u, hop - 1u})
                    for (uint32_t frames : {0u, 1u, hop - 1u, hop, 2u * hop + 3u}) {
                        if (n == 8192u && (nb == 2u || frames == hop - 1u)) continue;     // (the large size: fewer shapes)
                        Buf stems((size_t)nb * frames * 2u), master((size_t)frames * 2u);
                        fill_noise(stems); fill_noise(master);
                        const size_t made = ((size_t)pos0 + frames) / hop;
                        Buf st(18u * (size_t)n), rows(made * row, 7.0f);
                        fill_noise(st);
                        Buf st2(18u * (size_t)n), rows2(made * row, 7.0f);
                        for (size_t i = 0; i < st.n; i++) st2[i] = st[i];
                        uint32_t pos = pos0;
                        size_t got = 99;
                        CHECK(s2r_spectrum_reference(n, hop, w.p, nb ? stems.p : nullptr, nb, master.p, frames, st.p, &pos, rows.p, rows.n, &got) == S2R_OK);
                        CHECK(got == made && pos == (pos0 + frames) % hop);
                        for (size_t r = 0; r < made; r++)
                            for (uint32_t p = nb; p < 8u; p++)
                                for (size_t k = 0; k < bins; k++) CHECK(rows[r * row + p * bins + k] == 0.0f && !std::signbit(rows[r * row + p * bins + k]));
                        for (size_t i = 0; i < rows.n; i++) CHECK(std::isfinite(rows[i]) && rows[i] >= 0.0f);
                        // the same stream in two calls
                        const uint32_t f1 = frames / 2u, f2 = frames - f1;
                        uint32_t pos2 = pos0;
                        size_t g1 = 0, g2 = 0;
                        Buf s1((size_t)nb * f1 * 2u), s2((size_t)nb * f2 * 2u);
                        for (uint32_t b = 0; b < nb; b++) {
                            for (size_t i = 0; i < 2u * (size_t)f1; i++) s1[(size_t)b * f1 * 2u + i] = stems[(size_t)b * frames * 2u + i];
                            for (size_t i = 0; i < 2u * (size_t)f2; i++) s2[(size_t)b * f2 * 2u + i] = stems[(size_t)b * frames * 2u + 2u * f1 + i];
                        }
                        CHECK(s2r_spectrum_reference(n, hop, w.p, nb ? s1.p : nullptr, nb, master.p, f1, st2.p, &pos2, rows2.p, rows2.n, &g1) == S2R_OK);
                        CHECK(s2r_spectrum_reference(n, hop, w.p, nb ? s2.p : nullptr, nb, master.p + 2u * (size_t)f1, f2, st2.p, &pos2, rows2.p + g1 * row,
                                                     rows2.n - g1 * row, &g2) == S2R_OK);
                        CHECK(g1 + g2 == made && pos2 == pos);
                        for (size_t i = 0; i < rows.n; i++) CHECK(rows[i] == rows2[i]);
                        for (size_t i = 0; i < st.n; i++) CHECK(st[i] == st2[i]);
                        if (made) {                              // readings over exactly these rows, into buffers of exactly their size
                            DBuf db(bins), bands(160), centres(160);
                            CHECK(s2r_spectrum_readings(rows.p, made, n, w.p, 8u, (uint32_t)made, db.p, db.n) == S2R_OK);
                            for (size_t k = 0; k < bins; k++) CHECK(!std::isnan(db[k]));
                            size_t nbands = 0;
                            CHECK(s2r_spectrum_band_readings(rows.p, made, n, w.p, 8u, 1u, 48000.0, 12u, bands.p, centres.p, bands.n, &nbands) == S2R_OK);
                            CHECK(nbands > 0 && nbands <= 160 && centres[0] < centres[nbands - 1]);
                            DBuf exact(nbands);
                            CHECK(s2r_spectrum_band_readings(rows.p, made, n, w.p, 8u, 1u, 48000.0, 12u, exact.p, nullptr, exact.n, &nbands) == S2R_OK);
                            CHECK(s2r_spectrum_band_readings(rows.p, made, n, w.p, 8u, 1u, 48000.0, 12u, exact.p, nullptr, exact.n - 1u, &nbands) == S2R_ERR_INVALID);
                        }
                    }
    }
}

// answers that need no model: DC of 1 through a rectangular window reads 0 dB at bin 0 and nothing elsewhere; silence reads -inf
void answers() {
    const uint32_t n = 256;
    Buf w(n), master(2u * n, 1.0f), st(18u * n), rows(S2R_SPECTRUM_ROW(n));
    CHECK(s2r_spectrum_window(S2R_WINDOW_RECT, n, w.p) == S2R_OK);
    uint32_t pos = 0;
    size_t got = 0;
    CHECK(s2r_spectrum_reference(n, n, w.p, nullptr, 0, master.p, n, st.p, &pos, rows.p, rows.n, &got) == S2R_OK && got == 1 && pos == 0);
    DBuf db(n / 2u + 1u);
    CHECK(s2r_spectrum_readings(rows.p, 1, n, w.p, 8u, 1u, db.p, db.n) == S2R_OK);
    CHECK(db[0] == 0.0);
    for (size_t k = 1; k <= n / 2u; k++) CHECK(db[k] == -HUGE_VAL);
    CHECK(s2r_spectrum_readings(rows.p, 1, n, w.p, 0u, 1u, db.p, db.n) == S2R_OK);
    for (size_t k = 0; k <= n / 2u; k++) CHECK(db[k] == -HUGE_VAL);
    for (size_t i = 0; i < 2u * n; i++) CHECK(st[16u * n + i] == 1.0f);
}

void refusals() {
    const uint32_t n = 256;
    Buf w(n, 1.0f), master(20), st(18u * n, 3.0f), rows(S2R_SPECTRUM_ROW(n) - 1u, 5.0f);
    uint32_t pos = 31;
    size_t got = 42;
    CHECK(s2r_spectrum_reference(n, 32, w.p, nullptr, 0, master.p, 10, st.p, &pos, rows.p, rows.n, &got) == S2R_ERR_INVALID);     // one row, a buffer one float short
    CHECK(s2r_spectrum_reference(n, 31, w.p, nullptr, 0, master.p, 10, st.p, &pos, rows.p, rows.n, &got) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_spectrum_reference(300, 64, w.p, nullptr, 0, master.p, 10, st.p, &pos, rows.p, rows.n, &got) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_spectrum_reference(n, 32, w.p, nullptr, 9, master.p, 10, st.p, &pos, rows.p, rows.n, &got) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_spectrum_reference(n, 32, w.p, nullptr, 2, master.p, 10, st.p, &pos, rows.p, rows.n, &got) == S2R_ERR_INVALID);
    CHECK(s2r_spectrum_reference(n, 32, nullptr, nullptr, 0, master.p, 10, st.p, &pos, rows.p, rows.n, &got) == S2R_ERR_INVALID);
    w[n - 1u] = NAN;
    CHECK(s2r_spectrum_reference(n, 32, w.p, nullptr, 0, master.p, 10, st.p, &pos, rows.p, rows.n, &got) == S2R_ERR_PATCH_RANGE);
    CHECK(pos == 31 && got == 42);
    for (size_t i = 0; i < st.n; i++) CHECK(st[i] == 3.0f);
    for (size_t i = 0; i < rows.n; i++) CHECK(rows[i] == 5.0f);
    CHECK(s2r_spectrum_window(4u, n, w.p) == S2R_ERR_PATCH_RANGE && s2r_spectrum_window(1u, 128u, w.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_spectrum_window(1u, n, nullptr) == S2R_ERR_INVALID && s2r_spectrum_twiddles(n, nullptr) == S2R_ERR_INVALID);
    CHECK(s2r_spectrum_twiddles(16384u, w.p) == S2R_ERR_PATCH_RANGE);
    DBuf db(n / 2u);
    Buf full(S2R_SPECTRUM_ROW(n));
    w[n - 1u] = 1.0f;
    CHECK(s2r_spectrum_readings(full.p, 1, n, w.p, 0u, 1u, db.p, db.n) == S2R_ERR_INVALID);
    CHECK(s2r_spectrum_readings(full.p, 1, n, w.p, 9u, 1u, db.p, db.n) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_spectrum_readings(full.p, 1, n, w.p, 0u, 2u, db.p, db.n) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_spectrum_readings(full.p, 1, n, w.p, 0u, 0u, db.p, db.n) == S2R_ERR_PATCH_RANGE);
}

}  // namespace

int main() {
    shapes();
    answers();
    refusals();
    std::printf("spectrum ok\n");
    return 0;
}
