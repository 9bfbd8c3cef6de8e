// san_pcm.cpp — s2r_pcm_reference, s2r_pcm_dither, s2r_pcm_pack and s2r_pcm_shaper of csrc/s2r_rules.cpp under ASan + UBSan
// (tests/test_pcm_native.py) at the edges of their shapes — 0, 1, 2, 5 and 9 taps; 8, 16 and 24 bits; the three dither kinds; calls of
// 0, 1, K - 1, K, K + 1 and 1000 frames; 0, 2 and 8 buses; t across the wrap —, every buffer allocated at exactly the size s2r.h
// states, the answers that need no model, and refusals that touch nothing.  Built with -ffp-contract=off.  Prints "pcm ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "s2r.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "san_pcm.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

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
using IBuf = BufT<int32_t>;
using UBuf = BufT<uint32_t>;
using BBuf = BufT<uint8_t>;

uint32_t rng_state = 13579u;
float noise() {                                  // in (-1, 1), never 0
    rng_state = rng_state * 1664525u + 1013904223u;
    return ((float)(rng_state >> 8) + 0.5f) / 8388608.0f - 1.0f;
}
void fill_noise(Buf &b, float amp) { for (size_t i = 0; i < b.n; i++) b[i] = amp * noise(); }

// every shape: a stream in one call and the same stream in two calls leave the same integers, state, t and counts; a bus past the
// call's gets the dither's -1, 0 and 1 alone; the entries of the state past K are +0.0 after a call of a frame or more
void shapes() {
    const uint32_t kinds[5] = {S2R_SHAPER_FLAT, S2R_SHAPER_FIRST, S2R_SHAPER_SECOND, S2R_SHAPER_5TAP, S2R_SHAPER_9TAP};
    for (uint32_t kind : kinds) {
        Buf taps(S2R_PCM_MAX_TAPS);
        uint32_t K = 99;
        CHECK(s2r_pcm_shaper(kind, taps.p, &K) == S2R_OK && K <= S2R_PCM_MAX_TAPS);
        Buf h(K);                                // exactly the K taps
        for (uint32_t k = 0; k < K; k++) h[k] = taps[k];
        for (uint32_t k = K; k < S2R_PCM_MAX_TAPS; k++) CHECK(taps[k] == 0.0f && !std::signbit(taps[k]));
        for (uint32_t bits : {8u, 16u, 24u})
            for (uint32_t dither : {S2R_DITHER_NONE, S2R_DITHER_RECT, S2R_DITHER_TRI})
                for (uint32_t nb : {0u, 2u, 8u})
                    for (uint32_t frames : {0u, 1u, K ? K - 1u : 0u, K, K + 1u, 1000u}) {
                        if (frames == 1000u && (nb == 2u) != (bits == 16u)) continue;       // (the long call: fewer shapes)
                        Buf stems((size_t)nb * frames * 2u), master((size_t)frames * 2u);
                        fill_noise(stems, 0.5f); fill_noise(master, 0.5f);       // (8 bits: 64 + 2 sum |h| stays inside the rails)
                        Buf st(S2R_PCM_STATE), st2(S2R_PCM_STATE);
                        fill_noise(st, 1.9f);
                        for (size_t i = 0; i < st.n; i++) st2[i] = st[i];
                        IBuf pcm((size_t)S2R_PCM_PROGRAMMES * frames * 2u, 7), pcm_a((size_t)S2R_PCM_PROGRAMMES * (frames / 2u) * 2u, 7),
                            pcm_b((size_t)S2R_PCM_PROGRAMMES * (frames - frames / 2u) * 2u, 7);
                        UBuf clips(S2R_PCM_CHANNELS, 7u), clips_a(S2R_PCM_CHANNELS, 7u), clips_b(S2R_PCM_CHANNELS, 7u);
                        uint32_t t = 0xfffffff0u, t2 = 0xfffffff0u;
                        CHECK(s2r_pcm_reference(bits, dither, K ? h.p : nullptr, K, 5u, nb ? stems.p : nullptr, nb, master.p, frames, st.p, &t, pcm.p, clips.p) == S2R_OK);
                        CHECK(t == 0xfffffff0u + frames);
                        // the same stream in two calls: the halves of every programme, gathered
                        const uint32_t fa = frames / 2u, fb = frames - fa;
                        Buf stems_a((size_t)nb * fa * 2u), stems_b((size_t)nb * fb * 2u);
                        for (uint32_t b = 0; b < nb; b++) {
                            for (size_t i = 0; i < 2u * (size_t)fa; i++) stems_a[(size_t)b * fa * 2u + i] = stems[(size_t)b * frames * 2u + i];
                            for (size_t i = 0; i < 2u * (size_t)fb; i++) stems_b[(size_t)b * fb * 2u + i] = stems[(size_t)b * frames * 2u + 2u * fa + i];
                        }
                        CHECK(s2r_pcm_reference(bits, dither, K ? h.p : nullptr, K, 5u, nb ? stems_a.p : nullptr, nb, master.p, fa, st2.p, &t2, pcm_a.p, clips_a.p) == S2R_OK);
                        CHECK(s2r_pcm_reference(bits, dither, K ? h.p : nullptr, K, 5u, nb ? stems_b.p : nullptr, nb, master.p + 2u * (size_t)fa, fb, st2.p, &t2, pcm_b.p,
                                                clips_b.p) == S2R_OK);
                        CHECK(t2 == t);
                        for (uint32_t p = 0; p < S2R_PCM_PROGRAMMES; p++) {
                            for (size_t i = 0; i < 2u * (size_t)fa; i++) CHECK(pcm_a[(size_t)p * fa * 2u + i] == pcm[(size_t)p * frames * 2u + i]);
                            for (size_t i = 0; i < 2u * (size_t)fb; i++) CHECK(pcm_b[(size_t)p * fb * 2u + i] == pcm[(size_t)p * frames * 2u + 2u * fa + i]);
                        }
                        for (uint32_t q = 0; q < S2R_PCM_CHANNELS; q++) CHECK(clips_a[q] + clips_b[q] == clips[q] && clips[q] == 0u);
                        const int32_t top = (int32_t)(1u << (bits - 1u));
                        for (size_t i = 0; i < pcm.n; i++) CHECK(pcm[i] >= -top && pcm[i] < top);
                        for (uint32_t p = nb; p < S2R_MAX_BUSES && frames > 20u; p++)      // (behind the loaded errors: K frames and a margin)
                            for (size_t i = 40; i < 2u * (size_t)frames; i++) CHECK(std::abs(pcm[(size_t)p * frames * 2u + i]) <= (K ? 64 : 1));
                        for (size_t i = 0; i < st.n; i++) {
                            CHECK(st[i] == st2[i] && std::signbit(st[i]) == std::signbit(st2[i]) && std::fabs(st[i]) <= 2.0f);
                            if (frames && i % S2R_PCM_MAX_TAPS >= K) CHECK(st[i] == 0.0f && !std::signbit(st[i]));
                        }
                    }
    }
}

// what needs no model: 0.5 at 16 bits without dither or taps is 16384; full scale clips on the upper rail alone; NaN is 0
void answers() {
    Buf master(2u * 6u), st(S2R_PCM_STATE);
    const float in[6] = {0.5f, -0.5f, 1.0f, -1.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()};
    for (size_t i = 0; i < 6; i++) { master[2 * i] = in[i]; master[2 * i + 1] = -in[i]; }
    IBuf pcm((size_t)S2R_PCM_PROGRAMMES * 6u * 2u, 7);
    UBuf clips(S2R_PCM_CHANNELS, 7u);
    uint32_t t = 0;
    CHECK(s2r_pcm_reference(16, S2R_DITHER_NONE, nullptr, 0, 0, nullptr, 0, master.p, 6, st.p, &t, pcm.p, clips.p) == S2R_OK);
    const int32_t *m = pcm.p + (size_t)S2R_MAX_BUSES * 6u * 2u;
    CHECK(m[0] == 16384 && m[1] == -16384 && m[2] == -16384 && m[3] == 16384 && m[4] == 32767 && m[5] == -32768 && m[6] == -32768 && m[7] == 32767);
    CHECK(m[8] == 0 && m[9] == 0 && m[10] == 32767 && m[11] == -32768);
    CHECK(clips[16] == 2u && clips[17] == 2u && clips[0] == 0u && t == 6u);
    for (size_t i = 0; i < (size_t)S2R_MAX_BUSES * 6u * 2u; i++) CHECK(pcm[i] == 0);
    // the dither: on its grid, inside its range, +0.0 for none
    for (uint32_t tn : {0u, 1u, 0xffffffffu, 123456789u})
        for (uint32_t q = 0; q < S2R_PCM_CHANNELS; q++) {
            float d = 9.0f;
            CHECK(s2r_pcm_dither(42u, tn, q, S2R_DITHER_TRI, &d) == S2R_OK && std::fabs(d) < 1.0f && d * 65536.0f == std::rint(d * 65536.0f));
            CHECK(s2r_pcm_dither(42u, tn, q, S2R_DITHER_RECT, &d) == S2R_OK && std::fabs(d) < 0.5f && d * 131072.0f == std::rint(d * 131072.0f));
            CHECK(s2r_pcm_dither(42u, tn, q, S2R_DITHER_NONE, &d) == S2R_OK && d == 0.0f && !std::signbit(d));
        }
}

void packing() {
    const int32_t v[4] = {-32768, 32767, -1, 258};
    for (uint32_t bytes : {2u, 3u, 4u}) {
        IBuf in(4);
        for (size_t i = 0; i < 4; i++) in[i] = v[i];
        BBuf out(4u * bytes, 0xeeu);
        CHECK(s2r_pcm_pack(in.p, 4, 16, bytes, out.p) == S2R_OK);
        for (size_t i = 0; i < 4; i++) {
            const uint32_t u = (uint32_t)v[i] << (8u * bytes - 16u);
            for (uint32_t b = 0; b < bytes; b++) CHECK(out[i * bytes + b] == (uint8_t)(u >> (8u * b)));
        }
    }
    IBuf in24(2);
    in24[0] = -(1 << 23); in24[1] = (1 << 23) - 1;
    BBuf out24(6, 0xeeu);
    CHECK(s2r_pcm_pack(in24.p, 2, 24, 3, out24.p) == S2R_OK);
    CHECK(out24[0] == 0 && out24[1] == 0 && out24[2] == 0x80 && out24[3] == 0xff && out24[4] == 0xff && out24[5] == 0x7f);
    BBuf none(0);
    IBuf nothing(0);
    CHECK(s2r_pcm_pack(nothing.p, 0, 16, 2, none.p) == S2R_OK);
    // refusals: a container narrower than the bits, another container, bits out of range, a sample out of range — nothing is written
    BBuf keep(6, 0xeeu);
    CHECK(s2r_pcm_pack(in24.p, 2, 24, 2, keep.p) == S2R_ERR_PATCH_RANGE && s2r_pcm_pack(in24.p, 2, 24, 5, keep.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_pcm_pack(in24.p, 2, 24, 1, keep.p) == S2R_ERR_PATCH_RANGE && s2r_pcm_pack(in24.p, 2, 7, 2, keep.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_pcm_pack(in24.p, 2, 25, 4, keep.p) == S2R_ERR_PATCH_RANGE && s2r_pcm_pack(in24.p, 2, 16, 3, keep.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_pcm_pack(nullptr, 2, 16, 2, keep.p) == S2R_ERR_INVALID && s2r_pcm_pack(in24.p, 2, 24, 3, nullptr) == S2R_ERR_INVALID);
    for (size_t i = 0; i < keep.n; i++) CHECK(keep[i] == 0xeeu);
}

void refusals() {
    Buf taps(S2R_PCM_MAX_TAPS), st(S2R_PCM_STATE), master(2u * 4u), stems(2u * 2u * 4u);
    uint32_t K = 0;
    CHECK(s2r_pcm_shaper(S2R_SHAPER_9TAP, taps.p, &K) == S2R_OK && K == 9u);
    CHECK(s2r_pcm_shaper(6u, taps.p, &K) == S2R_ERR_PATCH_RANGE && s2r_pcm_shaper(0u, nullptr, &K) == S2R_ERR_INVALID && s2r_pcm_shaper(0u, taps.p, nullptr) == S2R_ERR_INVALID);
    CHECK(K == 9u && taps[0] == 2.412f);
    fill_noise(st, 1.0f); fill_noise(master, 0.5f); fill_noise(stems, 0.5f);
    Buf st0(S2R_PCM_STATE);
    for (size_t i = 0; i < st.n; i++) st0[i] = st[i];
    IBuf pcm((size_t)S2R_PCM_PROGRAMMES * 4u * 2u, 7);
    UBuf clips(S2R_PCM_CHANNELS, 7u);
    uint32_t t = 41;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    auto call = [&](uint32_t bits, uint32_t dither, const float *h, uint32_t k, uint32_t nb, float *state, uint32_t *tp, int32_t *out) {
        return s2r_pcm_reference(bits, dither, h, k, 1u, stems.p, nb, master.p, 4, state, tp, out, clips.p);
    };
    CHECK(call(7, 2, taps.p, 9, 2, st.p, &t, pcm.p) == S2R_ERR_PATCH_RANGE && call(25, 2, taps.p, 9, 2, st.p, &t, pcm.p) == S2R_ERR_PATCH_RANGE);
    CHECK(call(16, 3, taps.p, 9, 2, st.p, &t, pcm.p) == S2R_ERR_PATCH_RANGE && call(16, 2, taps.p, 10, 2, st.p, &t, pcm.p) == S2R_ERR_PATCH_RANGE);
    CHECK(call(16, 2, taps.p, 9, 9, st.p, &t, pcm.p) == S2R_ERR_PATCH_RANGE);
    Buf bad(S2R_PCM_MAX_TAPS);
    for (size_t i = 0; i < bad.n; i++) bad[i] = taps[i];
    bad[8] = 16.5f;
    CHECK(call(16, 2, bad.p, 9, 2, st.p, &t, pcm.p) == S2R_ERR_PATCH_RANGE);
    bad[8] = nan;
    CHECK(call(16, 2, bad.p, 9, 2, st.p, &t, pcm.p) == S2R_ERR_PATCH_RANGE && call(16, 2, bad.p, 8, 2, st.p, &t, pcm.p) == S2R_OK);
    CHECK(t == 45u);
    for (size_t i = 0; i < st.n; i++) st0[i] = st[i];
    for (size_t i = 0; i < pcm.n; i++) pcm[i] = 7;
    for (size_t i = 0; i < clips.n; i++) clips[i] = 7u;
    Buf wide(S2R_PCM_STATE);
    wide[161] = 2.5f;
    CHECK(call(16, 2, taps.p, 9, 2, wide.p, &t, pcm.p) == S2R_ERR_PATCH_RANGE && wide[161] == 2.5f);
    wide[161] = nan;
    CHECK(call(16, 2, taps.p, 9, 2, wide.p, &t, pcm.p) == S2R_ERR_PATCH_RANGE);
    CHECK(call(16, 2, nullptr, 9, 2, st.p, &t, pcm.p) == S2R_ERR_INVALID && call(16, 2, taps.p, 9, 2, nullptr, &t, pcm.p) == S2R_ERR_INVALID);
    CHECK(call(16, 2, taps.p, 9, 2, st.p, nullptr, pcm.p) == S2R_ERR_INVALID && call(16, 2, taps.p, 9, 2, st.p, &t, nullptr) == S2R_ERR_INVALID);
    CHECK(s2r_pcm_reference(16, 2, taps.p, 9, 1u, nullptr, 2, master.p, 4, st.p, &t, pcm.p, clips.p) == S2R_ERR_INVALID);
    CHECK(s2r_pcm_reference(16, 2, taps.p, 9, 1u, stems.p, 2, nullptr, 4, st.p, &t, pcm.p, clips.p) == S2R_ERR_INVALID);
    CHECK(t == 45u);
    for (size_t i = 0; i < st.n; i++) CHECK(st[i] == st0[i]);
    for (size_t i = 0; i < pcm.n; i++) CHECK(pcm[i] == 7);
    for (size_t i = 0; i < clips.n; i++) CHECK(clips[i] == 7u);
    // a call of no frames takes null signals and null samples, and no counts at all
    CHECK(s2r_pcm_reference(16, 2, taps.p, 9, 1u, nullptr, 8, nullptr, 0, st.p, &t, nullptr, nullptr) == S2R_OK && t == 45u);
    float d = 9.0f;
    CHECK(s2r_pcm_dither(1, 2, 18, 2, &d) == S2R_ERR_PATCH_RANGE && s2r_pcm_dither(1, 2, 0, 3, &d) == S2R_ERR_PATCH_RANGE && s2r_pcm_dither(1, 2, 0, 2, nullptr) == S2R_ERR_INVALID);
    CHECK(d == 9.0f);
}

}  // namespace

int main() {
    shapes();
    answers();
    packing();
    refusals();
    std::printf("pcm ok\n");
    return 0;
}
