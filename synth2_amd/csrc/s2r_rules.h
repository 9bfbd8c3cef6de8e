// s2r_rules.h — the ranges that the entry points (s2r_host_mix.cpp, s2r_host_post.cpp) and the handle-free rule functions (s2r_rules.cpp) share, so that a
// setter and its reference cannot disagree on one.  No HIP.  Every predicate is false for a NaN.
#pragma once
#include <cmath>
#include <cstdint>

#include "s2r.h"

static inline bool pan_in_range(float x) { return x >= -1.0f && x <= 1.0f; }
static inline bool unit_in_range(float x) { return x >= 0.0f && x <= 1.0f; }
static inline bool fader_in_range(float fader, float shift) { return fader >= 0.0f && fader <= 1.0f && shift >= -2.0f && shift <= 2.0f; }
static inline bool limiter_in_range(float ceiling, uint32_t lookahead, uint32_t hold) {
    const float lo = std::ldexp(1.0f, -S2R_LIMITER_CEILING_LOG2), hi = std::ldexp(1.0f, S2R_LIMITER_CEILING_LOG2);
    return ceiling >= lo && ceiling <= hi && lookahead >= 1u && lookahead <= S2R_LIMITER_MAX_LOOKAHEAD && hold <= S2R_LIMITER_MAX_HOLD;
}
// a delay's four levels: the sum condition in double, from the two floats
static inline bool delay_mix_in_range(float feedback, float cross, float dry, float wet) {
    return pan_in_range(feedback) && pan_in_range(cross) && std::fabs((double)feedback) + std::fabs((double)cross) <= 1.0 && unit_in_range(dry) &&
           unit_in_range(wet);
}
// a chorus's two levels, and its delay range: base >= 1, depth >= 0 and fl(base + depth) <= S2R_CHORUS_MAX_DELAY, the sum
// rounded to binary32 (-ffp-contract=off; the volatile keeps a build with excess precision honest).  A NaN or an infinity fails a comparison.
static inline bool chorus_mix_in_range(float dry, float wet) { return unit_in_range(dry) && unit_in_range(wet); }
static inline bool chorus_delay_in_range(float base, float depth) {
    if (!(base >= 1.0f) || !(depth >= 0.0f)) return false;
    volatile float top = base + depth;
    return top <= S2R_CHORUS_MAX_DELAY;
}
static inline bool chorus_in_range(uint32_t voices, float base, float depth, float dry, float wet) {
    return voices >= 1u && voices <= S2R_CHORUS_MAX_VOICES && chorus_delay_in_range(base, depth) && chorus_mix_in_range(dry, wet);
}
// H = floor(fl(base + depth)) + 1 for a pair in range
static inline uint32_t chorus_history(float base, float depth) { volatile float top = base + depth; return (uint32_t)top + 1u; }
// voice v's offset on the left channel: floor(v * 2^32 / V)
static inline uint32_t chorus_voice_offset(uint32_t v, uint32_t voices) { return (uint32_t)(((uint64_t)v << 32) / voices); }
// an EQ's bands, [n_bands][5] as (b0, b1, b2, a1, a2): every coefficient finite and every band inside the stability
// triangle, |a2| < 1 and |a1| < 1 + a2, in double from the floats
static inline bool eq_band_in_range(const float *c) {
    for (int i = 0; i < 5; i++) if (!std::isfinite(c[i])) return false;
    const double a1 = (double)c[3], a2 = (double)c[4];
    return std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2;
}
static inline bool eq_in_range(uint32_t n_bands, const float *coeffs) {
    if (n_bands > S2R_EQ_MAX_BANDS) return false;
    for (uint32_t k = 0; k < n_bands && coeffs; k++) if (!eq_band_in_range(coeffs + 5 * k)) return false;
    return true;
}
// a bus's dynamics: every curve entry finite and in [0, 2^8], both coefficients in [0, 1); a state finite and >= 0
static inline bool dyn_coef_in_range(float a) { return a >= 0.0f && a < 1.0f; }
static inline bool dyn_in_range(const float *curve, float a_att, float a_rel) {
    if (!dyn_coef_in_range(a_att) || !dyn_coef_in_range(a_rel)) return false;
    for (uint32_t j = 0; j < S2R_DYN_CURVE_POINTS && curve; j++) if (!(curve[j] >= 0.0f && curve[j] <= 256.0f)) return false;
    return true;
}
static inline bool dyn_state_in_range(float y) { return std::isfinite(y) && y >= 0.0f; }
// a bus's room: every effective delay — cd[i], cd[i] + spread, ad[j], ad[j] + spread — in [S2R_ROOM_MIN_DELAY,
// S2R_ROOM_MAX_DELAY]; feedback in [0, 1), damp in [0, 1], g in (-1, 1), gain, dry, wet and cross in [0, 1].  Null delays pass: the
// caller refuses them by another name.
static inline bool room_delay_in_range(uint32_t d, uint32_t spread) {
    return spread <= S2R_ROOM_MAX_DELAY && d >= S2R_ROOM_MIN_DELAY && d <= S2R_ROOM_MAX_DELAY && d + spread <= S2R_ROOM_MAX_DELAY;
}
static inline bool room_delays_in_range(const uint32_t *cd, const uint32_t *ad, uint32_t spread) {
    if (spread > S2R_ROOM_MAX_DELAY) return false;
    for (uint32_t i = 0; i < S2R_ROOM_COMBS && cd; i++) if (!room_delay_in_range(cd[i], spread)) return false;
    for (uint32_t j = 0; j < S2R_ROOM_ALLPASSES && ad; j++) if (!room_delay_in_range(ad[j], spread)) return false;
    return true;
}
static inline bool room_levels_in_range(float feedback, float damp, float g, float gain, float dry, float wet, float cross) {
    return feedback >= 0.0f && feedback < 1.0f && unit_in_range(damp) && g > -1.0f && g < 1.0f && unit_in_range(gain) && unit_in_range(dry) &&
           unit_in_range(wet) && unit_in_range(cross);
}
// the floats of a room's state, for delays in range
static inline size_t room_state_count(const uint32_t *cd, const uint32_t *ad, uint32_t spread) {
    size_t n = 0;
    for (uint32_t i = 0; i < S2R_ROOM_COMBS; i++) n += 2u * (size_t)cd[i] + spread + 2u;
    for (uint32_t j = 0; j < S2R_ROOM_ALLPASSES; j++) n += 2u * (size_t)ad[j] + spread;
    return n;
}
// Where the 24 lines sit in that array and how long they are.  Line c * 8 + i is comb i of channel c, line 16 + c * 4 + j allpass j;
// a comb's f follows its line.
static inline void room_layout(const uint32_t *cd, const uint32_t *ad, uint32_t spread, uint32_t len[24], uint32_t off[24]) {
    uint32_t at = 0;
    for (uint32_t c = 0; c < 2u; c++) {
        for (uint32_t i = 0; i < S2R_ROOM_COMBS; i++) { const uint32_t l = c * 8u + i; len[l] = cd[i] + c * spread; off[l] = at; at += len[l] + 1u; }
        for (uint32_t j = 0; j < S2R_ROOM_ALLPASSES; j++) { const uint32_t l = 16u + c * 4u + j; len[l] = ad[j] + c * spread; off[l] = at; at += len[l]; }
    }
}

// a bus's drive: every curve entry finite, pre in [0, S2R_DRIVE_MAX_PRE], dry and wet in [0, 1].  A null curve passes:
// the caller refuses it by another name, or keeps the table it has.
static inline bool drive_in_range(const float *curve, float pre, float dry, float wet) {
    if (!(pre >= 0.0f && pre <= S2R_DRIVE_MAX_PRE) || !unit_in_range(dry) || !unit_in_range(wet)) return false;
    for (uint32_t j = 0; j < S2R_DRIVE_CURVE_POINTS && curve; j++) if (!std::isfinite(curve[j])) return false;
    return true;
}
// The library's one prototype filter, h[S2R_DRIVE_TAPS], and the interpolator's g = 4 h (exact): computed at the first call, once per
// process (s2r_rules.cpp), never inside a fill.
struct S2rDriveTaps { float h[S2R_DRIVE_TAPS], g[S2R_DRIVE_TAPS]; };
const S2rDriveTaps &drive_taps();
// One oversampled sample through the table: the rule's second and third lines.  Sign and magnitude, so that a small signal keeps its
// relative precision; a NaN, outside the contract, reads inside the table like everything else.
static inline float drive_shape(const float *curve, float pre, float u) {
    const float t = pre * u;
    const float at = std::fabs(t);
    const float m = at < 1.0f ? at : 1.0f;
    const float a = m * 512.0f;
    const uint32_t ia = (uint32_t)a;
    const uint32_t i = ia < 511u ? ia : 511u;
    const float fr = a - (float)i;
    const bool neg = t < 0.0f;
    const float c0 = curve[neg ? 512u - i : 512u + i], c1 = curve[neg ? 511u - i : 513u + i];
    const float d = c1 - c0;
    const float e = fr * d;
    return c0 + e;
}

// a bus's flanger: base >= S2R_FLANGER_MIN_DELAY, depth >= 0 and fl(base + depth) <= S2R_FLANGER_MAX_DELAY, the sum
// rounded to binary32 as the chorus's; the four levels are the bus delay's, the sum condition in double.  False for a NaN or an infinity.
static inline bool flanger_delay_in_range(float base, float depth) {
    if (!(base >= S2R_FLANGER_MIN_DELAY) || !(depth >= 0.0f)) return false;
    volatile float top = base + depth;
    return top <= S2R_FLANGER_MAX_DELAY;
}
static inline bool flanger_in_range(float base, float depth, float feedback, float cross, float dry, float wet) {
    return flanger_delay_in_range(base, depth) && delay_mix_in_range(feedback, cross, dry, wet);
}
// H = floor(fl(base + depth)) + 1 for a pair in range: 33 .. 4096
static inline uint32_t flanger_history(float base, float depth) { volatile float top = base + depth; return (uint32_t)top + 1u; }

// the master's loudness meter: ten finite coefficients, the hop and the window of hop rows in their ranges.  Null
// coefficients pass: the caller refuses them by another name.
static inline bool loudness_hop_in_range(uint32_t hop) { return hop >= S2R_LOUDNESS_MIN_HOP && hop <= S2R_LOUDNESS_MAX_HOP; }
static inline bool loudness_in_range(const float *coeffs, uint32_t hop, uint32_t max_hops) {
    for (uint32_t i = 0; i < 10u && coeffs; i++) if (!std::isfinite(coeffs[i])) return false;
    return loudness_hop_in_range(hop) && max_hops >= S2R_LOUDNESS_MIN_HOPS && max_hops <= S2R_LOUDNESS_MAX_HOPS;
}
// where the state's parts sit among its S2R_LOUDNESS_STATE floats: filters [18][2][2], hop sums [18], the master's last frames [16][2]
enum { S2R_LOUD_FILT = 0, S2R_LOUD_SUMS = 72, S2R_LOUD_HIST = 90, S2R_LOUD_HIST_FRAMES = 16 };
static_assert(S2R_LOUD_HIST + 2 * S2R_LOUD_HIST_FRAMES == S2R_LOUDNESS_STATE && S2R_LOUD_SUMS == 4 * S2R_LOUDNESS_CHANNELS, "the layout s2r.h states");
static_assert(4 * S2R_LOUD_HIST_FRAMES + 1 == S2R_DRIVE_TAPS, "phase 0 of the interpolator reaches 16 frames back");

// the master's spectrum meter: a power-of-two size, the hop and the rows kept in their ranges, a finite window.  A null
// window passes: the caller refuses it by another name.
static inline bool spectrum_fft_in_range(uint32_t n) { return n >= S2R_SPECTRUM_MIN_FFT && n <= S2R_SPECTRUM_MAX_FFT && (n & (n - 1u)) == 0u; }
static inline bool spectrum_hop_in_range(uint32_t n, uint32_t hop) {
    const uint32_t lo = n / 8u > S2R_SPECTRUM_MIN_HOP ? n / 8u : S2R_SPECTRUM_MIN_HOP;
    return hop >= lo && hop <= S2R_SPECTRUM_MAX_HOP;
}
static inline bool spectrum_in_range(uint32_t n, uint32_t hop, const float *window, uint32_t max_rows) {
    if (!spectrum_fft_in_range(n) || !spectrum_hop_in_range(n, hop) || max_rows < 1u || max_rows > S2R_SPECTRUM_MAX_ROWS) return false;
    for (uint32_t i = 0; i < n && window; i++) if (!std::isfinite(window[i])) return false;
    return true;
}
static inline uint32_t spectrum_log2(uint32_t n) { uint32_t l = 0; while ((1u << l) < n) l++; return l; }

// the master's PCM stage: the word length, the dither kind and the tap count in their ranges, every tap finite and at
// most S2R_PCM_MAX_TAP in magnitude.  Null taps pass: the caller refuses them by another name.
static inline bool pcm_in_range(uint32_t bits, uint32_t dither, const float *taps, uint32_t n_taps) {
    if (bits < S2R_PCM_MIN_BITS || bits > S2R_PCM_MAX_BITS || dither > S2R_DITHER_TRI || n_taps > S2R_PCM_MAX_TAPS) return false;
    for (uint32_t k = 0; k < n_taps && taps; k++) if (!(std::fabs(taps[k]) <= S2R_PCM_MAX_TAP)) return false;
    return true;
}
// ... and a state of it: every shaped error within the clamp of the rule's step 6
static inline bool pcm_state_in_range(const float *state) {
    for (uint32_t i = 0; i < S2R_PCM_STATE && state; i++) if (!(std::fabs(state[i]) <= 2.0f)) return false;
    return true;
}
// the rule's integer hash and its step 4: the dither of frame t_n and channel q, exact in binary32
static inline uint32_t pcm_mix(uint32_t u) {
    u ^= u >> 16; u *= 0x7feb352du; u ^= u >> 15; u *= 0x846ca68bu; u ^= u >> 16;
    return u;
}
static inline float pcm_dither_value(uint32_t seed, uint32_t t_n, uint32_t q, uint32_t kind) {
    const uint32_t k = pcm_mix(pcm_mix(t_n ^ seed) + q);
    const int r1 = (int)(k >> 16), r2 = (int)(k & 0xffffu);
    if (kind == S2R_DITHER_TRI) return (float)(r1 - r2) * 0x1p-16f;
    if (kind == S2R_DITHER_RECT) return (float)(2 * r1 - 65535) * 0x1p-17f;
    return 0.0f;
}

// the master's sample-rate converter: the ratio, the taps per phase and the table's size in their ranges, every entry of
// the table finite and at most S2R_RESAMPLER_MAX_TAP in magnitude.  A null table passes: the caller refuses it by another name.
static inline bool resampler_ratio_in_range(uint32_t L, uint32_t M) {
    if (L < 1u || L > S2R_RESAMPLER_MAX_FACTOR || M < 1u || M > S2R_RESAMPLER_MAX_FACTOR || L > 4u * M || M > 4u * L) return false;
    uint32_t a = L, b = M;
    while (b) { const uint32_t r = a % b; a = b; b = r; }
    return a == 1u;
}
static inline bool resampler_in_range(uint32_t L, uint32_t M, uint32_t T, const float *table) {
    if (!resampler_ratio_in_range(L, M) || T < S2R_RESAMPLER_MIN_TAPS || T > S2R_RESAMPLER_MAX_TAPS || T % 4u || L * T > S2R_RESAMPLER_MAX_TABLE) return false;
    for (uint32_t i = 0; i < L * T && table; i++) if (!(std::fabs(table[i]) <= S2R_RESAMPLER_MAX_TAP)) return false;
    return true;
}
// the rule's step 1: the output frames of a call of `frames` frames that starts at ph
static inline uint64_t resampler_count(uint32_t L, uint32_t M, uint32_t ph, uint32_t frames) {
    const uint64_t span = (uint64_t)frames * L;
    return span <= ph ? 0u : (span - ph + M - 1u) / M;
}

// the master's multiband compressor: 1 .. 4 bands, every coefficient row as an EQ band's, every band's curve and
// retention coefficients as a bus's dynamics'.  Null arrays pass: the caller refuses them by another name.
static inline bool multiband_in_range(uint32_t B, const float *lp, const float *hp, const float *ap, const float *curves, const float *a_att, const float *a_rel) {
    if (B < 1u || B > S2R_MULTIBAND_MAX_BANDS) return false;
    for (uint32_t k = 0; k + 1u < B; k++) {
        if (lp && !eq_band_in_range(lp + 5u * k)) return false;
        if (hp && !eq_band_in_range(hp + 5u * k)) return false;
        if (ap && k >= 1u && !eq_band_in_range(ap + 5u * (k - 1u))) return false;
    }
    for (uint32_t j = 0; j < B; j++) {
        if (a_att && !dyn_coef_in_range(a_att[j])) return false;
        if (a_rel && !dyn_coef_in_range(a_rel[j])) return false;
        if (curves && !dyn_in_range(curves + (size_t)j * S2R_DYN_CURVE_POINTS, 0.0f, 0.0f)) return false;
    }
    return true;
}
// The crossover's sections in the state's order — LPa_0, LPb_0, HPa_0, HPb_0, LPa_1, ..., then AP_{0,1}, AP_{0,2}, AP_{1,2} —: where a
// section takes its input (-1: the stage's input x, else an earlier section), whose coefficients it uses (kind 0: lp[row], 1: hp[row],
// 2: ap[row]), how many sections lie in front of it, and the section that leaves band j (-1: x itself, at B = 1).
struct S2rMultibandGraph {
    uint32_t n;
    int32_t src[15], leaf[S2R_MULTIBAND_MAX_BANDS];
    uint32_t kind[15], row[15], depth[15];
};
static inline S2rMultibandGraph multiband_graph(uint32_t B) {
    S2rMultibandGraph g{};
    for (uint32_t k = 0; k + 1u < B; k++) {
        const int32_t r = k ? (int32_t)(4u * (k - 1u) + 3u) : -1;
        const uint32_t dr = k ? g.depth[r] + 1u : 0u;
        const uint32_t at = 4u * k;
        g.src[at] = r; g.src[at + 1u] = (int32_t)at; g.src[at + 2u] = r; g.src[at + 3u] = (int32_t)(at + 2u);
        for (uint32_t i = 0; i < 4u; i++) { g.kind[at + i] = i >> 1; g.row[at + i] = k; g.depth[at + i] = dr + (i & 1u); }
    }
    uint32_t at = 4u * (B - 1u);
    for (uint32_t j = 0; j < B; j++) g.leaf[j] = j + 1u < B ? (int32_t)(4u * j + 1u) : (B > 1u ? (int32_t)(4u * (B - 2u) + 3u) : -1);
    for (uint32_t j = 0; j + 2u < B; j++)
        for (uint32_t k = j + 1u; k + 1u < B; k++) {
            g.src[at] = g.leaf[j]; g.kind[at] = 2u; g.row[at] = k - 1u; g.depth[at] = g.depth[g.leaf[j]] + 1u;
            g.leaf[j] = (int32_t)at++;
        }
    g.n = at;
    return g;
}

// The voice mixer's gain rules, inline: the host's per-voice loops compile them in — a call per voice into s2r_rules.cpp showed as 10
// to 15 us of host time per fill of 65 536 voices (profiles/r12/post_chain.txt).  s2r_rules.cpp exports them under their s2r.h names.
static inline float rule_voice_pan(float pan, float key_spread, uint8_t note) {
    const float k = (float)((int)note - 64) * 0.015625f;        // exact
    const float spread = key_spread * k;                         // (-ffp-contract=off: rounded before the sum)
    const float p = pan + spread;
    return p < -1.0f ? -1.0f : (p > 1.0f ? 1.0f : p);
}

static inline void rule_pan_gains(float p, float *gl, float *gr) {
    const float l = (1.0f - p) * 0.5f, r = (1.0f + p) * 0.5f;
    if (gl) *gl = std::sqrt(l);                                  // IEEE 754 sqrt: correctly rounded
    if (gr) *gr = std::sqrt(r);
}

static inline float rule_voice_gain(float level, float velocity_sens, float velocity) {
    float u = velocity < 1.0f ? velocity : 1.0f;                 // NaN -> 1
    u = u > 0.0f ? u : 0.0f;
    const float d = 1.0f - u;
    const float t = velocity_sens * d;                           // (-ffp-contract=off: rounded before the difference)
    const float a = 1.0f - t;
    return level * a;
}

static inline void rule_fader_gains(float pan, float w, float fader, float pan_shift, float *gl, float *gr) {
    const float q0 = pan + pan_shift;
    const float q = q0 < -1.0f ? -1.0f : (q0 > 1.0f ? 1.0f : q0);
    float al, ar;
    rule_pan_gains(q, &al, &ar);
    const float tl = al * w, tr = ar * w;                        // (-ffp-contract=off; with fader 1 and shift 0: the mixer's a * w, bit for bit)
    if (gl) *gl = tl * fader;
    if (gr) *gr = tr * fader;
}
