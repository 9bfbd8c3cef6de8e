// s2r_rules.cpp — the rules of libs2r that need neither a handle nor HIP: the voice mixer's gains, and the reverb, the delay, the master
// section, the master's multiband compressor and the master limiter in plain host loops (s2r.h states each rule).  Plain C++17, -ffp-contract=off: every operation rounded on its own.
#include <cstddef>
#include <cstring>
#include <vector>

#include "s2r_rules.h"

extern "C" {

// ---- the voice mixer's gains: the rules are s2r_rules.h's, exported under their names ----
float s2r_voice_pan(float pan, float key_spread, uint8_t note) { return rule_voice_pan(pan, key_spread, note); }
void s2r_pan_gains(float p, float *gl, float *gr) { rule_pan_gains(p, gl, gr); }
float s2r_voice_gain(float level, float velocity_sens, float velocity) { return rule_voice_gain(level, velocity_sens, velocity); }
void s2r_fader_gains(float pan, float w, float fader, float pan_shift, float *gl, float *gr) { rule_fader_gains(pan, w, fader, pan_shift, gl, gr); }
float s2r_send_gain(float g, float send) { return g * send; }

// ---- per-bus convolution reverb, one channel ----
int s2r_reverb_reference(const float *ir, uint32_t n_taps, const float *x_with_history, uint32_t frames, float dry, float wet, float *out) {
    if (!unit_in_range(dry) || !unit_in_range(wet) || n_taps > S2R_MAX_IR_TAPS) return S2R_ERR_PATCH_RANGE;
    if (!ir || n_taps == 0 || !x_with_history || (!out && frames)) return S2R_ERR_INVALID;
    for (uint32_t k = 0; k < n_taps; k++) if (!std::isfinite(ir[k])) return S2R_ERR_PATCH_RANGE;
    for (uint32_t i = 0; i < frames; i++) {
        const float *x = x_with_history + (n_taps - 1u) + i;     // x[-k]: the dry sample k frames before frame i
        float r = 0.0f;
        for (uint32_t k0 = 0; k0 < n_taps; k0 += S2R_IR_SEGMENT) {
            const uint32_t k1 = k0 + S2R_IR_SEGMENT < n_taps ? k0 + S2R_IR_SEGMENT : n_taps;
            float p = 0.0f;
            for (uint32_t k = k0; k < k1; k++) {
                const float t = ir[k] * x[-(ptrdiff_t)k];
                p = p + t;
            }
            r = r + p;
        }
        const float d = dry * x[0], w = wet * r;
        out[i] = d + w;
    }
    return S2R_OK;
}

// ---- per-bus feedback delay, both channels: the cross-feed couples them ----
int s2r_delay_reference(uint32_t delay_frames, float feedback, float cross, float dry, float wet, const float *x_lr, uint32_t frames,
                        float *history_lr, float *out_lr) {
    if (!delay_mix_in_range(feedback, cross, dry, wet) || delay_frames == 0 || delay_frames > S2R_MAX_DELAY_FRAMES) return S2R_ERR_PATCH_RANGE;
    if (!history_lr || (!x_lr && frames)) return S2R_ERR_INVALID;
    const size_t D = delay_frames, N = frames;
    std::vector<float> w(2 * (D + N));                           // W[-D .. N): the history, then the call's line signal
    std::memcpy(w.data(), history_lr, 2 * D * sizeof(float));
    for (size_t n = 0; n < N; n++)
        for (size_t c = 0; c < 2; c++) {
            const float x = x_lr[2 * n + c], t = w[2 * n + c], u = w[2 * n + (1 - c)];     // (frame n - D of W sits at index n)
            const float p = feedback * t, q = cross * u;
            const float s = x + p;
            w[2 * (n + D) + c] = s + q;
            if (out_lr) { const float d = dry * x, e = wet * t; out_lr[2 * n + c] = d + e; }
        }
    std::memcpy(history_lr, w.data() + 2 * N, 2 * D * sizeof(float));
    return S2R_OK;
}

// ---- per-bus chorus: V taps at triangle-modulated fractional delays into the INPUT's history; no recursion ----
uint32_t s2r_chorus_history_frames(float base, float depth) { return chorus_delay_in_range(base, depth) ? chorus_history(base, depth) : 0u; }

int s2r_chorus_reference(uint32_t voices, float base, float depth, uint32_t phase_inc, uint32_t spread, float dry, float wet, const float *x_lr,
                         uint32_t frames, float *history_lr, uint32_t *phase, float *out_lr) {
    if (!chorus_in_range(voices, base, depth, dry, wet)) return S2R_ERR_PATCH_RANGE;
    if (!history_lr || !phase || (!x_lr && frames)) return S2R_ERR_INVALID;
    const size_t H = chorus_history(base, depth), N = frames;
    std::vector<float> s(2 * (H + N));                           // x[-H .. N): the history, then the call's input
    std::memcpy(s.data(), history_lr, 2 * H * sizeof(float));
    if (N) std::memcpy(s.data() + 2 * H, x_lr, 2 * N * sizeof(float));
    const uint32_t phase0 = *phase;
    for (size_t n = 0; n < N && out_lr; n++)
        for (uint32_t c = 0; c < 2; c++) {
            float acc = 0.0f;
            for (uint32_t v = 0; v < voices; v++) {
                const uint32_t off = chorus_voice_offset(v, voices) + c * spread;
                const uint32_t p = phase0 + off + phase_inc * (uint32_t)n;
                const uint32_t q = p >> 8;
                const uint32_t h = q < (1u << 23) ? q : (1u << 24) - q;
                const float m = (float)h * 0x1p-23f;
                const float dm = depth * m;
                const float d = base + dm;
                const uint32_t i = (uint32_t)d;                  // (i + 1 <= H: d <= fl(base + depth) by monotonic rounding)
                const float f = d - (float)i;
                const float a = s[2 * (H + n - i) + c], bb = s[2 * (H + n - i - 1) + c];
                const float e = bb - a;
                const float g = f * e;
                const float tap = a + g;
                acc = v ? acc + tap : tap;
            }
            const float dx = dry * s[2 * (H + n) + c], wa = wet * acc;
            out_lr[2 * n + c] = dx + wa;
        }
    std::memcpy(history_lr, s.data() + 2 * N, 2 * H * sizeof(float));
    *phase = phase0 + phase_inc * (uint32_t)N;
    return S2R_OK;
}

// ---- per-bus parametric EQ: a cascade of biquads in transposed direct form II, both channels the same coefficients ----
int s2r_eq_reference(uint32_t n_bands, const float *coeffs, const float *x_lr, uint32_t frames, float *state, float *out_lr) {
    if (n_bands < 1u || !eq_in_range(n_bands, coeffs)) return S2R_ERR_PATCH_RANGE;
    if (!coeffs || !state || (!x_lr && frames)) return S2R_ERR_INVALID;
    for (uint32_t n = 0; n < frames; n++)
        for (uint32_t c = 0; c < 2; c++) {
            float x = x_lr[2 * (size_t)n + c];
            for (uint32_t k = 0; k < n_bands; k++) {
                const float *q = coeffs + 5 * k;
                float &s1 = state[4 * k + c], &s2 = state[4 * k + 2 + c];
                const float p0 = q[0] * x;
                const float y = p0 + s1;
                const float p1 = q[1] * x, r1 = q[3] * y;
                const float d1 = p1 - r1;
                const float p2 = q[2] * x, r2 = q[4] * y;
                s1 = d1 + s2;
                s2 = p2 - r2;
                x = y;
            }
            if (out_lr) out_lr[2 * (size_t)n + c] = x;
        }
    return S2R_OK;
}

// the Audio-EQ-Cookbook's bands with q as Q: binary64 throughout, divided by a0, rounded once to binary32
int s2r_eq_design(int kind, double freq_hz, double gain_db, double q, double sample_rate, float coeffs[5]) {
    if (std::isnan(freq_hz) || std::isnan(gain_db) || std::isnan(q) || std::isnan(sample_rate)) return S2R_ERR_PATCH_RANGE;
    if (kind < S2R_EQ_PEAK || kind > S2R_EQ_HIGHPASS || !(freq_hz > 0.0) || !(freq_hz < sample_rate / 2.0) || !(q > 0.0) || !(std::fabs(gain_db) <= 48.0))
        return S2R_ERR_PATCH_RANGE;
    if (!coeffs) return S2R_ERR_INVALID;
    const double w0 = 2.0 * 3.141592653589793 * freq_hz / sample_rate;
    const double cw = std::cos(w0), alpha = std::sin(w0) / (2.0 * q);
    const double A = std::pow(10.0, gain_db / 40.0);
    double b0, b1, b2, a0, a1, a2;
    if (kind == S2R_EQ_PEAK) {
        b0 = 1.0 + alpha * A; b1 = -2.0 * cw; b2 = 1.0 - alpha * A;
        a0 = 1.0 + alpha / A; a1 = -2.0 * cw; a2 = 1.0 - alpha / A;
    } else if (kind == S2R_EQ_LOW_SHELF) {
        const double t = 2.0 * std::sqrt(A) * alpha;
        b0 = A * ((A + 1.0) - (A - 1.0) * cw + t); b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * cw); b2 = A * ((A + 1.0) - (A - 1.0) * cw - t);
        a0 = (A + 1.0) + (A - 1.0) * cw + t; a1 = -2.0 * ((A - 1.0) + (A + 1.0) * cw); a2 = (A + 1.0) + (A - 1.0) * cw - t;
    } else if (kind == S2R_EQ_HIGH_SHELF) {
        const double t = 2.0 * std::sqrt(A) * alpha;
        b0 = A * ((A + 1.0) + (A - 1.0) * cw + t); b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cw); b2 = A * ((A + 1.0) + (A - 1.0) * cw - t);
        a0 = (A + 1.0) - (A - 1.0) * cw + t; a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cw); a2 = (A + 1.0) - (A - 1.0) * cw - t;
    } else {
        const double e = kind == S2R_EQ_LOWPASS ? 1.0 - cw : 1.0 + cw;
        b0 = e / 2.0; b1 = kind == S2R_EQ_LOWPASS ? e : -e; b2 = e / 2.0;
        a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha;
    }
    const float out[5] = {(float)(b0 / a0), (float)(b1 / a0), (float)(b2 / a0), (float)(a1 / a0), (float)(a2 / a0)};
    if (!eq_band_in_range(out)) return S2R_ERR_PATCH_RANGE;
    std::memcpy(coeffs, out, sizeof out);
    return S2R_OK;
}

// ---- per-bus dynamics: level of the key, target gain by table, attack / release ballistics, both channels one gain ----
static inline float dyn_target(const float *curve, float p) {
    const uint32_t lo = 0x33800000u;                             // the bits of 2^-24; 2^8 is lo + (512 << 19)
    if (!(p >= 5.9604644775390625e-08f)) return curve[0];
    if (p >= 256.0f) return curve[S2R_DYN_CURVE_POINTS - 1u];
    uint32_t u;
    std::memcpy(&u, &p, sizeof u);
    const uint32_t i = (u - lo) >> 19;
    const float f = (float)((u - lo) & 0x7ffffu) * 1.9073486328125e-06f;     // exact: 19 bits times 2^-19
    const float d = curve[i + 1u] - curve[i];
    const float m = f * d;
    return curve[i] + m;
}

int s2r_dynamics_reference(const float *curve, float a_att, float a_rel, const float *key_lr, const float *x_lr, uint32_t frames, float *y, float *out_lr,
                           float *min_gain) {
    if (!dyn_in_range(curve, a_att, a_rel) || (y && !dyn_state_in_range(*y))) return S2R_ERR_PATCH_RANGE;
    if (!curve || !y || (!x_lr && frames)) return S2R_ERR_INVALID;
    if (!key_lr) key_lr = x_lr;
    float g = *y, mn = INFINITY;
    for (uint32_t n = 0; n < frames; n++) {
        const float kl = std::fabs(key_lr[2 * (size_t)n]), kr = std::fabs(key_lr[2 * (size_t)n + 1]);
        const float p = kl > kr ? kl : kr;
        const float t = dyn_target(curve, p);
        const float a = t < g ? a_att : a_rel;
        const float d = g - t;
        const float m = a * d;
        g = t + m;
        mn = g < mn ? g : mn;
        if (out_lr) { out_lr[2 * (size_t)n] = x_lr[2 * (size_t)n] * g; out_lr[2 * (size_t)n + 1] = x_lr[2 * (size_t)n + 1] * g; }
    }
    *y = g;
    if (min_gain && frames) *min_gain = mn;
    return S2R_OK;
}

// a soft-knee compressor's table: binary64 throughout, each entry rounded once to binary32
int s2r_dynamics_curve(double threshold_db, double ratio, double knee_db, double makeup_db, float *curve) {
    if (std::isnan(threshold_db) || std::isnan(ratio) || std::isnan(knee_db) || std::isnan(makeup_db) || !(ratio >= 1.0) || !(knee_db >= 0.0))
        return S2R_ERR_PATCH_RANGE;
    if (!curve) return S2R_ERR_INVALID;
    const double slope = 1.0 / ratio - 1.0, W = knee_db;
    float out[S2R_DYN_CURVE_POINTS];
    for (uint32_t j = 0; j < S2R_DYN_CURVE_POINTS; j++) {
        const double level = std::ldexp(1.0 + (double)(j % 16u) / 16.0, -24 + (int)(j / 16u));
        const double o = 20.0 * std::log10(level) - threshold_db;
        double G;
        if (2.0 * o < -W) G = 0.0;
        else if (W > 0.0 && 2.0 * std::fabs(o) <= W) G = slope * (o + W / 2.0) * (o + W / 2.0) / (2.0 * W);
        else G = slope * o;
        out[j] = (float)std::pow(10.0, (G + makeup_db) / 20.0);
        if (!(out[j] >= 0.0f && out[j] <= 256.0f)) return S2R_ERR_PATCH_RANGE;
    }
    std::memcpy(curve, out, sizeof out);
    return S2R_OK;
}

float s2r_dynamics_coef(double ms, double sample_rate) {
    if (std::isnan(ms) || std::isnan(sample_rate) || ms < 0.0 || !(sample_rate > 0.0)) return NAN;
    if (ms == 0.0) return 0.0f;
    return (float)std::exp(-1.0 / (ms * 0.001 * sample_rate));
}

// ---- per-bus room reverb: eight damped feedback combs in parallel, four allpasses in series, per channel ----
size_t s2r_room_state_floats(const uint32_t *cd, const uint32_t *ad, uint32_t spread) {
    if (!cd || !ad || !room_delays_in_range(cd, ad, spread)) return 0;
    return room_state_count(cd, ad, spread);
}

int s2r_room_reference(const uint32_t *cd, const uint32_t *ad, uint32_t spread, float feedback, float damp, float g, float gain, float dry, float wet,
                       float cross, const float *x_lr, uint32_t frames, float *state, float *out_lr) {
    if (!room_delays_in_range(cd, ad, spread) || !room_levels_in_range(feedback, damp, g, gain, dry, wet, cross)) return S2R_ERR_PATCH_RANGE;
    if (!cd || !ad || !state || (!x_lr && frames)) return S2R_ERR_INVALID;
    const size_t total = room_state_count(cd, ad, spread);
    for (size_t k = 0; k < total; k++) if (!std::isfinite(state[k])) return S2R_ERR_PATCH_RANGE;
    uint32_t len[24], off[24];
    room_layout(cd, ad, spread, len, off);
    const float d1 = 1.0f - damp;
    // every line as history followed by the call's frames: frame n sits at len + n, what it reads at n
    std::vector<float> w[24];
    float f[16];
    for (uint32_t l = 0; l < 24u; l++) {
        w[l].assign((size_t)len[l] + frames, 0.0f);
        std::memcpy(w[l].data(), state + off[l], (size_t)len[l] * sizeof(float));
        if (l < 16u) f[l] = state[off[l] + len[l]];
    }
    for (uint32_t n = 0; n < frames; n++) {
        const float xl = x_lr[2 * (size_t)n], xr = x_lr[2 * (size_t)n + 1];
        const float s = xl + xr;
        const float in = s * gain;
        float v[2];
        for (uint32_t c = 0; c < 2u; c++) {
            float acc = 0.0f;
            for (uint32_t i = 0; i < S2R_ROOM_COMBS; i++) {
                const uint32_t l = c * 8u + i;
                const float o = w[l][n];
                const float p = o * d1;
                const float q = f[l] * damp;
                f[l] = p + q;
                const float r = f[l] * feedback;
                w[l][(size_t)len[l] + n] = in + r;
                acc = acc + o;
            }
            for (uint32_t j = 0; j < S2R_ROOM_ALLPASSES; j++) {
                const uint32_t l = 16u + c * 4u + j;
                const float b = w[l][n];
                const float y = b - acc;
                const float m = b * g;
                w[l][(size_t)len[l] + n] = acc + m;
                acc = y;
            }
            v[c] = acc;
        }
        if (out_lr) {
            const float x[2] = {xl, xr};
            for (uint32_t c = 0; c < 2u; c++) {
                const float a = dry * x[c];
                const float p = wet * v[c];
                const float q = cross * v[1u - c];
                const float t = p + q;
                out_lr[2 * (size_t)n + c] = a + t;
            }
        }
    }
    for (uint32_t l = 0; l < 24u; l++) {
        std::memcpy(state + off[l], w[l].data() + frames, (size_t)len[l] * sizeof(float));
        if (l < 16u) state[off[l] + len[l]] = f[l];
    }
    return S2R_OK;
}

int s2r_room_design(double sample_rate, double size, uint32_t *cd, uint32_t *ad, uint32_t *spread) {
    static const double kComb[S2R_ROOM_COMBS] = {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617}, kAll[S2R_ROOM_ALLPASSES] = {556, 441, 341, 225};
    if (!(sample_rate > 0.0) || !(size > 0.0) || !std::isfinite(sample_rate) || !std::isfinite(size)) return S2R_ERR_PATCH_RANGE;
    if (!cd || !ad || !spread) return S2R_ERR_INVALID;
    const double k = sample_rate / 44100.0 * size;
    auto scaled = [&](double v, uint32_t &to) {                  // to nearest, ties to even, as the host rounds
        const double r = std::nearbyint(v * k);
        if (!(r >= 0.0 && r <= (double)S2R_ROOM_MAX_DELAY)) return false;
        to = (uint32_t)r;
        return true;
    };
    uint32_t c[S2R_ROOM_COMBS], a[S2R_ROOM_ALLPASSES], sp;
    for (uint32_t i = 0; i < S2R_ROOM_COMBS; i++) if (!scaled(kComb[i], c[i])) return S2R_ERR_PATCH_RANGE;
    for (uint32_t j = 0; j < S2R_ROOM_ALLPASSES; j++) if (!scaled(kAll[j], a[j])) return S2R_ERR_PATCH_RANGE;
    if (!scaled(23.0, sp) || !room_delays_in_range(c, a, sp)) return S2R_ERR_PATCH_RANGE;
    std::memcpy(cd, c, sizeof c); std::memcpy(ad, a, sizeof a); *spread = sp;
    return S2R_OK;
}

// ---- per-bus drive: up to 4x, the table there, filtered and back down ----
}  // extern "C"

// the decimator's design of s2r_fill_oversampled (s2r_host.cpp) at S2R_DRIVE_TAPS taps: a Blackman-windowed sinc, cutoff 0.115 cycles per
// oversampled sample, unit DC gain; binary64, rounded once
const S2rDriveTaps &drive_taps() {
    static const S2rDriveTaps taps = [] {
        S2rDriveTaps t;
        double d[S2R_DRIVE_TAPS], sum = 0.0;
        const double PI = 3.14159265358979323846, fc = 0.115;
        for (uint32_t k = 0; k <= S2R_DRIVE_TAPS / 2u; k++) {            // the first half and the centre; the second half is its mirror, on bits
            const double at = (double)((int)k - (int)(S2R_DRIVE_TAPS - 1u) / 2);
            const double ideal = at == 0.0 ? 2.0 * fc : std::sin(2.0 * PI * fc * at) / (PI * at);
            const double w = 0.42 - 0.5 * std::cos(2.0 * PI * k / (S2R_DRIVE_TAPS - 1u)) + 0.08 * std::cos(4.0 * PI * k / (S2R_DRIVE_TAPS - 1u));
            d[k] = d[S2R_DRIVE_TAPS - 1u - k] = ideal * w;
        }
        for (uint32_t k = 0; k < S2R_DRIVE_TAPS; k++) sum += d[k];
        for (uint32_t k = 0; k < S2R_DRIVE_TAPS; k++) { t.h[k] = (float)(d[k] / sum); t.g[k] = 4.0f * t.h[k]; }
        return t;
    }();
    return taps;
}

extern "C" {

int s2r_drive_taps(float *h) {
    if (!h) return S2R_ERR_INVALID;
    std::memcpy(h, drive_taps().h, sizeof drive_taps().h);
    return S2R_OK;
}

int s2r_drive_reference(const float *curve, float pre, float dry, float wet, const float *x_lr, uint32_t frames, float *history, float *out_lr) {
    if (!drive_in_range(curve, pre, dry, wet)) return S2R_ERR_PATCH_RANGE;
    if (!curve || !history || (!x_lr && frames)) return S2R_ERR_INVALID;
    for (uint32_t k = 0; k < 2u * S2R_DRIVE_HISTORY; k++) if (!std::isfinite(history[k])) return S2R_ERR_PATCH_RANGE;
    const S2rDriveTaps &taps = drive_taps();
    constexpr uint32_t H = S2R_DRIVE_HISTORY, L = S2R_DRIVE_LATENCY;
    // per channel: x as history followed by the call (frame q at H + q), w for frames q >= -L (sample 4 q + p at 4 (L + q) + p)
    std::vector<float> x((size_t)H + frames), w(4u * ((size_t)L + frames));
    for (uint32_t c = 0; c < 2u; c++) {
        for (uint32_t k = 0; k < H; k++) x[k] = history[2u * k + c];
        for (uint32_t n = 0; n < frames; n++) x[(size_t)H + n] = x_lr[2u * (size_t)n + c];
        for (size_t f = 0; f < (size_t)L + frames; f++) {              // frame q = f - L: x[q - j] sits at f + L - j
            for (uint32_t p = 0; p < S2R_DRIVE_OVERSAMPLE; p++) {
                float u = 0.0f;
                for (uint32_t j = 0; p + 4u * j < S2R_DRIVE_TAPS; j++) {
                    const float t = taps.g[p + 4u * j] * x[f + L - j];
                    u = u + t;
                }
                w[4u * f + p] = drive_shape(curve, pre, u);
            }
        }
        for (uint32_t n = 0; n < frames && out_lr; n++) {
            float v = 0.0f;
            for (uint32_t k = 0; k < S2R_DRIVE_TAPS; k++) {                // w[4 n - k] sits at 4 (L + n) - k
                const float t = taps.h[k] * w[4u * ((size_t)L + n) - k];
                v = v + t;
            }
            const float a = dry * x[(size_t)H + n - L];
            const float b = wet * v;
            out_lr[2u * (size_t)n + c] = a + b;
        }
        for (uint32_t k = 0; k < H; k++) history[2u * k + c] = x[(size_t)frames + k];
    }
    return S2R_OK;
}

int s2r_drive_curve(uint32_t kind, double amount, float *table) {
    if (kind > S2R_DRIVE_FOLD) return S2R_ERR_PATCH_RANGE;
    if (kind != S2R_DRIVE_LINEAR && !(amount >= S2R_DRIVE_MIN_AMOUNT && amount <= S2R_DRIVE_MAX_AMOUNT)) return S2R_ERR_PATCH_RANGE;
    if (!table) return S2R_ERR_INVALID;
    auto clamp = [](double z) { return z < -1.0 ? -1.0 : z > 1.0 ? 1.0 : z; };
    const double th = kind == S2R_DRIVE_TANH ? std::tanh(amount) : 1.0;
    for (uint32_t i = 0; i < S2R_DRIVE_CURVE_POINTS; i++) {
        const double u = (double)i / 512.0 - 1.0, z = amount * u;
        double y = u;
        if (kind == S2R_DRIVE_TANH) y = std::tanh(z) / th;
        else if (kind == S2R_DRIVE_HARD) y = clamp(z);
        else if (kind == S2R_DRIVE_CUBIC) { const double v = clamp(z); y = 1.5 * v - 0.5 * (v * v * v); }
        else if (kind == S2R_DRIVE_FOLD) { double r = std::fmod(z + 1.0, 4.0); if (r < 0.0) r += 4.0; y = r < 2.0 ? r - 1.0 : 3.0 - r; }
        table[i] = (float)y;
    }
    return S2R_OK;
}

// ---- the master section: energies by the adjacent-pair tree over blocks of S2R_METER_BLOCK frames ----
static float master_energy(const float *v, uint32_t frames) {     // v: one channel of an interleaved pair (stride 2)
    float total = 0.0f;
    for (uint32_t k0 = 0; k0 < frames; k0 += S2R_METER_BLOCK) {
        float sq[S2R_METER_BLOCK];
        for (uint32_t j = 0; j < S2R_METER_BLOCK; j++) {
            const float x = k0 + j < frames ? v[2 * (size_t)(k0 + j)] : 0.0f;
            sq[j] = x * x;
        }
        for (uint32_t n = S2R_METER_BLOCK / 2u; n >= 1u; n /= 2u)
            for (uint32_t j = 0; j < n; j++) sq[j] = sq[2 * j] + sq[2 * j + 1];
        total = total + sq[0];
    }
    return total;
}

static float master_peak(const float *v, uint32_t frames) {
    float peak = 0.0f;
    for (uint32_t i = 0; i < frames; i++) { const float a = std::fabs(v[2 * (size_t)i]); peak = a > peak ? a : peak; }
    return peak;
}

int s2r_master_reference(const float *stems, uint32_t n_buses, uint32_t frames, const float *r0, const float *r1, float m0, float m1,
                         float *master_lr, float *peak, float *energy) {
    if (!unit_in_range(m0) || !unit_in_range(m1)) return S2R_ERR_PATCH_RANGE;
    if (n_buses == 0 || n_buses > S2R_MAX_BUSES || !r0 || !r1 || (!stems && frames)) return S2R_ERR_INVALID;
    for (uint32_t b = 0; b < n_buses; b++) if (!unit_in_range(r0[b]) || !unit_in_range(r1[b])) return S2R_ERR_PATCH_RANGE;
    const float fn = (float)frames;
    float dr[S2R_MAX_BUSES];
    for (uint32_t b = 0; b < n_buses; b++) { const float d = r1[b] - r0[b]; dr[b] = d / fn; }
    const float dm0 = m1 - m0, dm = dm0 / fn;
    std::vector<float> own;
    if (!master_lr) { own.resize(2 * (size_t)frames); master_lr = own.data(); }
    for (uint32_t i = 0; i < frames; i++) {
        const float fi = (float)i;
        for (uint32_t c = 0; c < 2; c++) {
            float t = 0.0f;
            for (uint32_t b = 0; b < n_buses; b++) {
                const float step = fi * dr[b];
                const float r = r0[b] + step;
                const float p = r * stems[((size_t)b * frames + i) * 2 + c];
                t = t + p;
            }
            const float step = fi * dm;
            const float g = m0 + step;
            master_lr[2 * (size_t)i + c] = g * t;
        }
    }
    for (uint32_t b = 0; b <= n_buses; b++)
        for (uint32_t c = 0; c < 2; c++) {
            const float *v = (b < n_buses ? stems + (size_t)b * frames * 2 : master_lr) + c;
            if (peak) peak[2 * b + c] = master_peak(v, frames);
            if (energy) energy[2 * b + c] = master_energy(v, frames);
        }
    return S2R_OK;
}

// ---- the master limiter: it shares its three constants with the kernel, nothing else ----
int s2r_limiter_reference(const float *x, uint32_t frames, float ceiling, uint32_t lookahead, uint32_t hold, float *xh, float *gh,
                          float *y, float *gain) {
    if (!limiter_in_range(ceiling, lookahead, hold)) return S2R_ERR_PATCH_RANGE;
    if ((!x && frames) || !xh || !gh) return S2R_ERR_INVALID;
    const size_t L = lookahead, H = hold, G = 2 * L + H, N = frames;
    const float c = ceiling, w = (float)(lookahead + 1u);
    std::vector<float> ge(G + N), xe(2 * (L + N)), m(L + N);
    std::memcpy(ge.data(), gh, G * sizeof(float));
    std::memcpy(xe.data(), xh, 2 * L * sizeof(float));
    if (N) std::memcpy(xe.data() + 2 * L, x, 2 * N * sizeof(float));
    for (size_t n = 0; n < N; n++) {
        const float al = std::fabs(x[2 * n]), ar = std::fabs(x[2 * n + 1]);
        const float p = al > ar ? al : ar;
        ge[G + n] = p > c ? c / p : 1.0f;
    }
    for (size_t j = 0; j < L + N; j++) {                         // m[j] is m[n = j - L]: the minimum of g[n - L - H .. n], ge[j .. j + L + H]
        float v = ge[j];
        for (size_t k = 1; k <= L + H; k++) v = ge[j + k] < v ? ge[j + k] : v;
        m[j] = v;
    }
    for (size_t n = 0; n < N; n++) {
        float acc = 0.0f;
        for (size_t k = 0; k <= L; k++) acc = acc + m[n + L - k];
        const float s = acc / w, gd = ge[G - L + n];
        const float sp = s < gd ? s : gd;
        if (gain) gain[n] = sp;
        if (y)
            for (size_t ch = 0; ch < 2; ch++) {
                float v = xe[2 * n + ch] * sp;
                v = v < -c ? -c : v;
                y[2 * n + ch] = v > c ? c : v;
            }
    }
    std::memcpy(gh, ge.data() + N, G * sizeof(float));
    std::memcpy(xh, xe.data() + 2 * N, 2 * L * sizeof(float));
    return S2R_OK;
}

// ---- its true-peak detector: it shares the constants and drive_taps() with the kernel, nothing else ----
int s2r_limiter_tp_reference(const float *x, uint32_t frames, float ceiling, uint32_t lookahead, uint32_t hold, float *xh, float *gh,
                             float *y, float *gain) {
    if (!limiter_in_range(ceiling, lookahead, hold)) return S2R_ERR_PATCH_RANGE;
    if ((!x && frames) || !xh || !gh) return S2R_ERR_INVALID;
    constexpr size_t D = S2R_LIMITER_TP_LATENCY, P = S2R_LIMITER_TP_HISTORY;
    const size_t L = lookahead, H = hold, G = 2 * L + H, N = frames, X = L + P;
    const float c = ceiling, w = (float)(lookahead + 1u);
    const S2rDriveTaps &taps = drive_taps();
    std::vector<float> ge(G + N), xe(2 * (X + N)), m(L + N);      // frame n of the call at xe[X + n]
    std::memcpy(ge.data(), gh, G * sizeof(float));
    std::memcpy(xe.data(), xh, 2 * X * sizeof(float));
    if (N) std::memcpy(xe.data() + 2 * X, x, 2 * N * sizeof(float));
    for (size_t n = 0; n < N; n++) {
        const float al = std::fabs(xe[2 * (X + n - D)]), ar = std::fabs(xe[2 * (X + n - D) + 1]);
        float d = al > ar ? al : ar;
        for (uint32_t ch = 0; ch < 2u; ch++)
            for (uint32_t p = 0; p < S2R_DRIVE_OVERSAMPLE; p++) {
                float u = 0.0f;
                for (uint32_t j = 0; p + 4u * j < S2R_DRIVE_TAPS; j++) {
                    const float t = taps.g[p + 4u * j] * xe[2 * (X + n - j) + ch];
                    u = u + t;
                }
                const float au = std::fabs(u);
                d = au > d ? au : d;
            }
        ge[G + n] = d > c ? c / d : 1.0f;
    }
    for (size_t j = 0; j < L + N; j++) {
        float v = ge[j];
        for (size_t k = 1; k <= L + H; k++) v = ge[j + k] < v ? ge[j + k] : v;
        m[j] = v;
    }
    for (size_t n = 0; n < N; n++) {
        float acc = 0.0f;
        for (size_t k = 0; k <= L; k++) acc = acc + m[n + L - k];
        const float s = acc / w, gd = ge[G - L + n];
        const float sp = s < gd ? s : gd;
        if (gain) gain[n] = sp;
        if (y)
            for (size_t ch = 0; ch < 2; ch++) {                  // x[n - L - 8]
                float v = xe[2 * (n + P - D) + ch] * sp;
                v = v < -c ? -c : v;
                y[2 * n + ch] = v > c ? c : v;
            }
    }
    std::memcpy(gh, ge.data() + N, G * sizeof(float));
    std::memcpy(xh, xe.data() + 2 * N, 2 * X * sizeof(float));
    return S2R_OK;
}

}  // extern "C"

// ---- per-bus flanger: one tap at a triangle-modulated fractional delay into the stage's own line signal, fed back ----
extern "C" {

uint32_t s2r_flanger_history_frames(float base, float depth) { return flanger_delay_in_range(base, depth) ? flanger_history(base, depth) : 0u; }

int s2r_flanger_reference(float base, float depth, uint32_t phase_inc, uint32_t spread, float feedback, float cross, float dry, float wet,
                          const float *x_lr, uint32_t frames, float *history_lr, uint32_t *phase, float *out_lr) {
    if (!flanger_in_range(base, depth, feedback, cross, dry, wet)) return S2R_ERR_PATCH_RANGE;
    if (!history_lr || !phase || (!x_lr && frames)) return S2R_ERR_INVALID;
    const size_t H = flanger_history(base, depth), N = frames;
    std::vector<float> w(2 * (H + N));                           // w[-H .. N): the history, then the call's line signal
    std::memcpy(w.data(), history_lr, 2 * H * sizeof(float));
    const uint32_t phase0 = *phase;
    for (size_t n = 0; n < N; n++) {
        float tap[2];
        for (uint32_t c = 0; c < 2; c++) {
            const uint32_t p = phase0 + c * spread + phase_inc * (uint32_t)n;
            const uint32_t q = p >> 8;
            const uint32_t h = q < (1u << 23) ? q : (1u << 24) - q;
            const float m = (float)h * 0x1p-23f;
            const float dm = depth * m;
            const float d = base + dm;
            const uint32_t i = (uint32_t)d;                      // (32 <= i and i + 1 <= H: base <= d <= fl(base + depth) by monotonic rounding)
            const float f = d - (float)i;
            const float a = w[2 * (H + n - i) + c], bb = w[2 * (H + n - i - 1) + c];
            const float e = bb - a;
            const float g = f * e;
            tap[c] = a + g;
        }
        for (uint32_t c = 0; c < 2; c++) {
            const float x = x_lr[2 * n + c];
            const float pf = feedback * tap[c], pc = cross * tap[1u - c];
            const float s = pf + pc;
            w[2 * (H + n) + c] = x + s;
            if (out_lr) { const float dx = dry * x, wt = wet * tap[c]; out_lr[2 * n + c] = dx + wt; }
        }
    }
    std::memcpy(history_lr, w.data() + 2 * N, 2 * H * sizeof(float));
    *phase = phase0 + phase_inc * (uint32_t)N;
    return S2R_OK;
}

}  // extern "C"

// ---- the master's loudness and true-peak meters: BS.1770's pre-filter, hop sums, and the readings from the hop rows ----
extern "C" {

int s2r_loudness_design(double sample_rate, float coeffs[10]) {
    if (!(sample_rate >= S2R_LOUDNESS_MIN_RATE && sample_rate <= S2R_LOUDNESS_MAX_RATE)) return S2R_ERR_PATCH_RANGE;
    if (!coeffs) return S2R_ERR_INVALID;
    const double PI = 3.14159265358979323846;
    {                                                            // stage 1: the high shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(PI * f0 / sample_rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        coeffs[0] = (float)((Vh + Vb * K / Q + K * K) / a0);
        coeffs[1] = (float)(2.0 * (K * K - Vh) / a0);
        coeffs[2] = (float)((Vh - Vb * K / Q + K * K) / a0);
        coeffs[3] = (float)(2.0 * (K * K - 1.0) / a0);
        coeffs[4] = (float)((1.0 - K / Q + K * K) / a0);
    }
    {                                                            // stage 2: the high-pass
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(PI * f0 / sample_rate);
        const double a0 = 1.0 + K / Q + K * K;
        coeffs[5] = 1.0f; coeffs[6] = -2.0f; coeffs[7] = 1.0f;
        coeffs[8] = (float)(2.0 * (K * K - 1.0) / a0);
        coeffs[9] = (float)((1.0 - K / Q + K * K) / a0);
    }
    return S2R_OK;
}

// one stage, one frame: the nine operations of a band of s2r_eq_reference
static inline float loudness_stage(const float *q, float x, float &s1, float &s2) {
    const float p0 = q[0] * x;
    const float y = p0 + s1;
    const float p1 = q[1] * x, r1 = q[3] * y;
    const float d1 = p1 - r1;
    const float p2 = q[2] * x, r2 = q[4] * y;
    s1 = d1 + s2;
    s2 = p2 - r2;
    return y;
}

int s2r_loudness_reference(const float coeffs[10], uint32_t hop, const float *stems, uint32_t n_buses, const float *master_lr, uint32_t frames,
                           float *state, uint32_t *pos, float *rows, size_t rows_capacity, size_t *n_rows, float true_peak[2]) {
    if (!loudness_in_range(coeffs, hop, S2R_LOUDNESS_MIN_HOPS) || n_buses > S2R_MAX_BUSES || (pos && *pos >= hop)) return S2R_ERR_PATCH_RANGE;
    if (!coeffs || !state || !pos || !n_rows || (frames && (!master_lr || (n_buses && !stems)))) return S2R_ERR_INVALID;
    const size_t made = ((size_t)*pos + frames) / hop;
    if (made && (!rows || rows_capacity < made * S2R_LOUDNESS_CHANNELS)) return S2R_ERR_INVALID;
    const size_t N = frames;
    float *const filt = state + S2R_LOUD_FILT, *const e = state + S2R_LOUD_SUMS, *const hist = state + S2R_LOUD_HIST;
    uint32_t at = *pos;
    size_t row = 0;
    for (size_t n = 0; n < N; n++) {
        for (uint32_t q = 0; q < S2R_LOUDNESS_CHANNELS; q++) {
            const uint32_t p = q >> 1, c = q & 1u;
            const float v = p == S2R_MAX_BUSES ? master_lr[2 * n + c] : (p < n_buses ? stems[2 * (p * N + n) + c] : 0.0f);
            float *const f = filt + 4 * q;
            const float y1 = loudness_stage(coeffs, v, f[0], f[1]);
            const float y2 = loudness_stage(coeffs + 5, y1, f[2], f[3]);
            const float z = y2 * y2;
            e[q] = e[q] + z;
        }
        if (++at == hop) {
            for (uint32_t q = 0; q < S2R_LOUDNESS_CHANNELS; q++) { rows[row * S2R_LOUDNESS_CHANNELS + q] = e[q]; e[q] = 0.0f; }
            row++;
            at = 0;
        }
    }
    // the true peak: x as the state's 16 frames followed by the call (frame n at 16 + n)
    const S2rDriveTaps &taps = drive_taps();
    constexpr size_t H = S2R_LOUD_HIST_FRAMES;
    float tp[2] = {0.0f, 0.0f};
    std::vector<float> x(H + N);
    for (uint32_t c = 0; c < 2u; c++) {
        for (size_t k = 0; k < H; k++) x[k] = hist[2 * k + c];
        for (size_t n = 0; n < N; n++) x[H + n] = master_lr[2 * n + c];
        for (size_t n = 0; n < N; n++) {
            const float a = std::fabs(x[H + n]);
            tp[c] = a > tp[c] ? a : tp[c];
            for (uint32_t p = 0; p < S2R_DRIVE_OVERSAMPLE; p++) {
                float u = 0.0f;
                for (uint32_t j = 0; p + 4u * j < S2R_DRIVE_TAPS; j++) {
                    const float t = taps.g[p + 4u * j] * x[H + n - j];
                    u = u + t;
                }
                const float au = std::fabs(u);
                tp[c] = au > tp[c] ? au : tp[c];
            }
        }
        for (size_t k = 0; k < H; k++) hist[2 * k + c] = x[N + k];
    }
    if (true_peak) { true_peak[0] = tp[0]; true_peak[1] = tp[1]; }
    *pos = at;
    *n_rows = row;
    return S2R_OK;
}

int s2r_loudness_readings(const float *rows, size_t n_hops, uint32_t hop, uint32_t programme, double out[3]) {
    if (!loudness_hop_in_range(hop) || programme >= S2R_LOUDNESS_PROGRAMMES) return S2R_ERR_PATCH_RANGE;
    if (!out || (n_hops && !rows)) return S2R_ERR_INVALID;
    const double ninf = -HUGE_VAL;
    auto t = [&](size_t i) { const float *r = rows + i * S2R_LOUDNESS_CHANNELS + 2u * programme; return (double)r[0] + (double)r[1]; };
    auto loud = [](double m) { return -0.691 + 10.0 * std::log10(m); };          // (log10(0) is -inf: silence reads -inf)
    auto block = [&](size_t j) { return (((t(j - 3) + t(j - 2)) + t(j - 1)) + t(j)) / (4.0 * hop); };
    out[0] = out[1] = out[2] = ninf;
    if (n_hops >= 4) out[0] = loud(block(n_hops - 1));
    if (n_hops >= 30) {
        double s = 0.0;
        for (size_t i = n_hops - 30; i < n_hops; i++) s = s + t(i);
        out[1] = loud(s / (30.0 * hop));
    }
    double sum = 0.0; size_t kept = 0;
    for (size_t j = 3; j < n_hops; j++) { const double m = block(j); if (loud(m) > -70.0) { sum = sum + m; kept++; } }
    if (kept) {
        const double rel = loud(sum / (double)kept) - 10.0;
        sum = 0.0; kept = 0;
        for (size_t j = 3; j < n_hops; j++) { const double m = block(j), l = loud(m); if (l > -70.0 && l > rel) { sum = sum + m; kept++; } }
        if (kept) out[2] = loud(sum / (double)kept);
    }
    return S2R_OK;
}

}  // extern "C"

// ---- the master's spectrum meter: window and twiddle tables, the radix-2 transform, and the readings from the rows ----
extern "C" {

int s2r_spectrum_window(uint32_t kind, uint32_t n_fft, float *window) {
    if (kind > S2R_WINDOW_BLACKMAN_HARRIS || !spectrum_fft_in_range(n_fft)) return S2R_ERR_PATCH_RANGE;
    if (!window) return S2R_ERR_INVALID;
    const double PI = 3.14159265358979323846;
    for (uint32_t i = 0; i < n_fft; i++) {
        const double x = 2.0 * PI * ((double)i / (double)n_fft);
        double w = 1.0;
        if (kind == S2R_WINDOW_HANN) w = 0.5 - 0.5 * std::cos(x);
        else if (kind == S2R_WINDOW_HAMMING) w = 0.54 - 0.46 * std::cos(x);
        else if (kind == S2R_WINDOW_BLACKMAN_HARRIS) w = 0.35875 - 0.48829 * std::cos(x) + 0.14128 * std::cos(2.0 * x) - 0.01168 * std::cos(3.0 * x);
        window[i] = (float)w;
    }
    return S2R_OK;
}

int s2r_spectrum_twiddles(uint32_t n_fft, float *tw) {
    if (!spectrum_fft_in_range(n_fft)) return S2R_ERR_PATCH_RANGE;
    if (!tw) return S2R_ERR_INVALID;
    const double PI = 3.14159265358979323846;
    const uint32_t N = n_fft, q = N / 4u, e = N / 8u;
    for (uint32_t j = 0; j <= e; j++) {                          // the first octant from libm, the rest from it by symmetry
        const double x = 2.0 * PI * ((double)j / (double)N);
        tw[2 * j] = (float)std::cos(x);
        tw[2 * j + 1] = j ? (float)-std::sin(x) : 0.0f;
    }
    for (uint32_t j = e + 1u; j <= q; j++) { tw[2 * j] = -tw[2 * (q - j) + 1]; tw[2 * j + 1] = -tw[2 * (q - j)]; }
    for (uint32_t j = q + 1u; j < N / 2u; j++) { tw[2 * j] = tw[2 * (j - q) + 1]; tw[2 * j + 1] = -tw[2 * (j - q)]; }
    return S2R_OK;
}

// one row of one programme: x holds the N frames, oldest first; v is [N][2] of scratch; p receives N / 2 + 1 values
static void spectrum_row(uint32_t N, uint32_t L, const float *window, const float *tw, const float *x, float *v, float *p) {
    for (uint32_t i = 0; i < N; i++) {
        uint32_t r = 0;
        for (uint32_t b = 0; b < L; b++) r |= ((i >> b) & 1u) << (L - 1u - b);
        v[2 * r] = window[i] * x[2 * i];
        v[2 * r + 1] = window[i] * x[2 * i + 1];
    }
    for (uint32_t s = 1; s <= L; s++) {
        const uint32_t m = 1u << s, h = m >> 1, step = N / m;
        for (uint32_t g = 0; g < N; g += m)
            for (uint32_t j = 0; j < h; j++) {
                const float wr = tw[2 * (j * step)], wi = tw[2 * (j * step) + 1];
                float *const a = v + 2 * (g + j), *const b = v + 2 * (g + j + h);
                const float p0 = wr * b[0], p1 = wi * b[1], p2 = wr * b[1], p3 = wi * b[0];
                const float tr = p0 - p1, ti = p2 + p3;
                const float ar = a[0], ai = a[1];
                a[0] = ar + tr; a[1] = ai + ti;
                b[0] = ar - tr; b[1] = ai - ti;
            }
    }
    for (uint32_t k = 0; k <= N / 2u; k++) {
        const float *const a = v + 2 * k, *const b = v + 2 * ((N - k) & (N - 1u));
        const float a0 = a[0] * a[0], a1 = a[1] * a[1], b0 = b[0] * b[0], b1 = b[1] * b[1];
        const float sa = a0 + a1, sb = b0 + b1;
        const float t = sa + sb;
        p[k] = t * 0.5f;
    }
}

int s2r_spectrum_reference(uint32_t n_fft, uint32_t hop, const float *window, const float *stems, uint32_t n_buses, const float *master_lr,
                           uint32_t frames, float *state, uint32_t *pos, float *rows, size_t rows_capacity, size_t *n_rows) {
    if (!spectrum_in_range(n_fft, hop, window, 1u) || n_buses > S2R_MAX_BUSES || (pos && *pos >= hop)) return S2R_ERR_PATCH_RANGE;
    if (!window || !state || !pos || !n_rows || (frames && (!master_lr || (n_buses && !stems)))) return S2R_ERR_INVALID;
    const size_t N = n_fft, F = frames, bins = N / 2u + 1u, row_floats = S2R_SPECTRUM_ROW(N);
    const size_t made = ((size_t)*pos + F) / hop;
    if (made && (!rows || rows_capacity < made * row_floats)) return S2R_ERR_INVALID;
    const uint32_t L = spectrum_log2(n_fft);
    std::vector<float> tw(N), x(2u * (N + F)), v(2u * N);
    (void)s2r_spectrum_twiddles(n_fft, tw.data());
    for (uint32_t p = 0; p < S2R_SPECTRUM_PROGRAMMES; p++) {
        float *const st = state + (size_t)p * 2u * N;
        const bool master = p == S2R_MAX_BUSES, fed = master || p < n_buses;
        std::memcpy(x.data(), st, 2u * N * sizeof(float));       // the stream: the state's N frames, then the call's
        const float *const src = master ? master_lr : (fed ? stems + (size_t)p * 2u * F : nullptr);
        for (size_t i = 0; i < 2u * F; i++) x[2u * N + i] = fed ? src[i] : 0.0f;
        for (size_t r = 0; r < made; r++) {
            float *const out = rows + r * row_floats + (size_t)p * bins;
            const size_t first = (r + 1u) * hop - *pos;          // the row's oldest frame in x: it ends at frame (r + 1) hop - pos - 1 of the call
            if (fed) spectrum_row(n_fft, L, window, tw.data(), x.data() + 2u * first, v.data(), out);
            else for (size_t k = 0; k < bins; k++) out[k] = 0.0f;
        }
        std::memcpy(st, x.data() + 2u * F, 2u * N * sizeof(float));
    }
    *pos = (uint32_t)(((size_t)*pos + F) % hop);
    *n_rows = made;
    return S2R_OK;
}

// q[k] of the host rule over the last n_avg rows of one programme
static int spectrum_q(const float *rows, size_t n_rows, uint32_t n_fft, const float *window, uint32_t programme, uint32_t n_avg, std::vector<double> &q) {
    if (!spectrum_fft_in_range(n_fft) || programme >= S2R_SPECTRUM_PROGRAMMES || n_avg == 0u || n_avg > n_rows) return S2R_ERR_PATCH_RANGE;
    if (!rows || !window) return S2R_ERR_INVALID;
    const size_t N = n_fft, bins = N / 2u + 1u, row_floats = S2R_SPECTRUM_ROW(N);
    double s1 = 0.0;
    for (size_t i = 0; i < N; i++) s1 = s1 + (double)window[i];
    q.resize(bins);
    for (size_t k = 0; k < bins; k++) {
        double sum = 0.0;
        for (size_t r = n_rows - n_avg; r < n_rows; r++) sum = sum + (double)rows[r * row_floats + (size_t)programme * bins + k];
        const double c = (k == 0 || k == N / 2u) ? 0.5 : 2.0;
        q[k] = c * (sum / (double)n_avg) / (s1 * s1);
    }
    return S2R_OK;
}

int s2r_spectrum_readings(const float *rows, size_t n_rows, uint32_t n_fft, const float *window, uint32_t programme, uint32_t n_avg, double *out_db,
                          size_t capacity) {
    std::vector<double> q;
    const int rc = spectrum_q(rows, n_rows, n_fft, window, programme, n_avg, q);
    if (rc != S2R_OK) return rc;
    if (!out_db || capacity < q.size()) return S2R_ERR_INVALID;
    for (size_t k = 0; k < q.size(); k++) out_db[k] = 10.0 * std::log10(q[k]);     // (log10(0) is -inf: silence reads -inf)
    return S2R_OK;
}

int s2r_spectrum_band_readings(const float *rows, size_t n_rows, uint32_t n_fft, const float *window, uint32_t programme, uint32_t n_avg, double sample_rate,
                               uint32_t bands_per_octave, double *out_db, double *centres, size_t capacity, size_t *n_bands) {
    const uint32_t bpo = bands_per_octave;
    if ((bpo != 1u && bpo != 3u && bpo != 6u && bpo != 12u) || !(sample_rate > 0.0) || !std::isfinite(sample_rate)) return S2R_ERR_PATCH_RANGE;
    std::vector<double> q;
    const int rc = spectrum_q(rows, n_rows, n_fft, window, programme, n_avg, q);
    if (rc != S2R_OK) return rc;
    if (!out_db || !n_bands) return S2R_ERR_INVALID;
    const double df = sample_rate / (double)n_fft, down = std::exp2(-1.0 / (2.0 * bpo)), up = std::exp2(1.0 / (2.0 * bpo));
    std::vector<double> db, fc;
    for (int i = -64 * (int)bpo; i <= 64 * (int)bpo; i++) {
        const double centre = 1000.0 * std::exp2((double)i / (double)bpo), lo = centre * down, hi = centre * up;
        if (!(lo >= df && hi <= sample_rate / 2.0)) continue;
        double power = 0.0;
        for (size_t k = 0; k < q.size(); k++) {
            const double b0 = ((double)k - 0.5) * df, b1 = ((double)k + 0.5) * df;
            const double a = lo > b0 ? lo : b0, b = hi < b1 ? hi : b1;
            if (b > a) power = power + q[k] * ((b - a) / df);
        }
        db.push_back(10.0 * std::log10(power)); fc.push_back(centre);
    }
    if (capacity < db.size()) return S2R_ERR_INVALID;
    for (size_t i = 0; i < db.size(); i++) { out_db[i] = db[i]; if (centres) centres[i] = fc[i]; }
    *n_bands = db.size();
    return S2R_OK;
}

}  // extern "C"

// ---- the master's PCM stage: dither, error-feedback noise shaping and rounding to B-bit integers ----
extern "C" {

static inline float pcm_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

int s2r_pcm_reference(uint32_t bits, uint32_t dither, const float *taps, uint32_t n_taps, uint32_t seed, const float *stems, uint32_t n_buses,
                      const float *master_lr, uint32_t frames, float *state, uint32_t *t, int32_t *pcm, uint32_t *clips) {
    if (!pcm_in_range(bits, dither, taps, n_taps) || n_buses > S2R_MAX_BUSES || !pcm_state_in_range(state)) return S2R_ERR_PATCH_RANGE;
    if ((n_taps && !taps) || !state || !t || (frames && (!master_lr || !pcm || (n_buses && !stems)))) return S2R_ERR_INVALID;
    const size_t N = frames;
    const uint32_t K = n_taps;
    const float G = std::ldexp(1.0f, (int)bits - 1), top = G - 1.0f;
    for (uint32_t q = 0; q < S2R_PCM_CHANNELS; q++) {
        const uint32_t p = q >> 1, c = q & 1u;
        float *const e = state + (size_t)q * S2R_PCM_MAX_TAPS;   // e[k - 1] = e[n - k]
        uint32_t n_clips = 0;
        for (size_t n = 0; n < N; n++) {
            const float x = p == S2R_MAX_BUSES ? master_lr[2 * n + c] : (p < n_buses ? stems[2 * (p * N + n) + c] : 0.0f);
            const float xc = x != x ? 0.0f : pcm_clamp(x, -2.0f, 2.0f);
            const float s = xc * G;
            float f = 0.0f;
            for (uint32_t k = K; k >= 1u; k--) {
                const float h = taps[k - 1u] * e[k - 1u];
                f = f + h;
            }
            const float w = s - f;
            const float d = pcm_dither_value(seed, *t + (uint32_t)n, q, dither);
            const float v = w + d;
            const float r = std::nearbyint(v);                   // (the default rounding mode: to nearest, ties to even)
            const float y = pcm_clamp(r, -G, top);
            if (y != r) n_clips++;
            pcm[2 * (p * N + n) + c] = (int32_t)y;
            const float diff = y - w;
            for (uint32_t k = S2R_PCM_MAX_TAPS - 1u; k >= 1u; k--) e[k] = k < K ? e[k - 1u] : 0.0f;
            e[0] = K ? pcm_clamp(diff, -2.0f, 2.0f) : 0.0f;
        }
        if (clips) clips[q] = n_clips;
    }
    *t += frames;
    return S2R_OK;
}

int s2r_pcm_dither(uint32_t seed, uint32_t t, uint32_t q, uint32_t kind, float *d) {
    if (q >= S2R_PCM_CHANNELS || kind > S2R_DITHER_TRI) return S2R_ERR_PATCH_RANGE;
    if (!d) return S2R_ERR_INVALID;
    *d = pcm_dither_value(seed, t, q, kind);
    return S2R_OK;
}

int s2r_pcm_pack(const int32_t *pcm, size_t count, uint32_t bits, uint32_t bytes_per_sample, uint8_t *out) {
    const uint32_t B = bytes_per_sample;
    if (bits < S2R_PCM_MIN_BITS || bits > S2R_PCM_MAX_BITS || B < 2u || B > 4u || 8u * B < bits) return S2R_ERR_PATCH_RANGE;
    if (count && (!pcm || !out)) return S2R_ERR_INVALID;
    const int32_t lo = -(int32_t)(1u << (bits - 1u)), hi = (int32_t)(1u << (bits - 1u)) - 1;
    for (size_t i = 0; i < count; i++) {
        if (pcm[i] < lo || pcm[i] > hi) return S2R_ERR_PATCH_RANGE;
        const uint32_t u = (uint32_t)pcm[i] << (8u * B - bits);  // two's complement, left-justified; the bytes past the container fall away
        for (uint32_t b = 0; b < B; b++) out[i * B + b] = (uint8_t)(u >> (8u * b));
    }
    return S2R_OK;
}

int s2r_pcm_shaper(uint32_t kind, float *taps, uint32_t *n_taps) {
    static const float kSets[6][S2R_PCM_MAX_TAPS] = {
        {},
        {1.0f},
        {2.0f, -1.0f},
        {1.623f, -0.982f, 0.109f},
        {2.033f, -2.165f, 1.959f, -1.590f, 0.6149f},
        {2.412f, -3.370f, 3.937f, -4.174f, 3.353f, -2.205f, 1.281f, -0.569f, 0.0847f}};
    static const uint32_t kCount[6] = {0u, 1u, 2u, 3u, 5u, 9u};
    if (kind > S2R_SHAPER_9TAP) return S2R_ERR_PATCH_RANGE;
    if (!taps || !n_taps) return S2R_ERR_INVALID;
    std::memcpy(taps, kSets[kind], sizeof kSets[kind]);
    *n_taps = kCount[kind];
    return S2R_OK;
}

}  // extern "C"

// ---- the master's sample-rate converter: a polyphase FIR by the rational ratio L / M ----
extern "C" {

int s2r_resampler_count(uint32_t L, uint32_t M, uint32_t ph, uint32_t frames, size_t *count) {
    if (!resampler_ratio_in_range(L, M) || ph >= M) return S2R_ERR_PATCH_RANGE;
    if (!count) return S2R_ERR_INVALID;
    *count = (size_t)resampler_count(L, M, ph, frames);
    return S2R_OK;
}

int s2r_resampler_reference(uint32_t L, uint32_t M, uint32_t T, const float *table, const float *stems, uint32_t n_buses, const float *master_lr,
                            uint32_t frames, float *state, uint32_t *ph, float *out, size_t capacity, size_t *count) {
    if (!resampler_in_range(L, M, T, table) || n_buses > S2R_MAX_BUSES || (ph && *ph >= M)) return S2R_ERR_PATCH_RANGE;
    if (!table || !state || !ph || !count || (frames && (!master_lr || (n_buses && !stems)))) return S2R_ERR_INVALID;
    const size_t N = frames, H = T - 1u;
    const uint64_t made = resampler_count(L, M, *ph, frames);
    if (made > capacity || (made && !out)) return S2R_ERR_INVALID;
    std::vector<float> xs(H + N);                                // the channel's history, oldest first, then the call: x[n] = xs[H + n]
    for (uint32_t q = 0; q < S2R_RESAMPLER_CHANNELS; q++) {
        const uint32_t p = q >> 1, c = q & 1u;
        float *const hist = state + (size_t)q * H;               // hist[j - 1] = x[-j]
        for (size_t j = 0; j < H; j++) xs[H - 1u - j] = hist[j];
        for (size_t n = 0; n < N; n++) xs[H + n] = p == S2R_MAX_BUSES ? master_lr[2 * n + c] : (p < n_buses ? stems[2 * (p * N + n) + c] : 0.0f);
        for (uint64_t i = 0; i < made; i++) {
            const uint64_t u = (uint64_t)*ph + i * M;
            const size_t n = (size_t)(u / L);
            const float *const h = table + (size_t)(u % L) * T;
            const float *const x = xs.data() + H + n;            // x[-k]: the frame k in front of frame n
            float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (uint32_t k = 0; k < T; k++) {
                const float t = h[k] * x[-(ptrdiff_t)k];
                a[k & 3u] = a[k & 3u] + t;
            }
            const float lo = a[0] + a[1], hi = a[2] + a[3];
            out[2 * ((size_t)p * capacity + (size_t)i) + c] = lo + hi;
        }
        for (size_t j = 0; j < H; j++) hist[j] = xs[H + N - 1u - j];
    }
    *ph = (uint32_t)((uint64_t)*ph + made * M - (uint64_t)frames * L);
    *count = (size_t)made;
    return S2R_OK;
}

// the modified Bessel function of the first kind and order 0, by its power series: every term positive, so no cancellation
static double resampler_i0(double x) {
    const double q = x * x * 0.25;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

int s2r_resampler_design(uint32_t L, uint32_t M, uint32_t T, double beta, double rolloff, float *table) {
    if (!resampler_in_range(L, M, T, nullptr) || !(beta >= 0.0 && beta <= 20.0) || !(rolloff > 0.0 && rolloff <= 1.0)) return S2R_ERR_PATCH_RANGE;
    if (!table) return S2R_ERR_INVALID;
    const double kPi = 3.14159265358979323846;
    const size_t N = (size_t)L * T;
    const double c = ((double)N - 1.0) * 0.5, fc = rolloff * 0.5 / (double)(L > M ? L : M), i0b = resampler_i0(beta);
    std::vector<double> g(N);
    for (size_t i = 0; i < N; i++) {
        const double d = (double)i - c, x = 2.0 * fc * d, r = d / c;
        const double sinc = x == 0.0 ? 1.0 : std::sin(kPi * x) / (kPi * x);
        const double inside = 1.0 - r * r;
        g[i] = 2.0 * fc * (double)L * sinc * (resampler_i0(beta * std::sqrt(inside > 0.0 ? inside : 0.0)) / i0b);
    }
    for (uint32_t p = 0; p < L; p++) {
        double sum = 0.0;
        for (uint32_t k = 0; k < T; k++) sum += g[(size_t)k * L + p];
        for (uint32_t k = 0; k < T; k++) table[(size_t)p * T + k] = (float)(g[(size_t)k * L + p] / sum);
    }
    return S2R_OK;
}

}  // extern "C"

// ---- the master's multiband compressor: a tree of crossover sections, a gain per band by the dynamics' rule, the bands
// added in band order ----
extern "C" {

// one section, one frame: the nine operations of s2r_eq_reference
static inline float multiband_section(const float *q, float x, float &s1, float &s2) {
    const float p0 = q[0] * x;
    const float y = p0 + s1;
    const float p1 = q[1] * x, r1 = q[3] * y;
    const float d1 = p1 - r1;
    const float p2 = q[2] * x, r2 = q[4] * y;
    s1 = d1 + s2;
    s2 = p2 - r2;
    return y;
}

int s2r_multiband_reference(uint32_t n_bands, const float *lp, const float *hp, const float *ap, const float *curves, const float *a_att,
                            const float *a_rel, const float *x_lr, uint32_t frames, float *state, float *out_lr, float *bands, float *min_gain) {
    const uint32_t B = n_bands;
    if (!multiband_in_range(B, lp, hp, ap, curves, a_att, a_rel)) return S2R_ERR_PATCH_RANGE;
    const uint32_t S = S2R_MULTIBAND_SECTIONS(B);
    if (state) {
        for (uint32_t i = 0; i < 4u * S; i++) if (!std::isfinite(state[i])) return S2R_ERR_PATCH_RANGE;
        for (uint32_t j = 0; j < B; j++) if (!dyn_state_in_range(state[4u * S + j])) return S2R_ERR_PATCH_RANGE;
    }
    if (!curves || !a_att || !a_rel || !state || (!x_lr && frames) || (B >= 2u && (!lp || !hp)) || (B >= 3u && !ap)) return S2R_ERR_INVALID;
    const S2rMultibandGraph g = multiband_graph(B);
    const float *rows[3] = {lp, hp, ap};
    float *y = state + 4u * S;
    float mn[S2R_MULTIBAND_MAX_BANDS] = {INFINITY, INFINITY, INFINITY, INFINITY};
    for (uint32_t n = 0; n < frames; n++) {
        float band[S2R_MULTIBAND_MAX_BANDS][2];
        for (uint32_t c = 0; c < 2u; c++) {
            const float x = x_lr[2 * (size_t)n + c];
            float v[15];
            for (uint32_t i = 0; i < g.n; i++)
                v[i] = multiband_section(rows[g.kind[i]] + 5u * g.row[i], g.src[i] < 0 ? x : v[g.src[i]], state[4u * i + c], state[4u * i + 2u + c]);
            for (uint32_t j = 0; j < B; j++) band[j][c] = g.leaf[j] < 0 ? x : v[g.leaf[j]];
        }
        float out[2] = {0.0f, 0.0f};
        for (uint32_t j = 0; j < B; j++) {
            const float l = std::fabs(band[j][0]), r = std::fabs(band[j][1]);
            const float p = l > r ? l : r;
            const float t = dyn_target(curves + (size_t)j * S2R_DYN_CURVE_POINTS, p);
            const float a = t < y[j] ? a_att[j] : a_rel[j];
            const float d = y[j] - t;
            const float m = a * d;
            y[j] = t + m;
            mn[j] = y[j] < mn[j] ? y[j] : mn[j];
            for (uint32_t c = 0; c < 2u; c++) {
                const float o = band[j][c] * y[j];
                out[c] = j ? out[c] + o : o;
                if (bands) bands[((size_t)j * frames + n) * 2u + c] = band[j][c];
            }
        }
        if (out_lr) { out_lr[2 * (size_t)n] = out[0]; out_lr[2 * (size_t)n + 1] = out[1]; }
    }
    if (min_gain && frames) for (uint32_t j = 0; j < B; j++) min_gain[j] = mn[j];
    return S2R_OK;
}

// the Audio-EQ-Cookbook's low-pass, high-pass and allpass at Q = 1 / sqrt 2: binary64 throughout, divided by a0, rounded once
int s2r_multiband_design(double sample_rate, const double *freqs_hz, uint32_t n_splits, float *lp, float *hp, float *ap) {
    if (n_splits > S2R_MULTIBAND_MAX_BANDS - 1u || !(sample_rate > 0.0) || !std::isfinite(sample_rate)) return S2R_ERR_PATCH_RANGE;
    for (uint32_t k = 0; k < n_splits && freqs_hz; k++)
        if (!(freqs_hz[k] > (k ? freqs_hz[k - 1u] : 0.0)) || !(freqs_hz[k] < sample_rate / 2.0)) return S2R_ERR_PATCH_RANGE;
    if (n_splits && (!freqs_hz || !lp || !hp || (n_splits >= 2u && !ap))) return S2R_ERR_INVALID;
    float out[3][S2R_MULTIBAND_MAX_BANDS - 1u][5];
    for (uint32_t k = 0; k < n_splits; k++) {
        const double w0 = 2.0 * 3.141592653589793 * freqs_hz[k] / sample_rate;
        const double cw = std::cos(w0), alpha = std::sin(w0) / (2.0 * 0.70710678118654752440);
        const double a0 = 1.0 + alpha, a1 = -2.0 * cw, a2 = 1.0 - alpha;
        const double b[3][3] = {{(1.0 - cw) / 2.0, 1.0 - cw, (1.0 - cw) / 2.0}, {(1.0 + cw) / 2.0, -(1.0 + cw), (1.0 + cw) / 2.0}, {a2, a1, a0}};
        for (uint32_t f = 0; f < 3u; f++) {
            float *q = out[f][k];
            q[0] = (float)(b[f][0] / a0); q[1] = (float)(b[f][1] / a0); q[2] = (float)(b[f][2] / a0); q[3] = (float)(a1 / a0); q[4] = (float)(a2 / a0);
            if (!eq_band_in_range(q)) return S2R_ERR_PATCH_RANGE;
        }
    }
    for (uint32_t k = 0; k < n_splits; k++) {
        std::memcpy(lp + 5u * k, out[0][k], sizeof out[0][k]);
        std::memcpy(hp + 5u * k, out[1][k], sizeof out[1][k]);
        if (k >= 1u) std::memcpy(ap + 5u * (k - 1u), out[2][k], sizeof out[2][k]);
    }
    return S2R_OK;
}

}  // extern "C"
