// s2r_host_post.cpp — the C entries of libs2r in front of the post-mix chain (s2r_post.h; include/s2r.h): the eight bus stages, bus
// returns, master fader, multiband compressor, limiter, both meters, the sample-rate converter and the PCM stage, and the chain's measurement getters.  The chain owns what they set; what is
// here checks the caller's values and the handle (s2r_handle.h).  Compiled with hipcc, -ffp-contract=off.
#include "s2r_handle.h"

#include <cmath>
#include <cstring>
#include <functional>

#include "s2r_rules.h"

using namespace s2r_host;

extern "C" {

// ---- the post-mix chain: the eight bus stages, master section, master limiter (s2r_post.h) ----
// Every entry below looks at its values first (they are wrong whatever the handle holds), then at the handle, quiesces where it touches
// the device, and calls into s->post for whatever is more than one value.  `what`: "bus reverbs are", "the master section is", ...
static int post_handle(const s2r_synth *s, const char *who, const char *what) {
    if (!s) return S2R_ERR_INVALID;
    if (!s->kids.empty() || s->parent) return set_err(const_cast<s2r_synth *>(s), S2R_ERR_INVALID, "%s: %s kept by single-device handles, not by a device list", who, what);
    return S2R_OK;
}

// the words in which the entries of a bus stage differ, by S2rBusStage
static const struct { const char *one, *are; } kStemWords[S2R_BUS_STAGES] = {{"EQ", "bus equalisers are"}, {"dynamics", "bus dynamics are"}, {"drive", "bus drives are"},
                                                                             {"flanger", "bus flangers are"}, {"chorus", "bus choruses are"}, {"delay", "bus delays are"},
                                                                             {"reverb", "bus reverbs are"}, {"room", "bus rooms are"}};

// The guard of an entry that reads or changes the effect one bus carries: the bus in range, a single-device handle, and the bus
// carries one.  `who` null: a getter, which answers for a bus without one too and leaves the handle's error text alone; `named`:
// the refusal of a bus without one begins with `who`.
static int stem_bus(const s2r_synth *s, S2rBusStage k, uint32_t bus, const char *who, bool named) {
    if (!who) return bus >= S2R_MAX_BUSES ? S2R_ERR_PATCH_RANGE : (!s || !s->kids.empty() || s->parent) ? S2R_ERR_INVALID : S2R_OK;
    s2r_synth *m = const_cast<s2r_synth *>(s);
    if (bus >= S2R_MAX_BUSES) return set_err(m, S2R_ERR_PATCH_RANGE, "%s: bus %u, below %u", who, bus, S2R_MAX_BUSES);
    S2R_TRY(post_handle(s, who, kStemWords[k].are));
    if (s->post.bus(k, bus).present()) return S2R_OK;
    if (named) return set_err(m, S2R_ERR_INVALID, "%s: bus %u carries no %s", who, bus, kStemWords[k].one);
    return set_err(m, S2R_ERR_INVALID, "bus %u carries no %s", bus, kStemWords[k].one);
}

// no resident kernel, the handle's device current, nothing left on its stream: in front of whatever reads or writes an effect's memory
static int quiet_device(s2r_synth *s) {
    S2R_QUIESCE(s);
    S2R_HIP(s, hipSetDevice(s->device));
    S2R_HIP(s, hipStreamSynchronize(s->stream));
    return S2R_OK;
}

// The common tail of the entries that set or clear an effect, behind their checks of the values and the handle: no fills in
// flight, a quiet stream, the chain's setter, and its error.
static int stem_set(s2r_synth *s, const char *who, const std::function<hipError_t(const S2rPostCtx &)> &set) {
    if (s->ring_count) return set_err(s, S2R_ERR_INVALID, "%s with fills of s2r_fill_begin in flight: s2r_fill_end first", who);
    S2R_TRY(quiet_device(s));
    const hipError_t e = set(post_ctx(s));
    if (e != hipSuccess) return set_err(s, e == hipErrorOutOfMemory ? S2R_ERR_OUT_OF_MEMORY : S2R_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return S2R_OK;
}

// An effect's history out (`get`, `count` the capacity) or in (`set`, `count` exact): it crosses the boundary as frames, oldest
// first, L then R.  A reverb of one tap has none, and nothing to copy.
static int stem_history(s2r_synth *s, S2rBusStage k, uint32_t bus, float *get, const float *set, size_t count, const char *who) {
    S2R_TRY(stem_bus(s, k, bus, who, true));
    const size_t h = s->post.bus(k, bus).history;
    if (set ? count != 2 * h : count < 2 * h) return set_err(s, S2R_ERR_INVALID, "%s: the history of bus %u is %zu floats, not %zu", who, bus, 2 * h, count);
    if (h == 0) return S2R_OK;
    if (!get && !set) return set_err(s, S2R_ERR_INVALID, "%s: null buffer", who);
    S2R_TRY(quiet_device(s));
    S2R_HIP(s, s->post.history(post_ctx(s), k, bus, get, set));
    return S2R_OK;
}

// An effect's whole state out (`get`, `count` the capacity) or in (`set`, `count` exact), for the stages whose checkpoint is every
// float of their line.  `values`: the stage's own check of a state coming in, behind the count's and in front of the device.
static int stem_state(s2r_synth *s, S2rBusStage k, uint32_t bus, float *get, const float *set, size_t count, const char *who,
                      int (*values)(s2r_synth *, const float *, size_t, const char *) = nullptr) {
    S2R_TRY(stem_bus(s, k, bus, who, true));
    const size_t n = s->post.bus(k, bus).floats;
    if (set ? count != n : count < n) {                          // (the dynamics' state is one float, and their text says so)
        if (n == 1u) return set_err(s, S2R_ERR_INVALID, "%s: the state of bus %u is 1 float, not %zu", who, bus, count);
        return set_err(s, S2R_ERR_INVALID, "%s: the state of bus %u is %zu floats, not %zu", who, bus, n, count);
    }
    if (!get && !set) return set_err(s, S2R_ERR_INVALID, "%s: null buffer", who);
    if (set && values) S2R_TRY(values(s, set, n, who));
    S2R_TRY(quiet_device(s));
    S2R_HIP(s, s->post.state(post_ctx(s), k, bus, get, set));
    return S2R_OK;
}

int s2r_set_bus_reverb(s2r_synth *s, uint32_t bus, const float *ir_l, const float *ir_r, uint32_t n_taps, float dry, float wet) {
    if (!unit_in_range(dry) || !unit_in_range(wet) || n_taps > S2R_MAX_IR_TAPS || bus >= S2R_MAX_BUSES)
        return set_err(s, S2R_ERR_PATCH_RANGE, "bus %u: %u taps, dry %g, wet %g: dry and wet lie in [0, 1], at most %u taps, the bus below %u", bus, n_taps,
                       (double)dry, (double)wet, S2R_MAX_IR_TAPS, S2R_MAX_BUSES);
    if (!ir_r) ir_r = ir_l;
    if (ir_l)
        for (uint32_t k = 0; k < n_taps; k++)
            if (!std::isfinite(ir_l[k]) || !std::isfinite(ir_r[k])) return set_err(s, S2R_ERR_PATCH_RANGE, "bus %u: tap %u is not finite", bus, k);
    S2R_TRY(post_handle(s, "s2r_set_bus_reverb", "bus reverbs are"));
    if (n_taps && !ir_l) return set_err(s, S2R_ERR_INVALID, "s2r_set_bus_reverb: %u taps and no response", n_taps);
    return stem_set(s, "s2r_set_bus_reverb", [&](const S2rPostCtx &c) { return s->post.set_reverb(c, bus, ir_l, ir_r, n_taps, dry, wet); });
}

int s2r_set_bus_reverb_mix(s2r_synth *s, uint32_t bus, float dry, float wet) {
    if (!unit_in_range(dry) || !unit_in_range(wet) || bus >= S2R_MAX_BUSES)
        return set_err(s, S2R_ERR_PATCH_RANGE, "bus %u: dry %g, wet %g: both lie in [0, 1], the bus below %u", bus, (double)dry, (double)wet, S2R_MAX_BUSES);
    S2R_TRY(stem_bus(s, S2R_BUS_REVERB, bus, "s2r_set_bus_reverb_mix", false));
    s->post.fx[bus].dry = dry; s->post.fx[bus].wet = wet;
    return S2R_OK;
}

int s2r_get_bus_reverb(const s2r_synth *s, uint32_t bus, uint32_t *n_taps, float *dry, float *wet) {
    S2R_TRY(stem_bus(s, S2R_BUS_REVERB, bus, nullptr, false));
    put(n_taps, s->post.fx[bus].n_taps); put(dry, s->post.fx[bus].dry); put(wet, s->post.fx[bus].wet);
    return S2R_OK;
}

int s2r_get_bus_reverb_history(s2r_synth *s, uint32_t bus, float *lr, size_t capacity) {
    return stem_history(s, S2R_BUS_REVERB, bus, lr, nullptr, capacity, "s2r_get_bus_reverb_history");
}

int s2r_set_bus_reverb_history(s2r_synth *s, uint32_t bus, const float *lr, size_t count) {
    static const float none = 0.0f;                              // (a null lr: refused by stem_history unless K = 1, which has no history)
    return stem_history(s, S2R_BUS_REVERB, bus, nullptr, lr ? lr : &none, lr ? count : (count ? (size_t)-1 : 0), "s2r_set_bus_reverb_history");
}

// ---- per-bus equalisers: the first bus stage, at the head of the chain ----
static int eq_values(s2r_synth *s, const char *who, uint32_t bus, uint32_t n_bands, const float *coeffs) {
    if (bus >= S2R_MAX_BUSES || !eq_in_range(n_bands, coeffs))
        return set_err(s, S2R_ERR_PATCH_RANGE, "%s: bus %u, %u bands: at most %u bands of finite coefficients (b0, b1, b2, a1, a2) with |a2| < 1 and "
                       "|a1| < 1 + a2, the bus below %u", who, bus, n_bands, S2R_EQ_MAX_BANDS, S2R_MAX_BUSES);
    return S2R_OK;
}

int s2r_set_bus_eq(s2r_synth *s, uint32_t bus, uint32_t n_bands, const float *coeffs) {
    S2R_TRY(eq_values(s, "s2r_set_bus_eq", bus, n_bands, coeffs));
    S2R_TRY(post_handle(s, "s2r_set_bus_eq", "bus equalisers are"));
    if (n_bands && !coeffs) return set_err(s, S2R_ERR_INVALID, "s2r_set_bus_eq: %u bands and no coefficients", n_bands);
    return stem_set(s, "s2r_set_bus_eq", [&](const S2rPostCtx &c) { return s->post.set_eq(c, bus, n_bands, coeffs); });
}

int s2r_set_bus_eq_coeffs(s2r_synth *s, uint32_t bus, uint32_t n_bands, const float *coeffs) {
    S2R_TRY(eq_values(s, "s2r_set_bus_eq_coeffs", bus, n_bands, coeffs));
    S2R_TRY(stem_bus(s, S2R_BUS_EQ, bus, "s2r_set_bus_eq_coeffs", true));
    S2rPostChain::BusEq &d = s->post.eq[bus];
    if (n_bands != d.n_bands || !coeffs) return set_err(s, S2R_ERR_INVALID, "s2r_set_bus_eq_coeffs: the EQ of bus %u has %u bands, not %u", bus, d.n_bands, n_bands);
    std::memcpy(d.c, coeffs, (size_t)n_bands * 5u * sizeof(float));          // (the state stays: the band moves without a restart)
    return S2R_OK;
}

int s2r_get_bus_eq(const s2r_synth *s, uint32_t bus, uint32_t *n_bands, float *coeffs, size_t capacity) {
    S2R_TRY(stem_bus(s, S2R_BUS_EQ, bus, nullptr, false));
    const S2rPostChain::BusEq &d = s->post.eq[bus];
    if (coeffs && capacity < 5u * (size_t)d.n_bands) return S2R_ERR_INVALID;
    put(n_bands, d.n_bands);
    if (coeffs) std::memcpy(coeffs, d.c, (size_t)d.n_bands * 5u * sizeof(float));
    return S2R_OK;
}

int s2r_get_bus_eq_state(s2r_synth *s, uint32_t bus, float *state, size_t capacity) {
    return stem_state(s, S2R_BUS_EQ, bus, state, nullptr, capacity, "s2r_get_bus_eq_state");
}

int s2r_set_bus_eq_state(s2r_synth *s, uint32_t bus, const float *state, size_t count) {
    return stem_state(s, S2R_BUS_EQ, bus, nullptr, state, state ? count : (size_t)-1, "s2r_set_bus_eq_state");
}

// ---- per-bus dynamics: the second bus stage, behind the equalisers ----
static int dyn_values(s2r_synth *s, const char *who, uint32_t bus, uint32_t key_bus, const float *curve, float a_att, float a_rel) {
    if (bus >= S2R_MAX_BUSES || key_bus >= S2R_MAX_BUSES || !dyn_in_range(curve, a_att, a_rel))
        return set_err(s, S2R_ERR_PATCH_RANGE, "%s: bus %u, key bus %u, attack %g, release %g: %u finite curve entries in [0, 256], both coefficients in "
                       "[0, 1), both buses below %u", who, bus, key_bus, (double)a_att, (double)a_rel, S2R_DYN_CURVE_POINTS, S2R_MAX_BUSES);
    return S2R_OK;
}

int s2r_set_bus_dynamics(s2r_synth *s, uint32_t bus, uint32_t key_bus, const float *curve, float a_att, float a_rel) {
    S2R_TRY(dyn_values(s, "s2r_set_bus_dynamics", bus, key_bus, curve, a_att, a_rel));
    S2R_TRY(post_handle(s, "s2r_set_bus_dynamics", "bus dynamics are"));
    if (!curve) return set_err(s, S2R_ERR_INVALID, "s2r_set_bus_dynamics: no curve");
    return stem_set(s, "s2r_set_bus_dynamics", [&](const S2rPostCtx &c) { return s->post.set_dyn(c, bus, key_bus, curve, a_att, a_rel, false); });
}

int s2r_clear_bus_dynamics(s2r_synth *s, uint32_t bus) {
    if (bus >= S2R_MAX_BUSES) return set_err(s, S2R_ERR_PATCH_RANGE, "s2r_clear_bus_dynamics: bus %u, below %u", bus, S2R_MAX_BUSES);
    S2R_TRY(post_handle(s, "s2r_clear_bus_dynamics", "bus dynamics are"));
    return stem_set(s, "s2r_clear_bus_dynamics", [&](const S2rPostCtx &c) { return s->post.set_dyn(c, bus, 0, nullptr, 0.0f, 0.0f, false); });
}

int s2r_set_bus_dynamics_params(s2r_synth *s, uint32_t bus, uint32_t key_bus, const float *curve, float a_att, float a_rel) {
    S2R_TRY(dyn_values(s, "s2r_set_bus_dynamics_params", bus, key_bus, curve, a_att, a_rel));
    S2R_TRY(stem_bus(s, S2R_BUS_DYN, bus, "s2r_set_bus_dynamics_params", true));
    if (!curve) return set_err(s, S2R_ERR_INVALID, "s2r_set_bus_dynamics_params: no curve");
    return stem_set(s, "s2r_set_bus_dynamics_params", [&](const S2rPostCtx &c) { return s->post.set_dyn(c, bus, key_bus, curve, a_att, a_rel, true); });   // (y stays)
}

int s2r_get_bus_dynamics(const s2r_synth *s, uint32_t bus, uint32_t *present, uint32_t *key_bus, float *curve, size_t capacity, float *a_att, float *a_rel) {
    S2R_TRY(stem_bus(s, S2R_BUS_DYN, bus, nullptr, false));
    const S2rPostChain::BusDyn &d = s->post.dyn[bus];
    if (d.present() && curve && capacity < S2R_DYN_CURVE_POINTS) return S2R_ERR_INVALID;
    put(present, d.present() ? 1u : 0u); put(key_bus, d.key); put(a_att, d.a_att); put(a_rel, d.a_rel);
    if (d.present() && curve) std::memcpy(curve, d.curve.data(), S2R_DYN_CURVE_POINTS * sizeof(float));
    return S2R_OK;
}

static int dyn_state(s2r_synth *s, uint32_t bus, float *get, const float *set, size_t count, const char *who) {
    if (set && count == 1u && !dyn_state_in_range(set[0])) return set_err(s, S2R_ERR_PATCH_RANGE, "%s: a gain of %g: finite and not below 0", who, (double)set[0]);
    return stem_state(s, S2R_BUS_DYN, bus, get, set, count, who);
}

int s2r_get_bus_dynamics_state(s2r_synth *s, uint32_t bus, float *state, size_t capacity) {
    return dyn_state(s, bus, state, nullptr, capacity, "s2r_get_bus_dynamics_state");
}

int s2r_set_bus_dynamics_state(s2r_synth *s, uint32_t bus, const float *state, size_t count) {
    return dyn_state(s, bus, nullptr, state, state ? count : (size_t)-1, "s2r_set_bus_dynamics_state");
}

int s2r_get_bus_dynamics_meter(const s2r_synth *s, uint32_t bus, float *min_gain) {
    S2R_TRY(stem_bus(s, S2R_BUS_DYN, bus, nullptr, false));
    put(min_gain, s->post.dyn[bus].min_gain);
    return S2R_OK;
}

// ---- per-bus drives: the third bus stage, behind the dynamics ----
static int drive_values(s2r_synth *s, const char *who, uint32_t bus, const float *curve, float pre, float dry, float wet) {
    if (bus >= S2R_MAX_BUSES || !drive_in_range(curve, pre, dry, wet))
        return set_err(s, S2R_ERR_PATCH_RANGE, "%s: bus %u, pre %g, dry %g, wet %g: %u finite curve entries, pre in [0, %g], dry and wet in [0, 1], the bus below %u",
                       who, bus, (double)pre, (double)dry, (double)wet, S2R_DRIVE_CURVE_POINTS, (double)S2R_DRIVE_MAX_PRE, S2R_MAX_BUSES);
    return S2R_OK;
}

int s2r_set_bus_drive(s2r_synth *s, uint32_t bus, const float *curve, float pre, float dry, float wet) {
    S2R_TRY(drive_values(s, "s2r_set_bus_drive", bus, curve, pre, dry, wet));
    S2R_TRY(post_handle(s, "s2r_set_bus_drive", kStemWords[S2R_BUS_DRIVE].are));
    if (!curve) return set_err(s, S2R_ERR_INVALID, "s2r_set_bus_drive: no curve");
    return stem_set(s, "s2r_set_bus_drive", [&](const S2rPostCtx &c) { return s->post.set_drive(c, bus, curve, pre, dry, wet, false); });
}

int s2r_clear_bus_drive(s2r_synth *s, uint32_t bus) {
    if (bus >= S2R_MAX_BUSES) return set_err(s, S2R_ERR_PATCH_RANGE, "s2r_clear_bus_drive: bus %u, below %u", bus, S2R_MAX_BUSES);
    S2R_TRY(post_handle(s, "s2r_clear_bus_drive", kStemWords[S2R_BUS_DRIVE].are));
    return stem_set(s, "s2r_clear_bus_drive", [&](const S2rPostCtx &c) { return s->post.set_drive(c, bus, nullptr, -1.0f, 0.0f, 0.0f, false); });
}

int s2r_set_bus_drive_params(s2r_synth *s, uint32_t bus, const float *curve, float pre, float dry, float wet) {
    S2R_TRY(drive_values(s, "s2r_set_bus_drive_params", bus, curve, pre, dry, wet));
    S2R_TRY(stem_bus(s, S2R_BUS_DRIVE, bus, "s2r_set_bus_drive_params", true));
    return stem_set(s, "s2r_set_bus_drive_params", [&](const S2rPostCtx &c) { return s->post.set_drive(c, bus, curve, pre, dry, wet, true); });   // (the history stays)
}

int s2r_get_bus_drive(const s2r_synth *s, uint32_t bus, uint32_t *present, float *curve, size_t capacity, float *pre, float *dry, float *wet) {
    S2R_TRY(stem_bus(s, S2R_BUS_DRIVE, bus, nullptr, false));
    const S2rPostChain::BusDrive &d = s->post.drive[bus];
    if (d.present() && curve && capacity < S2R_DRIVE_CURVE_POINTS) return S2R_ERR_INVALID;
    put(present, d.present() ? 1u : 0u); put(pre, d.pre); put(dry, d.dry); put(wet, d.wet);
    if (d.present() && curve) std::memcpy(curve, d.curve.data(), S2R_DRIVE_CURVE_POINTS * sizeof(float));
    return S2R_OK;
}

// the checkpoint pair: the room's state pair's checks, then the stem stages' copy
static int drive_history(s2r_synth *s, uint32_t bus, float *get, const float *set, size_t count, const char *who) {
    S2R_TRY(stem_bus(s, S2R_BUS_DRIVE, bus, who, true));
    const size_t n = 2u * S2R_DRIVE_HISTORY;
    if (set ? count != n : count < n) return set_err(s, S2R_ERR_INVALID, "%s: the history of bus %u is %zu floats, not %zu", who, bus, n, count);
    if (!get && !set) return set_err(s, S2R_ERR_INVALID, "%s: null buffer", who);
    if (set) for (size_t k = 0; k < n; k++) if (!std::isfinite(set[k])) return set_err(s, S2R_ERR_PATCH_RANGE, "%s: value %zu of the history is not finite", who, k);
    return stem_history(s, S2R_BUS_DRIVE, bus, get, set, count, who);
}

int s2r_get_bus_drive_history(s2r_synth *s, uint32_t bus, float *lr, size_t capacity) {
    return drive_history(s, bus, lr, nullptr, capacity, "s2r_get_bus_drive_history");
}

int s2r_set_bus_drive_history(s2r_synth *s, uint32_t bus, const float *lr, size_t count) {
    return drive_history(s, bus, nullptr, lr, lr ? count : (size_t)-1, "s2r_set_bus_drive_history");
}

// ---- per-bus flangers: the fourth bus stage, behind the drives and in front of the choruses ----
static int flanger_levels(s2r_synth *s, const char *who, uint32_t bus, float feedback, float cross, float dry, float wet) {
    if (bus >= S2R_MAX_BUSES || !delay_mix_in_range(feedback, cross, dry, wet))
        return set_err(s, S2R_ERR_PATCH_RANGE, "%s: bus %u, feedback %g, cross %g, dry %g, wet %g: feedback and cross in [-1, 1] with |feedback| + |cross| <= 1, dry and "
                       "wet in [0, 1], the bus below %u", who, bus, (double)feedback, (double)cross, (double)dry, (double)wet, S2R_MAX_BUSES);
    return S2R_OK;
}

int s2r_set_bus_flanger(s2r_synth *s, uint32_t bus, float base, float depth, uint32_t phase_inc, uint32_t spread, float feedback, float cross, float dry,
                        float wet) {
    if (!flanger_delay_in_range(base, depth))
        return set_err(s, S2R_ERR_PATCH_RANGE, "s2r_set_bus_flanger: bus %u, base %g, depth %g: base >= %g and depth >= 0 with base + depth <= %g frames", bus,
                       (double)base, (double)depth, (double)S2R_FLANGER_MIN_DELAY, (double)S2R_FLANGER_MAX_DELAY);
    S2R_TRY(flanger_levels(s, "s2r_set_bus_flanger", bus, feedback, cross, dry, wet));
    S2R_TRY(post_handle(s, "s2r_set_bus_flanger", kStemWords[S2R_BUS_FLANGER].are));
    return stem_set(s, "s2r_set_bus_flanger", [&](const S2rPostCtx &c) { return s->post.set_flanger(c, bus, base, depth, phase_inc, spread, feedback, cross, dry, wet); });
}

int s2r_clear_bus_flanger(s2r_synth *s, uint32_t bus) {
    if (bus >= S2R_MAX_BUSES) return set_err(s, S2R_ERR_PATCH_RANGE, "s2r_clear_bus_flanger: bus %u, below %u", bus, S2R_MAX_BUSES);
    S2R_TRY(post_handle(s, "s2r_clear_bus_flanger", kStemWords[S2R_BUS_FLANGER].are));
    return stem_set(s, "s2r_clear_bus_flanger", [&](const S2rPostCtx &c) { return s->post.set_flanger(c, bus, -1.0f, 0.0f, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f); });
}

int s2r_set_bus_flanger_params(s2r_synth *s, uint32_t bus, uint32_t phase_inc, uint32_t spread, float feedback, float cross, float dry, float wet) {
    S2R_TRY(flanger_levels(s, "s2r_set_bus_flanger_params", bus, feedback, cross, dry, wet));
    S2R_TRY(stem_bus(s, S2R_BUS_FLANGER, bus, "s2r_set_bus_flanger_params", true));
    S2rPostChain::BusFlanger &d = s->post.flanger[bus];          // (the phase and the line stay: the LFO bends, the comb retunes, nothing clicks)
    d.phase_inc = phase_inc; d.spread = spread; d.feedback = feedback; d.cross = cross; d.dry = dry; d.wet = wet;
    return S2R_OK;
}

int s2r_get_bus_flanger(const s2r_synth *s, uint32_t bus, float *base, float *depth, uint32_t *phase_inc, uint32_t *spread, float *feedback, float *cross,
                        float *dry, float *wet) {
    S2R_TRY(stem_bus(s, S2R_BUS_FLANGER, bus, nullptr, false));
    const S2rPostChain::BusFlanger &d = s->post.flanger[bus];
    put(base, d.base); put(depth, d.depth); put(phase_inc, d.phase_inc); put(spread, d.spread); put(feedback, d.feedback); put(cross, d.cross);
    put(dry, d.dry); put(wet, d.wet);
    return S2R_OK;
}

// (the flanger's phase lives on the host, as the chorus's)
int s2r_get_bus_flanger_state(s2r_synth *s, uint32_t bus, float *lr, size_t capacity, uint32_t *phase) {
    S2R_TRY(stem_history(s, S2R_BUS_FLANGER, bus, lr, nullptr, capacity, "s2r_get_bus_flanger_state"));
    put(phase, s->post.flanger[bus].phase);
    return S2R_OK;
}

int s2r_set_bus_flanger_state(s2r_synth *s, uint32_t bus, const float *lr, size_t count, uint32_t phase) {
    S2R_TRY(stem_history(s, S2R_BUS_FLANGER, bus, nullptr, lr, lr ? count : (size_t)-1, "s2r_set_bus_flanger_state"));
    s->post.flanger[bus].phase = phase;
    return S2R_OK;
}

// ---- per-bus rooms: the last bus stage, behind the reverbs ----
static int room_levels(s2r_synth *s, const char *who, uint32_t bus, float feedback, float damp, float g, float gain, float dry, float wet, float cross) {
    if (bus >= S2R_MAX_BUSES || !room_levels_in_range(feedback, damp, g, gain, dry, wet, cross))
        return set_err(s, S2R_ERR_PATCH_RANGE, "%s: bus %u, feedback %g, damp %g, g %g, gain %g, dry %g, wet %g, cross %g: feedback in [0, 1), g in (-1, 1), "
                       "the others in [0, 1], the bus below %u", who, bus, (double)feedback, (double)damp, (double)g, (double)gain, (double)dry, (double)wet,
                       (double)cross, S2R_MAX_BUSES);
    return S2R_OK;
}

int s2r_set_bus_room(s2r_synth *s, uint32_t bus, const uint32_t *cd, const uint32_t *ad, uint32_t spread, float feedback, float damp, float g, float gain,
                     float dry, float wet, float cross) {
    S2R_TRY(room_levels(s, "s2r_set_bus_room", bus, feedback, damp, g, gain, dry, wet, cross));
    if (!room_delays_in_range(cd, ad, spread))
        return set_err(s, S2R_ERR_PATCH_RANGE, "s2r_set_bus_room: bus %u, spread %u: every delay, and every delay plus the spread, in [%u, %u]", bus, spread,
                       S2R_ROOM_MIN_DELAY, S2R_ROOM_MAX_DELAY);
    S2R_TRY(post_handle(s, "s2r_set_bus_room", "bus rooms are"));
    if (!cd || !ad) return set_err(s, S2R_ERR_INVALID, "s2r_set_bus_room: no delays");
    const float levels[7] = {feedback, damp, g, gain, dry, wet, cross};
    return stem_set(s, "s2r_set_bus_room", [&](const S2rPostCtx &c) { return s->post.set_room(c, bus, cd, ad, spread, levels); });
}

int s2r_clear_bus_room(s2r_synth *s, uint32_t bus) {
    if (bus >= S2R_MAX_BUSES) return set_err(s, S2R_ERR_PATCH_RANGE, "s2r_clear_bus_room: bus %u, below %u", bus, S2R_MAX_BUSES);
    S2R_TRY(post_handle(s, "s2r_clear_bus_room", "bus rooms are"));
    return stem_set(s, "s2r_clear_bus_room", [&](const S2rPostCtx &c) { return s->post.set_room(c, bus, nullptr, nullptr, 0, nullptr); });
}

int s2r_set_bus_room_params(s2r_synth *s, uint32_t bus, float feedback, float damp, float g, float gain, float dry, float wet, float cross) {
    S2R_TRY(room_levels(s, "s2r_set_bus_room_params", bus, feedback, damp, g, gain, dry, wet, cross));
    S2R_TRY(stem_bus(s, S2R_BUS_ROOM, bus, "s2r_set_bus_room_params", true));
    const float levels[7] = {feedback, damp, g, gain, dry, wet, cross};
    return stem_set(s, "s2r_set_bus_room_params", [&](const S2rPostCtx &) { s->post.set_room_params(bus, levels); return hipSuccess; });   // (the state stays)
}

int s2r_get_bus_room(const s2r_synth *s, uint32_t bus, uint32_t *present, uint32_t *cd, uint32_t *ad, uint32_t *spread, float *levels) {
    if (bus >= S2R_MAX_BUSES) return S2R_ERR_PATCH_RANGE;
    if (!s || !s->kids.empty() || s->parent) return S2R_ERR_INVALID;
    const S2rPostChain::BusRoom &f = s->post.room[bus];
    put(present, f.present() ? 1u : 0u); put(spread, f.spread);
    if (cd) std::memcpy(cd, f.cd, sizeof f.cd);
    if (ad) std::memcpy(ad, f.ad, sizeof f.ad);
    if (levels) { const float l[7] = {f.feedback, f.damp, f.g, f.gain, f.dry, f.wet, f.cross}; std::memcpy(levels, l, sizeof l); }
    return S2R_OK;
}

// a room's state coming in is finite throughout
static int room_state_finite(s2r_synth *s, const float *set, size_t n, const char *who) {
    for (size_t k = 0; k < n; k++) if (!std::isfinite(set[k])) return set_err(s, S2R_ERR_PATCH_RANGE, "%s: value %zu of the state is not finite", who, k);
    return S2R_OK;
}

int s2r_get_bus_room_state(s2r_synth *s, uint32_t bus, float *state, size_t capacity) {
    return stem_state(s, S2R_BUS_ROOM, bus, state, nullptr, capacity, "s2r_get_bus_room_state");
}

int s2r_set_bus_room_state(s2r_synth *s, uint32_t bus, const float *state, size_t count) {
    return stem_state(s, S2R_BUS_ROOM, bus, nullptr, state, state ? count : (size_t)-1, "s2r_set_bus_room_state", room_state_finite);
}

// ---- per-bus choruses: in front of the delays ----
int s2r_set_bus_chorus(s2r_synth *s, uint32_t bus, uint32_t voices, float base, float depth, uint32_t phase_inc, uint32_t spread, float dry, float wet) {
    if ((voices && !chorus_in_range(voices, base, depth, dry, wet)) || bus >= S2R_MAX_BUSES)
        return set_err(s, S2R_ERR_PATCH_RANGE, "bus %u: a chorus of %u voices, base %g, depth %g, dry %g, wet %g: at most %u voices, base >= 1 and depth >= 0 with "
                       "base + depth <= %g frames, dry and wet in [0, 1], the bus below %u", bus, voices, (double)base, (double)depth, (double)dry, (double)wet,
                       S2R_CHORUS_MAX_VOICES, (double)S2R_CHORUS_MAX_DELAY, S2R_MAX_BUSES);
    S2R_TRY(post_handle(s, "s2r_set_bus_chorus", "bus choruses are"));
    return stem_set(s, "s2r_set_bus_chorus", [&](const S2rPostCtx &c) { return s->post.set_chorus(c, bus, voices, base, depth, phase_inc, spread, dry, wet); });
}

int s2r_set_bus_chorus_mix(s2r_synth *s, uint32_t bus, float dry, float wet) {
    if (!chorus_mix_in_range(dry, wet) || bus >= S2R_MAX_BUSES)
        return set_err(s, S2R_ERR_PATCH_RANGE, "bus %u: dry %g, wet %g: dry and wet lie in [0, 1], the bus below %u", bus, (double)dry, (double)wet, S2R_MAX_BUSES);
    S2R_TRY(stem_bus(s, S2R_BUS_CHORUS, bus, "s2r_set_bus_chorus_mix", false));
    s->post.chorus[bus].dry = dry; s->post.chorus[bus].wet = wet;
    return S2R_OK;
}

int s2r_set_bus_chorus_rate(s2r_synth *s, uint32_t bus, uint32_t phase_inc, uint32_t spread) {
    S2R_TRY(stem_bus(s, S2R_BUS_CHORUS, bus, "s2r_set_bus_chorus_rate", false));
    s->post.chorus[bus].phase_inc = phase_inc; s->post.chorus[bus].spread = spread;      // (the phase and the history stay: the LFO bends, nothing clicks)
    return S2R_OK;
}

int s2r_get_bus_chorus(const s2r_synth *s, uint32_t bus, uint32_t *voices, float *base, float *depth, uint32_t *phase_inc, uint32_t *spread, float *dry,
                       float *wet) {
    S2R_TRY(stem_bus(s, S2R_BUS_CHORUS, bus, nullptr, false));
    const S2rPostChain::BusChorus &d = s->post.chorus[bus];
    put(voices, d.voices); put(base, d.base); put(depth, d.depth); put(phase_inc, d.phase_inc); put(spread, d.spread); put(dry, d.dry); put(wet, d.wet);
    return S2R_OK;
}

// (the chorus's phase lives on the host)
int s2r_get_bus_chorus_state(s2r_synth *s, uint32_t bus, float *lr, size_t capacity, uint32_t *phase) {
    S2R_TRY(stem_history(s, S2R_BUS_CHORUS, bus, lr, nullptr, capacity, "s2r_get_bus_chorus_state"));
    put(phase, s->post.chorus[bus].phase);
    return S2R_OK;
}

int s2r_set_bus_chorus_state(s2r_synth *s, uint32_t bus, const float *lr, size_t count, uint32_t phase) {
    S2R_TRY(stem_history(s, S2R_BUS_CHORUS, bus, nullptr, lr, lr ? count : (size_t)-1, "s2r_set_bus_chorus_state"));
    s->post.chorus[bus].phase = phase;
    return S2R_OK;
}

// ---- per-bus feedback delays: in front of the reverbs ----
int s2r_set_bus_delay(s2r_synth *s, uint32_t bus, uint32_t delay_frames, float feedback, float cross, float dry, float wet) {
    if (!delay_mix_in_range(feedback, cross, dry, wet) || delay_frames > S2R_MAX_DELAY_FRAMES || bus >= S2R_MAX_BUSES)
        return set_err(s, S2R_ERR_PATCH_RANGE, "bus %u: a delay of %u frames, feedback %g, cross %g, dry %g, wet %g: feedback and cross lie in [-1, 1] with "
                       "|feedback| + |cross| <= 1, dry and wet in [0, 1], at most %u frames, the bus below %u", bus, delay_frames, (double)feedback, (double)cross,
                       (double)dry, (double)wet, S2R_MAX_DELAY_FRAMES, S2R_MAX_BUSES);
    S2R_TRY(post_handle(s, "s2r_set_bus_delay", "bus delays are"));
    return stem_set(s, "s2r_set_bus_delay", [&](const S2rPostCtx &c) { return s->post.set_delay(c, bus, delay_frames, feedback, cross, dry, wet); });
}

int s2r_set_bus_delay_mix(s2r_synth *s, uint32_t bus, float feedback, float cross, float dry, float wet) {
    if (!delay_mix_in_range(feedback, cross, dry, wet) || bus >= S2R_MAX_BUSES)
        return set_err(s, S2R_ERR_PATCH_RANGE, "bus %u: feedback %g, cross %g, dry %g, wet %g: feedback and cross lie in [-1, 1] with |feedback| + |cross| <= 1, "
                       "dry and wet in [0, 1], the bus below %u", bus, (double)feedback, (double)cross, (double)dry, (double)wet, S2R_MAX_BUSES);
    S2R_TRY(stem_bus(s, S2R_BUS_DELAY, bus, "s2r_set_bus_delay_mix", false));
    S2rPostChain::BusDelay &d = s->post.delay[bus];
    d.feedback = feedback; d.cross = cross; d.dry = dry; d.wet = wet;
    return S2R_OK;
}

int s2r_get_bus_delay(const s2r_synth *s, uint32_t bus, uint32_t *delay_frames, float *feedback, float *cross, float *dry, float *wet) {
    S2R_TRY(stem_bus(s, S2R_BUS_DELAY, bus, nullptr, false));
    const S2rPostChain::BusDelay &d = s->post.delay[bus];
    put(delay_frames, d.history); put(feedback, d.feedback); put(cross, d.cross); put(dry, d.dry); put(wet, d.wet);
    return S2R_OK;
}

int s2r_get_bus_delay_history(s2r_synth *s, uint32_t bus, float *lr, size_t capacity) {
    return stem_history(s, S2R_BUS_DELAY, bus, lr, nullptr, capacity, "s2r_get_bus_delay_history");
}

int s2r_set_bus_delay_history(s2r_synth *s, uint32_t bus, const float *lr, size_t count) {
    return stem_history(s, S2R_BUS_DELAY, bus, nullptr, lr, lr ? count : (size_t)-1, "s2r_set_bus_delay_history");
}

// ---- the master section ----
int s2r_set_bus_return(s2r_synth *s, uint32_t bus, float level) {
    if (!unit_in_range(level) || bus >= S2R_MAX_BUSES)
        return set_err(s, S2R_ERR_PATCH_RANGE, "bus %u: return %g: the level lies in [0, 1], the bus below %u", bus, (double)level, S2R_MAX_BUSES);
    S2R_TRY(post_handle(s, "s2r_set_bus_return", "the master section is"));
    s->post.master.ret[bus] = level;
    return S2R_OK;
}

int s2r_get_bus_return(const s2r_synth *s, uint32_t bus, float *level, float *applied) {
    if (bus >= S2R_MAX_BUSES) return S2R_ERR_PATCH_RANGE;
    if (!s || !s->kids.empty() || s->parent) return S2R_ERR_INVALID;
    put(level, s->post.master.ret[bus]); put(applied, s->post.master.ret_app[bus]);
    return S2R_OK;
}

int s2r_set_master_fader(s2r_synth *s, float level) {
    if (!unit_in_range(level)) return set_err(s, S2R_ERR_PATCH_RANGE, "master fader %g: the level lies in [0, 1]", (double)level);
    S2R_TRY(post_handle(s, "s2r_set_master_fader", "the master section is"));
    s->post.master.fader = level;
    return S2R_OK;
}

int s2r_get_master_fader(const s2r_synth *s, float *level, float *applied) {
    if (!s || !s->kids.empty() || s->parent) return S2R_ERR_INVALID;
    put(level, s->post.master.fader); put(applied, s->post.master.fader_app);
    return S2R_OK;
}

int s2r_snap_master(s2r_synth *s) {
    S2R_TRY(post_handle(s, "s2r_snap_master", "the master section is"));
    s->post.snap_master();
    return S2R_OK;
}

int s2r_get_meters(const s2r_synth *s, uint32_t *n_buses, float *peak, float *energy, size_t capacity) {
    if (!s || !s->kids.empty() || s->parent || !s->post.master.metered) return S2R_ERR_INVALID;
    const S2rPostChain::Master &ms = s->post.master;
    const size_t n = ((size_t)ms.meter_buses + 1u) * 2u;
    if (capacity < n) return S2R_ERR_INVALID;
    if (n_buses) *n_buses = ms.meter_buses;
    if (peak) std::memcpy(peak, ms.peak, n * sizeof(float));
    if (energy) std::memcpy(energy, ms.energy, n * sizeof(float));
    return S2R_OK;
}

// ---- the master limiter ----
int s2r_set_master_limiter_ex(s2r_synth *s, float ceiling, uint32_t lookahead, uint32_t hold, uint32_t detector) {
    if (!limiter_in_range(ceiling, lookahead, hold) || detector > S2R_LIMITER_TRUE_PEAK)
        return set_err(s, S2R_ERR_PATCH_RANGE, "master limiter: ceiling %g, lookahead %u, hold %u, detector %u: the ceiling lies in [2^-%d, 2^%d], the lookahead in 1 .. %u, the hold in 0 .. %u, the detector is 0 or 1",
                       (double)ceiling, lookahead, hold, detector, S2R_LIMITER_CEILING_LOG2, S2R_LIMITER_CEILING_LOG2, S2R_LIMITER_MAX_LOOKAHEAD, S2R_LIMITER_MAX_HOLD);
    S2R_TRY(post_handle(s, "s2r_set_master_limiter", "the master limiter is"));
    s->post.set_limiter(ceiling, lookahead, hold, detector);
    return S2R_OK;
}

int s2r_set_master_limiter(s2r_synth *s, float ceiling, uint32_t lookahead, uint32_t hold) { return s2r_set_master_limiter_ex(s, ceiling, lookahead, hold, S2R_LIMITER_SAMPLE_PEAK); }

int s2r_clear_master_limiter(s2r_synth *s) {
    S2R_TRY(post_handle(s, "s2r_clear_master_limiter", "the master limiter is"));
    s->post.set_limiter(0.0f, 0, 0, S2R_LIMITER_SAMPLE_PEAK);
    return S2R_OK;
}

int s2r_get_master_limiter(const s2r_synth *s, float *ceiling, uint32_t *lookahead, uint32_t *hold) {
    if (!s || !s->kids.empty() || s->parent) return S2R_ERR_INVALID;
    put(ceiling, s->post.limiter.ceiling); put(lookahead, s->post.limiter.lookahead); put(hold, s->post.limiter.hold);
    return S2R_OK;
}

int s2r_get_master_limiter_detector(const s2r_synth *s, uint32_t *detector) {
    if (!s || !s->kids.empty() || s->parent || !detector) return S2R_ERR_INVALID;
    *detector = s->post.limiter.detector;
    return S2R_OK;
}

// A master stage's state for a getter: where the device holds it, it is fetched once into the stage's host copy, and kept until the next fill.
static int mirror_fetch(s2r_synth *s, S2rMirror &m, const char *who) {
    if (m.host_valid) return S2R_OK;
    if (s->ring_count) return set_err(s, S2R_ERR_INVALID, "%s with fills of s2r_fill_begin in flight: s2r_fill_end first", who);
    S2R_QUIESCE(s);
    S2R_HIP(s, hipSetDevice(s->device));
    S2R_HIP(s, m.fetch(s->stream));
    return S2R_OK;
}

static int limiter_state(s2r_synth *s, float *get_x, float *get_g, const float *set_x, const float *set_g, size_t n_x, size_t n_g, const char *who) {
    S2R_TRY(post_handle(s, who, "the master limiter is"));
    S2rPostChain::Limiter &lm = s->post.limiter;
    if (!lm.lookahead) return set_err(s, S2R_ERR_INVALID, "%s: no master limiter is set", who);
    const size_t nx = lm.n_x(), ng = lm.n_g();
    const bool set = set_x || set_g;
    if (set ? (n_x != nx || n_g != ng) : (n_x < nx || n_g < ng))
        return set_err(s, S2R_ERR_INVALID, "%s: the state is %zu and %zu floats, not %zu and %zu", who, nx, ng, n_x, n_g);
    if (set ? (!set_x || !set_g) : (!get_x || !get_g)) return set_err(s, S2R_ERR_INVALID, "%s: null buffer", who);
    if (set) {
        for (size_t i = 0; i < ng; i++)
            if (!unit_in_range(set_g[i])) return set_err(s, S2R_ERR_PATCH_RANGE, "%s: gain %zu is %g, outside [0, 1]", who, i, (double)set_g[i]);
        s->post.set_limiter_state(set_x, set_g);
        return S2R_OK;
    }
    S2R_TRY(mirror_fetch(s, lm.state, who));
    std::memcpy(get_x, lm.state.host.data(), nx * sizeof(float));
    std::memcpy(get_g, lm.state.host.data() + nx, ng * sizeof(float));
    return S2R_OK;
}

int s2r_get_limiter_state(s2r_synth *s, float *xh, size_t n_x, float *gh, size_t n_g) { return limiter_state(s, xh, gh, nullptr, nullptr, n_x, n_g, "s2r_get_limiter_state"); }

int s2r_set_limiter_state(s2r_synth *s, const float *xh, size_t n_x, const float *gh, size_t n_g) {
    if (!s) return S2R_ERR_INVALID;
    if (!xh || !gh) return set_err(s, S2R_ERR_INVALID, "s2r_set_limiter_state: null buffer");
    return limiter_state(s, nullptr, nullptr, xh, gh, n_x, n_g, "s2r_set_limiter_state");
}

int s2r_get_limiter_meters(const s2r_synth *s, float *min_gain, float *out_peak) {
    if (!s || !s->kids.empty() || s->parent || !s->post.limiter.metered) return S2R_ERR_INVALID;
    put(min_gain, s->post.limiter.min_gain); put(out_peak, s->post.limiter.out_peak);
    return S2R_OK;
}

// ---- the master's multiband compressor, between the master fader and the limiter ----
// the values of a set, wrong whatever the handle holds: the ranges first, then the arrays that have rows
static int multiband_values(s2r_synth *s, const char *who, uint32_t B, const float *lp, const float *hp, const float *ap, const float *curves, const float *a_att,
                            const float *a_rel) {
    if (!multiband_in_range(B, lp, hp, ap, curves, a_att, a_rel))
        return set_err(s, S2R_ERR_PATCH_RANGE, "%s: %u bands: 1 .. %u bands, every coefficient finite and every section inside the stability triangle, every curve entry in [0, 256], every retention coefficient in [0, 1)",
                       who, B, S2R_MULTIBAND_MAX_BANDS);
    S2R_TRY(post_handle(s, who, "the master multiband compressor is"));
    if (!curves || !a_att || !a_rel || (B >= 2u && (!lp || !hp)) || (B >= 3u && !ap)) return set_err(s, S2R_ERR_INVALID, "%s: null array", who);
    return S2R_OK;
}

// the guard of the entries that need the stage set
static int multiband_set(const s2r_synth *s, const char *who) {
    S2R_TRY(post_handle(s, who, "the master multiband compressor is"));
    if (!s->post.mb.n_bands) return set_err(const_cast<s2r_synth *>(s), S2R_ERR_INVALID, "%s: no master multiband compressor is set", who);
    return S2R_OK;
}

int s2r_set_master_multiband(s2r_synth *s, uint32_t n_bands, const float *lp, const float *hp, const float *ap, const float *curves, const float *a_att,
                             const float *a_rel) {
    S2R_TRY(multiband_values(s, "s2r_set_master_multiband", n_bands, lp, hp, ap, curves, a_att, a_rel));
    s->post.set_multiband(n_bands, lp, hp, ap, curves, a_att, a_rel, false);
    return S2R_OK;
}

int s2r_set_master_multiband_params(s2r_synth *s, uint32_t n_bands, const float *lp, const float *hp, const float *ap, const float *curves,
                                    const float *a_att, const float *a_rel) {
    S2R_TRY(multiband_values(s, "s2r_set_master_multiband_params", n_bands, lp, hp, ap, curves, a_att, a_rel));
    S2R_TRY(multiband_set(s, "s2r_set_master_multiband_params"));
    if (n_bands != s->post.mb.n_bands)
        return set_err(s, S2R_ERR_INVALID, "s2r_set_master_multiband_params: %u bands where %u are set: s2r_set_master_multiband changes the count", n_bands, s->post.mb.n_bands);
    s->post.set_multiband(n_bands, lp, hp, ap, curves, a_att, a_rel, true);
    return S2R_OK;
}

int s2r_clear_master_multiband(s2r_synth *s) {
    S2R_TRY(post_handle(s, "s2r_clear_master_multiband", "the master multiband compressor is"));
    s->post.set_multiband(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false);
    return S2R_OK;
}

int s2r_get_master_multiband(const s2r_synth *s, uint32_t *n_bands, float *lp, float *hp, float *ap, float *curves, float *a_att, float *a_rel) {
    if (!s || !s->kids.empty() || s->parent) return S2R_ERR_INVALID;
    const S2rPostChain::Multiband &f = s->post.mb;
    const uint32_t B = f.n_bands;
    put(n_bands, B);
    if (B >= 2u) {
        if (lp) std::memcpy(lp, f.lp, (size_t)(B - 1u) * 5u * sizeof(float));
        if (hp) std::memcpy(hp, f.hp, (size_t)(B - 1u) * 5u * sizeof(float));
    }
    if (B >= 3u && ap) std::memcpy(ap, f.ap, (size_t)(B - 2u) * 5u * sizeof(float));
    if (B && curves) std::memcpy(curves, f.curves.data(), f.curves.size() * sizeof(float));
    if (B && a_att) std::memcpy(a_att, f.a_att, B * sizeof(float));
    if (B && a_rel) std::memcpy(a_rel, f.a_rel, B * sizeof(float));
    return S2R_OK;
}

int s2r_reset_master_multiband(s2r_synth *s) {
    S2R_TRY(multiband_set(s, "s2r_reset_master_multiband"));
    s->post.reset_multiband();
    return S2R_OK;
}

int s2r_get_multiband_state(s2r_synth *s, float *state, size_t capacity) {
    S2R_TRY(multiband_set(s, "s2r_get_multiband_state"));
    S2rPostChain::Multiband &f = s->post.mb;
    const size_t n = S2R_MULTIBAND_STATE(f.n_bands);
    if (capacity < n) return set_err(s, S2R_ERR_INVALID, "s2r_get_multiband_state: the state is %zu floats, not %zu", n, capacity);
    if (!state) return set_err(s, S2R_ERR_INVALID, "s2r_get_multiband_state: null buffer");
    S2R_TRY(mirror_fetch(s, f.state, "s2r_get_multiband_state"));
    std::memcpy(state, f.state.host.data(), n * sizeof(float));
    return S2R_OK;
}

int s2r_set_multiband_state(s2r_synth *s, const float *state, size_t count) {
    S2R_TRY(multiband_set(s, "s2r_set_multiband_state"));
    S2rPostChain::Multiband &f = s->post.mb;
    const size_t n = S2R_MULTIBAND_STATE(f.n_bands), n_filt = 4u * (size_t)S2R_MULTIBAND_SECTIONS(f.n_bands);
    if (count != n) return set_err(s, S2R_ERR_INVALID, "s2r_set_multiband_state: the state is %zu floats, not %zu", n, count);
    if (!state) return set_err(s, S2R_ERR_INVALID, "s2r_set_multiband_state: null buffer");
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(state[i]) || (i >= n_filt && !dyn_state_in_range(state[i])))
            return set_err(s, S2R_ERR_PATCH_RANGE, "s2r_set_multiband_state: float %zu is %g: every float finite, the gains not below 0", i, (double)state[i]);
    f.state.set(state, n);
    return S2R_OK;
}

int s2r_get_multiband_meters(const s2r_synth *s, float *min_gain, size_t capacity) {
    if (!s || !s->kids.empty() || s->parent || !s->post.mb.n_bands || !s->post.mb.metered || !min_gain || capacity < s->post.mb.n_bands) return S2R_ERR_INVALID;
    std::memcpy(min_gain, s->post.mb.min_gain, s->post.mb.n_bands * sizeof(float));
    return S2R_OK;
}

// ---- what the entries of the two meters behind the limiter share: their guard, their state pair and their rows pair ----
enum { kLoudness, kSpectrum };
static const struct { const char *are, *none, *rows; } kMeterWords[2] = {{"the loudness meter is", "no loudness meter is set", "hops"},
                                                                         {"the spectrum meter is", "no spectrum meter is set", "rows"}};
struct Meter { S2rMirror *state; S2rRowStore *kept; size_t floats; uint32_t *pos, hop; };        // a meter that is set, as far as the two are alike

// the guard of the entries that need the meter set
static int meter_on(const s2r_synth *s, int which, const char *who, Meter *m = nullptr) {
    S2R_TRY(post_handle(s, who, kMeterWords[which].are));
    S2rPostChain &p = const_cast<s2r_synth *>(s)->post;
    const Meter is = which == kLoudness ? Meter{&p.loud.state, &p.loud.kept, S2R_LOUDNESS_STATE, &p.loud.pos, p.loud.hop}
                                        : Meter{&p.spec.state, &p.spec.kept, S2R_SPECTRUM_STATE(p.spec.n_fft), &p.spec.pos, p.spec.hop};
    if (!is.hop) return set_err(const_cast<s2r_synth *>(s), S2R_ERR_INVALID, "%s: %s", who, kMeterWords[which].none);
    if (m) *m = is;
    return S2R_OK;
}

static int meter_get_state(s2r_synth *s, int which, float *state, size_t capacity, uint32_t *pos, const char *who) {
    Meter m;
    S2R_TRY(meter_on(s, which, who, &m));
    if (capacity < m.floats) return set_err(s, S2R_ERR_INVALID, "%s: the state is %zu floats, not %zu", who, m.floats, capacity);
    if (!state) return set_err(s, S2R_ERR_INVALID, "%s: null buffer", who);
    S2R_TRY(mirror_fetch(s, *m.state, who));
    std::memcpy(state, m.state->host.data(), m.floats * sizeof(float));
    put(pos, *m.pos);
    return S2R_OK;
}

static int meter_set_state(s2r_synth *s, int which, const float *state, size_t count, uint32_t pos, const char *who) {
    Meter m;
    S2R_TRY(meter_on(s, which, who, &m));
    if (count != m.floats) return set_err(s, S2R_ERR_INVALID, "%s: the state is %zu floats, not %zu", who, m.floats, count);
    if (!state) return set_err(s, S2R_ERR_INVALID, "%s: null buffer", who);
    if (pos >= m.hop) return set_err(s, S2R_ERR_PATCH_RANGE, "%s: position %u, below the hop of %u", who, pos, m.hop);
    m.state->set(state, m.floats);
    *m.pos = pos;
    return S2R_OK;
}

static int meter_get_rows(const s2r_synth *s, int which, float *rows, size_t capacity, size_t *n_rows, const char *who) {
    Meter m;
    S2R_TRY(meter_on(s, which, who, &m));
    const size_t n = m.kept->n_rows() * m.kept->width;
    if (capacity < n || (n && !rows))
        return set_err(const_cast<s2r_synth *>(s), S2R_ERR_INVALID, "%s: the rows are %zu floats, the buffer holds %zu", who, n, rows ? capacity : (size_t)0);
    if (n) std::memcpy(rows, m.kept->stored(), n * sizeof(float));
    put(n_rows, m.kept->n_rows());
    return S2R_OK;
}

static int meter_set_rows(s2r_synth *s, int which, const float *rows, size_t n_rows, size_t count, const char *who) {
    Meter m;
    S2R_TRY(meter_on(s, which, who, &m));
    const char *const word = kMeterWords[which].rows;
    if (n_rows > m.kept->max_rows) return set_err(s, S2R_ERR_PATCH_RANGE, "%s: %zu %s, at most the %u the meter keeps", who, n_rows, word, m.kept->max_rows);
    if (count != n_rows * m.kept->width || (count && !rows))
        return set_err(s, S2R_ERR_INVALID, "%s: %zu %s are %zu floats, not %zu", who, n_rows, word, n_rows * m.kept->width, rows ? count : (size_t)0);
    m.kept->assign(rows, n_rows);
    return S2R_OK;
}

// ---- the loudness and true-peak meters behind the limiter ----
int s2r_set_master_loudness(s2r_synth *s, const float coeffs[10], uint32_t hop, uint32_t max_hops) {
    if (!loudness_in_range(coeffs, hop, max_hops))
        return set_err(s, S2R_ERR_PATCH_RANGE, "master loudness: hop %u, %u hops: ten finite coefficients, the hop in %u .. %u, the hops kept in %u .. %u", hop, max_hops,
                       S2R_LOUDNESS_MIN_HOP, S2R_LOUDNESS_MAX_HOP, S2R_LOUDNESS_MIN_HOPS, S2R_LOUDNESS_MAX_HOPS);
    S2R_TRY(post_handle(s, "s2r_set_master_loudness", "the loudness meter is"));
    if (!coeffs) return set_err(s, S2R_ERR_INVALID, "s2r_set_master_loudness: no coefficients");
    s->post.set_loudness(coeffs, hop, max_hops);
    return S2R_OK;
}

int s2r_clear_master_loudness(s2r_synth *s) {
    S2R_TRY(post_handle(s, "s2r_clear_master_loudness", "the loudness meter is"));
    s->post.set_loudness(nullptr, 0, 0);
    return S2R_OK;
}

int s2r_get_master_loudness(const s2r_synth *s, float coeffs[10], uint32_t *hop, uint32_t *max_hops, size_t *n_hops) {
    if (!s || !s->kids.empty() || s->parent) return S2R_ERR_INVALID;
    const S2rPostChain::Loudness &ld = s->post.loud;
    if (coeffs) std::memcpy(coeffs, ld.c, sizeof ld.c);
    put(hop, ld.hop); put(max_hops, ld.kept.max_rows); put(n_hops, ld.kept.n_rows());
    return S2R_OK;
}

int s2r_reset_master_loudness(s2r_synth *s) {
    S2R_TRY(meter_on(s, kLoudness, "s2r_reset_master_loudness"));
    s->post.reset_loudness();
    return S2R_OK;
}

int s2r_get_loudness(const s2r_synth *s, uint32_t programme, double out[3]) {
    if (programme >= S2R_LOUDNESS_PROGRAMMES) return S2R_ERR_PATCH_RANGE;
    if (!s || !s->kids.empty() || s->parent || !s->post.loud.hop || !out) return S2R_ERR_INVALID;
    const S2rPostChain::Loudness &ld = s->post.loud;
    return s2r_loudness_readings(ld.kept.stored(), ld.kept.n_rows(), ld.hop, programme, out);
}

int s2r_get_true_peak(const s2r_synth *s, float last[2], float held[2]) {
    if (!s || !s->kids.empty() || s->parent || !s->post.loud.hop) return S2R_ERR_INVALID;
    const S2rPostChain::Loudness &ld = s->post.loud;
    if (last) { last[0] = ld.tp_last[0]; last[1] = ld.tp_last[1]; }
    if (held) { held[0] = ld.tp_held[0]; held[1] = ld.tp_held[1]; }
    return S2R_OK;
}

int s2r_get_loudness_state(s2r_synth *s, float *state, size_t capacity, uint32_t *pos) { return meter_get_state(s, kLoudness, state, capacity, pos, "s2r_get_loudness_state"); }
int s2r_set_loudness_state(s2r_synth *s, const float *state, size_t count, uint32_t pos) { return meter_set_state(s, kLoudness, state, count, pos, "s2r_set_loudness_state"); }
int s2r_get_loudness_hops(const s2r_synth *s, float *rows, size_t capacity, size_t *n_hops) { return meter_get_rows(s, kLoudness, rows, capacity, n_hops, "s2r_get_loudness_hops"); }
int s2r_set_loudness_hops(s2r_synth *s, const float *rows, size_t n_hops, size_t count) { return meter_set_rows(s, kLoudness, rows, n_hops, count, "s2r_set_loudness_hops"); }

// ---- the spectrum meters behind the loudness meters ----
int s2r_set_master_spectrum(s2r_synth *s, uint32_t n_fft, uint32_t hop, const float *window, uint32_t max_rows) {
    if (!spectrum_in_range(n_fft, hop, window, max_rows))
        return set_err(s, S2R_ERR_PATCH_RANGE, "master spectrum: size %u, hop %u, %u rows: a power of two in %u .. %u, the hop in max(%u, size / 8) .. %u, the rows kept in 1 .. %u, a finite window",
                       n_fft, hop, max_rows, S2R_SPECTRUM_MIN_FFT, S2R_SPECTRUM_MAX_FFT, S2R_SPECTRUM_MIN_HOP, S2R_SPECTRUM_MAX_HOP, S2R_SPECTRUM_MAX_ROWS);
    S2R_TRY(post_handle(s, "s2r_set_master_spectrum", "the spectrum meter is"));
    if (!window) return set_err(s, S2R_ERR_INVALID, "s2r_set_master_spectrum: no window");
    s->post.set_spectrum(n_fft, hop, window, max_rows);
    return S2R_OK;
}

int s2r_clear_master_spectrum(s2r_synth *s) {
    S2R_TRY(post_handle(s, "s2r_clear_master_spectrum", "the spectrum meter is"));
    s->post.set_spectrum(0, 0, nullptr, 0);
    return S2R_OK;
}

int s2r_get_master_spectrum(const s2r_synth *s, uint32_t *n_fft, uint32_t *hop, uint32_t *max_rows, size_t *n_rows, float *window, size_t window_capacity) {
    if (!s || !s->kids.empty() || s->parent) return S2R_ERR_INVALID;
    const S2rPostChain::Spectrum &sp = s->post.spec;
    if (window && window_capacity < sp.n_fft) return S2R_ERR_INVALID;
    if (window && sp.n_fft) std::memcpy(window, sp.window.data(), sp.n_fft * sizeof(float));
    put(n_fft, sp.n_fft); put(hop, sp.hop); put(max_rows, sp.kept.max_rows); put(n_rows, sp.kept.n_rows());
    return S2R_OK;
}

int s2r_reset_master_spectrum(s2r_synth *s) {
    S2R_TRY(meter_on(s, kSpectrum, "s2r_reset_master_spectrum"));
    s->post.reset_spectrum();
    return S2R_OK;
}

int s2r_get_spectrum(const s2r_synth *s, uint32_t programme, uint32_t n_avg, double *out_db, size_t capacity) {
    if (programme >= S2R_SPECTRUM_PROGRAMMES) return S2R_ERR_PATCH_RANGE;
    if (!s || !s->kids.empty() || s->parent || !s->post.spec.n_fft || !out_db) return S2R_ERR_INVALID;
    const S2rPostChain::Spectrum &sp = s->post.spec;
    if (n_avg == 0u || n_avg > sp.kept.n_rows()) return S2R_ERR_PATCH_RANGE;
    return s2r_spectrum_readings(sp.kept.stored(), sp.kept.n_rows(), sp.n_fft, sp.window.data(), programme, n_avg, out_db, capacity);
}

int s2r_get_spectrum_bands(const s2r_synth *s, uint32_t programme, uint32_t n_avg, double sample_rate, uint32_t bands_per_octave, double *out_db, double *centres,
                           size_t capacity, size_t *n_bands) {
    if (programme >= S2R_SPECTRUM_PROGRAMMES) return S2R_ERR_PATCH_RANGE;
    if (!s || !s->kids.empty() || s->parent || !s->post.spec.n_fft || !out_db || !n_bands) return S2R_ERR_INVALID;
    const S2rPostChain::Spectrum &sp = s->post.spec;
    if (n_avg == 0u || n_avg > sp.kept.n_rows()) return S2R_ERR_PATCH_RANGE;
    return s2r_spectrum_band_readings(sp.kept.stored(), sp.kept.n_rows(), sp.n_fft, sp.window.data(), programme, n_avg, sample_rate, bands_per_octave, out_db, centres, capacity,
                                      n_bands);
}

int s2r_get_spectrum_rows(const s2r_synth *s, float *rows, size_t capacity, size_t *n_rows) { return meter_get_rows(s, kSpectrum, rows, capacity, n_rows, "s2r_get_spectrum_rows"); }
int s2r_set_spectrum_rows(s2r_synth *s, const float *rows, size_t n_rows, size_t count) { return meter_set_rows(s, kSpectrum, rows, n_rows, count, "s2r_set_spectrum_rows"); }
int s2r_get_spectrum_state(s2r_synth *s, float *state, size_t capacity, uint32_t *pos) { return meter_get_state(s, kSpectrum, state, capacity, pos, "s2r_get_spectrum_state"); }
int s2r_set_spectrum_state(s2r_synth *s, const float *state, size_t count, uint32_t pos) { return meter_set_state(s, kSpectrum, state, count, pos, "s2r_set_spectrum_state"); }

// ---- the PCM stage behind the spectrum meters ----
// the guard of the entries that need the stage set
static int pcm_set(const s2r_synth *s, const char *who) {
    S2R_TRY(post_handle(s, who, "the PCM stage is"));
    if (!s->post.pcm.bits) return set_err(const_cast<s2r_synth *>(s), S2R_ERR_INVALID, "%s: no PCM stage is set", who);
    return S2R_OK;
}

int s2r_set_master_pcm(s2r_synth *s, uint32_t bits, uint32_t dither, const float *taps, uint32_t n_taps, uint32_t seed) {
    if (!pcm_in_range(bits, dither, taps, n_taps))
        return set_err(s, S2R_ERR_PATCH_RANGE, "master pcm: %u bits, dither %u, %u taps: the bits in %u .. %u, the dither one of 0, 1, 2, at most %u finite taps of at most %g", bits,
                       dither, n_taps, S2R_PCM_MIN_BITS, S2R_PCM_MAX_BITS, S2R_PCM_MAX_TAPS, (double)S2R_PCM_MAX_TAP);
    S2R_TRY(post_handle(s, "s2r_set_master_pcm", "the PCM stage is"));
    if (n_taps && !taps) return set_err(s, S2R_ERR_INVALID, "s2r_set_master_pcm: no taps");
    s->post.set_pcm(bits, dither, taps, n_taps, seed);
    return S2R_OK;
}

int s2r_clear_master_pcm(s2r_synth *s) {
    S2R_TRY(post_handle(s, "s2r_clear_master_pcm", "the PCM stage is"));
    s->post.set_pcm(0, 0, nullptr, 0, 0);
    return S2R_OK;
}

int s2r_get_master_pcm(const s2r_synth *s, uint32_t *bits, uint32_t *dither, float *taps, uint32_t *n_taps, uint32_t *seed) {
    if (!s || !s->kids.empty() || s->parent) return S2R_ERR_INVALID;
    const S2rPostChain::Pcm &pm = s->post.pcm;
    if (taps) std::memcpy(taps, pm.h, sizeof pm.h);
    put(bits, pm.bits); put(dither, pm.dither); put(n_taps, pm.n_taps); put(seed, pm.seed);
    return S2R_OK;
}

int s2r_reset_master_pcm(s2r_synth *s) {
    S2R_TRY(pcm_set(s, "s2r_reset_master_pcm"));
    s->post.reset_pcm();
    return S2R_OK;
}

int s2r_get_pcm(const s2r_synth *s, uint32_t programme, int32_t *pcm_lr, size_t capacity, size_t *frames) {
    if (programme >= S2R_PCM_PROGRAMMES) return S2R_ERR_PATCH_RANGE;
    if (!s || !s->kids.empty() || s->parent || !s->post.pcm.bits || !s->post.pcm.have || !pcm_lr) return S2R_ERR_INVALID;
    const S2rPostChain::Pcm &pm = s->post.pcm;
    if (capacity < 2u * (size_t)pm.frames) return S2R_ERR_INVALID;
    if (pm.frames) std::memcpy(pcm_lr, pm.samples.host + (size_t)programme * 2u * pm.cap(), 2u * (size_t)pm.frames * sizeof(int32_t));
    put(frames, (size_t)pm.frames);
    return S2R_OK;
}

int s2r_get_pcm_clips(const s2r_synth *s, uint32_t *last, uint32_t *held) {
    if (!s || !s->kids.empty() || s->parent || !s->post.pcm.bits) return S2R_ERR_INVALID;
    const S2rPostChain::Pcm &pm = s->post.pcm;
    if (last) std::memcpy(last, pm.clips_last, sizeof pm.clips_last);
    if (held) std::memcpy(held, pm.clips_held, sizeof pm.clips_held);
    return S2R_OK;
}

int s2r_get_pcm_state(s2r_synth *s, float *state, size_t capacity, uint32_t *t) {
    S2R_TRY(pcm_set(s, "s2r_get_pcm_state"));
    if (capacity < S2R_PCM_STATE) return set_err(s, S2R_ERR_INVALID, "s2r_get_pcm_state: the state is %u floats, not %zu", S2R_PCM_STATE, capacity);
    if (!state) return set_err(s, S2R_ERR_INVALID, "s2r_get_pcm_state: null buffer");
    S2rPostChain::Pcm &pm = s->post.pcm;
    S2R_TRY(mirror_fetch(s, pm.state, "s2r_get_pcm_state"));
    std::memcpy(state, pm.state.host.data(), S2R_PCM_STATE * sizeof(float));
    put(t, pm.t);
    return S2R_OK;
}

int s2r_set_pcm_state(s2r_synth *s, const float *state, size_t count, uint32_t t) {
    S2R_TRY(pcm_set(s, "s2r_set_pcm_state"));
    if (count != S2R_PCM_STATE) return set_err(s, S2R_ERR_INVALID, "s2r_set_pcm_state: the state is %u floats, not %zu", S2R_PCM_STATE, count);
    if (!state) return set_err(s, S2R_ERR_INVALID, "s2r_set_pcm_state: null buffer");
    if (!pcm_state_in_range(state)) return set_err(s, S2R_ERR_PATCH_RANGE, "s2r_set_pcm_state: an error outside [-2, 2]");
    s->post.set_pcm_state(state, t);
    return S2R_OK;
}

// ---- the sample-rate converter behind the spectrum meters and in front of the PCM stage ----
// the guard of the entries that need the stage set
static int resampler_set(const s2r_synth *s, const char *who) {
    S2R_TRY(post_handle(s, who, "the sample-rate converter is"));
    if (!s->post.res.L) return set_err(const_cast<s2r_synth *>(s), S2R_ERR_INVALID, "%s: no master resampler is set", who);
    return S2R_OK;
}

int s2r_set_master_resampler(s2r_synth *s, uint32_t L, uint32_t M, uint32_t T, const float *table) {
    if (!resampler_in_range(L, M, T, table))
        return set_err(s, S2R_ERR_PATCH_RANGE, "master resampler: %u / %u with %u taps a phase: coprime factors of 1 .. %u within 1/4 .. 4, taps a multiple of 4 in %u .. %u, at most %u finite entries of at most %g",
                       L, M, T, S2R_RESAMPLER_MAX_FACTOR, S2R_RESAMPLER_MIN_TAPS, S2R_RESAMPLER_MAX_TAPS, S2R_RESAMPLER_MAX_TABLE, (double)S2R_RESAMPLER_MAX_TAP);
    S2R_TRY(post_handle(s, "s2r_set_master_resampler", "the sample-rate converter is"));
    if (!table) return set_err(s, S2R_ERR_INVALID, "s2r_set_master_resampler: no table");
    s->post.set_resampler(L, M, T, table);
    return S2R_OK;
}

int s2r_clear_master_resampler(s2r_synth *s) {
    S2R_TRY(post_handle(s, "s2r_clear_master_resampler", "the sample-rate converter is"));
    s->post.set_resampler(0, 0, 0, nullptr);
    return S2R_OK;
}

int s2r_get_master_resampler(const s2r_synth *s, uint32_t *L, uint32_t *M, uint32_t *T, float *table) {
    if (!s || !s->kids.empty() || s->parent) return S2R_ERR_INVALID;
    const S2rPostChain::Resampler &rs = s->post.res;
    if (table && !rs.table.empty()) std::memcpy(table, rs.table.data(), rs.table.size() * sizeof(float));
    put(L, rs.L); put(M, rs.M); put(T, rs.T);
    return S2R_OK;
}

int s2r_reset_master_resampler(s2r_synth *s) {
    S2R_TRY(resampler_set(s, "s2r_reset_master_resampler"));
    s->post.reset_resampler();
    return S2R_OK;
}

int s2r_get_resampled(const s2r_synth *s, uint32_t programme, float *out_lr, size_t capacity, size_t *frames) {
    if (programme >= S2R_RESAMPLER_PROGRAMMES) return S2R_ERR_PATCH_RANGE;
    if (!s || !s->kids.empty() || s->parent || !s->post.res.L || !s->post.res.have || !out_lr) return S2R_ERR_INVALID;
    const S2rPostChain::Resampler &rs = s->post.res;
    if (capacity < 2u * (size_t)rs.count) return S2R_ERR_INVALID;
    if (rs.count) std::memcpy(out_lr, rs.res.host + (size_t)programme * 2u * rs.cap(), 2u * (size_t)rs.count * sizeof(float));
    put(frames, (size_t)rs.count);
    return S2R_OK;
}

int s2r_get_resampler_state(s2r_synth *s, float *state, size_t capacity, uint32_t *ph) {
    S2R_TRY(resampler_set(s, "s2r_get_resampler_state"));
    S2rPostChain::Resampler &rs = s->post.res;
    const size_t n = S2R_RESAMPLER_STATE(rs.T);
    if (capacity < n) return set_err(s, S2R_ERR_INVALID, "s2r_get_resampler_state: the state is %zu floats, not %zu", n, capacity);
    if (!state) return set_err(s, S2R_ERR_INVALID, "s2r_get_resampler_state: null buffer");
    S2R_TRY(mirror_fetch(s, rs.state, "s2r_get_resampler_state"));
    std::memcpy(state, rs.state.host.data(), n * sizeof(float));
    put(ph, rs.ph);
    return S2R_OK;
}

int s2r_set_resampler_state(s2r_synth *s, const float *state, size_t count, uint32_t ph) {
    S2R_TRY(resampler_set(s, "s2r_set_resampler_state"));
    const S2rPostChain::Resampler &rs = s->post.res;
    const size_t n = S2R_RESAMPLER_STATE(rs.T);
    if (count != n) return set_err(s, S2R_ERR_INVALID, "s2r_set_resampler_state: the state is %zu floats, not %zu", n, count);
    if (!state) return set_err(s, S2R_ERR_INVALID, "s2r_set_resampler_state: null buffer");
    if (ph >= rs.M) return set_err(s, S2R_ERR_PATCH_RANGE, "s2r_set_resampler_state: a position of %u at M = %u", ph, rs.M);
    s->post.set_resampler_state(state, ph);
    return S2R_OK;
}

// ---- measurement (tools/*_time.py load these by name; not declared in s2r.h) ----
// device time of one stage's kernels in the last bus or master fill, in milliseconds (s2r_set_timing on; < 0 otherwise)
#define POST_MS(timer) (s && s->timing ? s->post.timer.ms : -1.0f)
#define MASTER_MS(k) POST_MS(master_timer[k])
// of the buses' EQ kernel in that fill: 0 when it ran none (tools/eq_time.py); whether the handle holds the EQs' staging buffer;
// and the frames the kernel stages at a time (tests/test_gpu_eq.py picks its call lengths around it)
float s2r_debug_bus_eq_ms(const s2r_synth *s) { return POST_MS(stage[S2R_BUS_EQ].timer); }
int s2r_debug_bus_eq_allocated(const s2r_synth *s) { return s && s->post.stage[S2R_BUS_EQ].buffer ? 1 : 0; }
uint32_t s2r_debug_eq_tile(void) { return S2R_EQ_TILE; }
// ... of the buses' dynamics kernel in that fill: 0 when it ran none (tools/dyn_time.py); whether the handle holds the dynamics' staging
// buffer; and the frames of one stage of the kernel's pipeline (tests/test_gpu_dyn.py picks its call lengths around it)
float s2r_debug_dyn_ms(const s2r_synth *s) { return POST_MS(stage[S2R_BUS_DYN].timer); }
int s2r_debug_dyn_allocated(const s2r_synth *s) { return s && (s->post.stage[S2R_BUS_DYN].buffer || s->post.dyn_curves.dev || s->post.dyn_meter.host) ? 1 : 0; }
uint32_t s2r_debug_dyn_tile(void) { return S2R_DYN_TILE; }
// ... of the buses' room kernel in that fill: 0 when it ran none (tools/room_time.py); whether the handle holds the rooms' staging buffer;
// and the frames of one pass of the kernel (tests/test_gpu_room.py picks its call lengths around it)
float s2r_debug_bus_room_ms(const s2r_synth *s) { return POST_MS(stage[S2R_BUS_ROOM].timer); }
int s2r_debug_room_allocated(const s2r_synth *s) { return s && s->post.stage[S2R_BUS_ROOM].buffer ? 1 : 0; }
uint32_t s2r_debug_room_tile(void) { return S2R_ROOM_TILE; }
// ... of the buses' drive kernel in that fill: 0 when it ran none (tools/drive_time.py); whether the handle holds the drives' staging
// buffer or their tables; and the output frames of one workgroup of the kernel (tests/test_gpu_drive.py picks its call lengths around it)
float s2r_debug_bus_drive_ms(const s2r_synth *s) { return POST_MS(stage[S2R_BUS_DRIVE].timer); }
int s2r_debug_drive_allocated(const s2r_synth *s) { return s && (s->post.stage[S2R_BUS_DRIVE].buffer || s->post.drive_curves.dev) ? 1 : 0; }
uint32_t s2r_debug_drive_tile(void) { return S2R_DRIVE_TILE; }
// ... of the buses' flanger kernel in that fill: 0 when it ran none (tools/flanger_time.py); whether the handle holds the flangers'
// staging buffer; and the frames of one tile of the kernel (tests/test_gpu_flanger.py picks its call lengths around it)
float s2r_debug_bus_flanger_ms(const s2r_synth *s) { return POST_MS(stage[S2R_BUS_FLANGER].timer); }
int s2r_debug_flanger_allocated(const s2r_synth *s) { return s && s->post.stage[S2R_BUS_FLANGER].buffer ? 1 : 0; }
uint32_t s2r_debug_flanger_tile(void) { return S2R_FLANGER_TILE; }
// ... of the buses' chorus kernel in that fill: 0 when it ran none (tools/chorus_time.py)
float s2r_debug_bus_chorus_ms(const s2r_synth *s) { return POST_MS(stage[S2R_BUS_CHORUS].timer); }
// ... of the buses' delay kernel in that fill: 0 when it ran none (tools/delay_time.py)
float s2r_debug_bus_delay_ms(const s2r_synth *s) { return POST_MS(stage[S2R_BUS_DELAY].timer); }
// ... and of the buses' reverb kernels in that fill: 0 when it ran none (tools/reverb_time.py)
float s2r_debug_bus_fx_ms(const s2r_synth *s) { return POST_MS(stage[S2R_BUS_REVERB].timer); }
// ... and of the master kernel in the last s2r_fill_master (tools/master_time.py)
float s2r_debug_master_ms(const s2r_synth *s) { return MASTER_MS(S2R_MASTER_MIX); }
// ... and of the limiter kernel in that fill: 0 when it ran none (tools/limiter_time.py)
float s2r_debug_limiter_ms(const s2r_synth *s) { return MASTER_MS(S2R_MASTER_LIMITER); }
// ... and of the loudness kernel in that fill: 0 when it ran none (tools/loudness_time.py)
float s2r_debug_loudness_ms(const s2r_synth *s) { return MASTER_MS(S2R_MASTER_LOUDNESS); }
// ... and of the spectrum kernel in that fill: 0 when it ran none (tools/spectrum_time.py)
float s2r_debug_spectrum_ms(const s2r_synth *s) { return MASTER_MS(S2R_MASTER_SPECTRUM); }
// ... and of the PCM kernel in that fill: 0 when it ran none (tools/pcm_time.py); whether the handle holds anything of the stage's; and
// the frames the kernel stages at a time (tests/test_gpu_pcm.py picks its call lengths around it)
float s2r_debug_pcm_ms(const s2r_synth *s) { return MASTER_MS(S2R_MASTER_PCM); }
int s2r_debug_pcm_allocated(const s2r_synth *s) { return s && (s->post.pcm.samples.host || s->post.pcm.counts.host || s->post.pcm.state.dev[0] || s->post.loud.in.dev) ? 1 : 0; }
uint32_t s2r_debug_pcm_tile(void) { return S2R_PCM_TILE; }
// ... and of the resampler kernel in that fill: 0 when it ran none (tools/resampler_time.py); whether the handle holds anything of the
// stage's; and the output frames of one of the kernel's workgroups (tests/test_gpu_resampler.py picks its call lengths around it)
float s2r_debug_resampler_ms(const s2r_synth *s) { return MASTER_MS(S2R_MASTER_RESAMPLER); }
int s2r_debug_resampler_allocated(const s2r_synth *s) { return s && (s->post.res.res.host || s->post.res.res_dev.dev || s->post.res.table_dev.dev || s->post.res.state.dev[0] || s->post.loud.in.dev) ? 1 : 0; }
uint32_t s2r_debug_resampler_tile(void) { return S2R_RESAMPLER_TILE; }
// ... and of the multiband kernel in that fill: 0 when it ran none (tools/multiband_time.py); whether the handle holds anything of the
// stage's; and the frames of one stage of the kernel's pipeline (tests/test_gpu_multiband.py picks its call lengths around it)
float s2r_debug_multiband_ms(const s2r_synth *s) { return MASTER_MS(S2R_MASTER_MULTIBAND); }
int s2r_debug_multiband_allocated(const s2r_synth *s) { return s && (s->post.mb.in.dev || s->post.mb.curves_dev.dev || s->post.mb.meter.host || s->post.mb.state.dev[0]) ? 1 : 0; }
uint32_t s2r_debug_multiband_tile(void) { return S2R_MULTIBAND_TILE; }

}  // extern "C"
