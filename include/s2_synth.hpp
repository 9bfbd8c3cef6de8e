// s2_synth.hpp — header-only C++ mirror of `s2_lib::try3::synth` over the C ABI (s2r.h).
//
// Same names, argument meaning and call pattern as the reference
// (/root/reference/components/s2_lib/src/try3/synth.rs:9-21,53-80,154-156; units.rs:11-14), so a
// C++ caller — or a test — reads like the reference's own call sites
// (components/s2_bin/src/main.rs:132-147,198-205):
//
//     s2::Synth synth;                                   // Synth::new()
//     synth.note_on(s2::Note{69}, s2::Velocity{{1.0f}});
//     synth.sample(buffer, n, s2::SampleRateKhz{48000}); // overwrites buffer
//     synth.note_off(s2::Note{69});
//
// Where the reference panics (offset overflow, process.rs:36) this throws s2::Error.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include "s2r.h"

namespace s2 {

template <unsigned N> struct Unipolar { float v; };   // units.rs:11
struct Note { uint8_t v; };                           // synth.rs:16  Note(pub u8)
struct Velocity { Unipolar<1> v; };                   // synth.rs:18  Velocity(pub Unipolar<1>)
struct SampleRateKhz { uint32_t v; };                 // units.rs:14  (holds Hz, units.rs:21)

struct Error : std::runtime_error {
    int status;
    Error(int st, const std::string &msg) : std::runtime_error(msg), status(st) {}
};

class Synth {
  public:
    // Synth::new(): NUM_VOICES = 8 in the reference (synth.rs:7); here a run-time size.
    explicit Synth(uint32_t num_voices = 8, uint32_t max_frames = 2048, int device = -1) {
        s2r_config cfg{};
        cfg.struct_size = sizeof cfg;
        cfg.total_voices = num_voices;
        cfg.max_frames = max_frames;
        cfg.device = device;
        const int rc = s2r_create(&cfg, &h_);
        if (rc != S2R_OK) throw Error(rc, s2r_status_string(rc));
    }
    explicit Synth(const s2r_config &cfg) {
        const int rc = s2r_create(&cfg, &h_);
        if (rc != S2R_OK) throw Error(rc, s2r_status_string(rc));
    }
    // ONE Synth over several GPUs (s2r_config.devices): the pool cut into one shard per device, the allocation policy
    // run once per event, the shards' partial mixes added in shard order on devices[0]
    static Synth with_devices(uint32_t num_voices, const int *devices, uint32_t n_devices, uint32_t max_frames = 2048,
                              uint32_t shard_interleave = 64) {
        s2r_config cfg{};
        cfg.struct_size = sizeof cfg;
        cfg.total_voices = num_voices;
        cfg.max_frames = max_frames;
        cfg.device = -1;
        cfg.shard_interleave = shard_interleave;
        cfg.n_devices = n_devices;
        for (uint32_t k = 0; k < n_devices && k < S2R_MAX_DEVICES; ++k) cfg.devices[k] = devices[k];
        return Synth(cfg);
    }
    ~Synth() { s2r_destroy(h_); }
    Synth(const Synth &) = delete;
    Synth &operator=(const Synth &) = delete;
    Synth(Synth &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }

    void load_patch(const std::string &synth2_text) { check(s2r_load_patch(h_, synth2_text.data(), synth2_text.size())); }
    // multi-timbral extension: a bank of patches, the current program picks the one a note_on uses
    void set_patch_bank(const s2r_patch *patches, uint32_t n) { check(s2r_set_patch_bank(h_, patches, n)); }
    void program_change(uint32_t program) { check(s2r_program_change(h_, program)); }
    void note_on(Note note, Velocity velocity) { check(s2r_note_on(h_, note.v, velocity.v.v)); }     // synth.rs:61-70
    void note_off(Note note) { check(s2r_note_off(h_, note.v)); }                                    // synth.rs:72-80
    // Synth::sample(&mut [f32], SampleRateKhz), synth.rs:154-169
    void sample(float *buffer, size_t len, SampleRateKhz sample_rate) { check(s2r_fill(h_, buffer, len, sample_rate.v)); }
    // the same in two halves for a caller with two buffers in flight (s2_bin: audio_player.rs:56-60, main.rs:135-149)
    void sample_begin(size_t len, SampleRateKhz sample_rate) { check(s2r_fill_begin(h_, len, sample_rate.v)); }
    void sample_end(float *buffer, size_t capacity) { check(s2r_fill_end(h_, buffer, capacity)); }
    // sample() per 16 frames from the audio callback (main.rs:138-147) without a launch per call: a resident render kernel
    // between calls, small pools only (s2r.h: s2r_set_low_latency); same samples either way
    void set_low_latency(bool enabled) { check(s2r_set_low_latency(h_, enabled ? 1 : 0)); }
    // a batch of events, each at frame 0 or at its 16-frame boundary inside the next buffer (main.rs:138-143)
    void note_events(const s2r_note_event *events, size_t n) { check(s2r_note_events(h_, events, n)); }

    // true stereo (build-defined; s2r.h: s2r_fill_panned): a pan and a key spread per bank program, given to a voice at its
    // note_on; `buffer` takes 2 * len floats, interleaved L, R
    void set_program_pan(uint32_t program, float pan, float key_spread = 0.0f) { check(s2r_set_program_pan(h_, program, pan, key_spread)); }
    void get_program_pan(uint32_t program, float *pan, float *key_spread) const { check(s2r_get_program_pan(h_, program, pan, key_spread)); }
    void voice_pans(float *pans) { check(s2r_get_voice_pans(h_, pans)); }                     // shard_voices entries, local order
    void set_voice_pans(const float *pans) { check(s2r_set_voice_pans(h_, pans)); }
    void sample_panned(float *buffer, size_t len, SampleRateKhz sample_rate) { check(s2r_fill_panned(h_, buffer, len, sample_rate.v)); }
    // host only: the pan a note_on gives its voice, and a pan's constant-power gains
    static float voice_pan(float pan, float key_spread, Note note) { return s2r_voice_pan(pan, key_spread, note.v); }
    static void pan_gains(float p, float *gl, float *gr) { s2r_pan_gains(p, gl, gr); }

    // the voice mixer (build-defined; s2r.h: s2r_fill_buses): level, velocity sensitivity and output bus per bank program, given
    // to a voice at its note_on; `buffer` takes 2 * len * n_buses floats, bus-major, L, R interleaved inside a bus
    void set_program_mix(uint32_t program, float level, float velocity_sens = 0.0f, uint32_t bus = 0) { check(s2r_set_program_mix(h_, program, level, velocity_sens, bus)); }
    void get_program_mix(uint32_t program, float *level, float *velocity_sens, uint32_t *bus) const { check(s2r_get_program_mix(h_, program, level, velocity_sens, bus)); }
    void voice_mix(float *gains, uint8_t *buses) { check(s2r_get_voice_mix(h_, gains, buses)); }    // shard_voices entries each, local order
    void set_voice_mix(const float *gains, const uint8_t *buses) { check(s2r_set_voice_mix(h_, gains, buses)); }
    void sample_buses(float *buffer, size_t capacity, uint32_t n_buses, size_t len, SampleRateKhz sample_rate) {
        check(s2r_fill_buses(h_, buffer, capacity, n_buses, len, sample_rate.v));
    }
    // host only: the gain a note_on of `velocity` gives its voice
    static float voice_gain(float level, float velocity_sens, float velocity) { return s2r_voice_gain(level, velocity_sens, velocity); }

    // live program faders (build-defined; s2r.h: s2r_set_program_fader): a fader and a pan shift per bank program that act on
    // every voice sounding on it and reach their target as a ramp across the next sample_buses call
    void set_program_fader(uint32_t program, float fader, float pan_shift = 0.0f) { check(s2r_set_program_fader(h_, program, fader, pan_shift)); }
    void get_program_fader(uint32_t program, float *fader, float *pan_shift, float *applied_fader = nullptr, float *applied_pan_shift = nullptr) const {
        check(s2r_get_program_fader(h_, program, fader, pan_shift, applied_fader, applied_pan_shift));
    }
    void snap_program_faders() { check(s2r_snap_program_faders(h_)); }
    // host only: the two gains of a voice with pan `pan` and gain `w` under a fader pair
    static void fader_gains(float pan, float w, float fader, float pan_shift, float *gl, float *gr) { s2r_fader_gains(pan, w, fader, pan_shift, gl, gr); }

    // aux sends (build-defined; s2r.h: s2r_set_program_send): a send in [0, 1] and the bus it feeds per bank program, given to a
    // voice at its note_on — a second feed of gain * send, post-pan and post-fader, in sample_buses only
    void set_program_send(uint32_t program, float send, uint32_t send_bus = 0) { check(s2r_set_program_send(h_, program, send, send_bus)); }
    void get_program_send(uint32_t program, float *send, uint32_t *send_bus) const { check(s2r_get_program_send(h_, program, send, send_bus)); }
    void voice_sends(float *sends, uint8_t *send_buses) { check(s2r_get_voice_sends(h_, sends, send_buses)); }    // shard_voices entries each, local order
    void set_voice_sends(const float *sends, const uint8_t *send_buses) { check(s2r_set_voice_sends(h_, sends, send_buses)); }
    static float send_gain(float g, float send) { return s2r_send_gain(g, send); }

    // per-bus convolution reverb (build-defined; s2r.h: s2r_set_bus_reverb): n_taps taps per channel (ir_r nullptr: ir_l for both), a
    // dry and a wet in [0, 1] and a history of n_taps - 1 stereo frames that carries from call to call — in sample_buses only
    void set_bus_reverb(uint32_t bus, const float *ir_l, const float *ir_r, uint32_t n_taps, float dry = 0.0f, float wet = 1.0f) {
        check(s2r_set_bus_reverb(h_, bus, ir_l, ir_r, n_taps, dry, wet));
    }
    void clear_bus_reverb(uint32_t bus) { check(s2r_set_bus_reverb(h_, bus, nullptr, nullptr, 0, 0.0f, 0.0f)); }
    void set_bus_reverb_mix(uint32_t bus, float dry, float wet) { check(s2r_set_bus_reverb_mix(h_, bus, dry, wet)); }
    void get_bus_reverb(uint32_t bus, uint32_t *n_taps, float *dry, float *wet) const { check(s2r_get_bus_reverb(h_, bus, n_taps, dry, wet)); }
    void bus_reverb_history(uint32_t bus, float *lr, size_t capacity) { check(s2r_get_bus_reverb_history(h_, bus, lr, capacity)); }     // 2 * (n_taps - 1) floats, oldest first, L R
    void set_bus_reverb_history(uint32_t bus, const float *lr, size_t count) { check(s2r_set_bus_reverb_history(h_, bus, lr, count)); }
    static int reverb_reference(const float *ir, uint32_t n_taps, const float *x_with_history, uint32_t frames, float dry, float wet, float *out) {
        return s2r_reverb_reference(ir, n_taps, x_with_history, frames, dry, wet, out);
    }
    // per-bus feedback delay in front of the bus's reverb (build-defined; s2r.h: s2r_set_bus_delay): delay_frames in 1 ..
    // S2R_MAX_DELAY_FRAMES, feedback and cross in [-1, 1] with |feedback| + |cross| <= 1, dry and wet in [0, 1]; in sample_buses and
    // sample_master only
    void set_bus_delay(uint32_t bus, uint32_t delay_frames, float feedback = 0.0f, float cross = 0.0f, float dry = 1.0f, float wet = 1.0f) {
        check(s2r_set_bus_delay(h_, bus, delay_frames, feedback, cross, dry, wet));
    }
    void clear_bus_delay(uint32_t bus) { check(s2r_set_bus_delay(h_, bus, 0, 0.0f, 0.0f, 0.0f, 0.0f)); }
    void set_bus_delay_mix(uint32_t bus, float feedback, float cross, float dry, float wet) { check(s2r_set_bus_delay_mix(h_, bus, feedback, cross, dry, wet)); }
    void get_bus_delay(uint32_t bus, uint32_t *delay_frames, float *feedback, float *cross, float *dry, float *wet) const {
        check(s2r_get_bus_delay(h_, bus, delay_frames, feedback, cross, dry, wet));
    }
    void bus_delay_history(uint32_t bus, float *lr, size_t capacity) { check(s2r_get_bus_delay_history(h_, bus, lr, capacity)); }     // 2 * delay_frames floats, oldest first, L R
    void set_bus_delay_history(uint32_t bus, const float *lr, size_t count) { check(s2r_set_bus_delay_history(h_, bus, lr, count)); }
    static int delay_reference(uint32_t delay_frames, float feedback, float cross, float dry, float wet, const float *x_lr, uint32_t frames, float *history_lr,
                               float *out_lr) {
        return s2r_delay_reference(delay_frames, feedback, cross, dry, wet, x_lr, frames, history_lr, out_lr);
    }
    // per-bus chorus in front of the bus's delay (build-defined; s2r.h: s2r_set_bus_chorus): voices in 1 .. S2R_CHORUS_MAX_VOICES, base >= 1 and
    // depth >= 0 frames with float(base + depth) <= S2R_CHORUS_MAX_DELAY, phase_inc (chorus_rate) and spread in 2^-32 turns, dry and wet in
    // [0, 1] (1 / voices goes into wet); in sample_buses and sample_master only
    void set_bus_chorus(uint32_t bus, uint32_t voices, float base, float depth, uint32_t phase_inc, uint32_t spread = 0, float dry = 1.0f, float wet = 1.0f) {
        check(s2r_set_bus_chorus(h_, bus, voices, base, depth, phase_inc, spread, dry, wet));
    }
    void clear_bus_chorus(uint32_t bus) { check(s2r_set_bus_chorus(h_, bus, 0, 0.0f, 0.0f, 0, 0, 0.0f, 0.0f)); }
    void set_bus_chorus_mix(uint32_t bus, float dry, float wet) { check(s2r_set_bus_chorus_mix(h_, bus, dry, wet)); }
    void set_bus_chorus_rate(uint32_t bus, uint32_t phase_inc, uint32_t spread) { check(s2r_set_bus_chorus_rate(h_, bus, phase_inc, spread)); }     // phase and history stay
    void get_bus_chorus(uint32_t bus, uint32_t *voices, float *base, float *depth, uint32_t *phase_inc, uint32_t *spread, float *dry, float *wet) const {
        check(s2r_get_bus_chorus(h_, bus, voices, base, depth, phase_inc, spread, dry, wet));
    }
    // 2 * chorus_history_frames(base, depth) floats, oldest first, L R, and the LFO's phase
    void bus_chorus_state(uint32_t bus, float *lr, size_t capacity, uint32_t *phase) { check(s2r_get_bus_chorus_state(h_, bus, lr, capacity, phase)); }
    void set_bus_chorus_state(uint32_t bus, const float *lr, size_t count, uint32_t phase) { check(s2r_set_bus_chorus_state(h_, bus, lr, count, phase)); }
    static uint32_t chorus_history_frames(float base, float depth) { return s2r_chorus_history_frames(base, depth); }
    static uint32_t chorus_rate(double hz, double sample_rate) { return (uint32_t)(uint64_t)(hz * 4294967296.0 / sample_rate + 0.5); }
    static int chorus_reference(uint32_t voices, float base, float depth, uint32_t phase_inc, uint32_t spread, float dry, float wet, const float *x_lr,
                                uint32_t frames, float *history_lr, uint32_t *phase, float *out_lr) {
        return s2r_chorus_reference(voices, base, depth, phase_inc, spread, dry, wet, x_lr, frames, history_lr, phase, out_lr);
    }
    // per-bus parametric EQ at the head of the chain, in front of the bus's chorus (build-defined; s2r.h: s2r_set_bus_eq): n_bands in
    // 1 .. S2R_EQ_MAX_BANDS biquads, coeffs [n_bands][5] as (b0, b1, b2, a1, a2) normalised by a0 (eq_design makes a band), finite, |a2| < 1
    // and |a1| < 1 + a2; in sample_buses and sample_master only
    void set_bus_eq(uint32_t bus, uint32_t n_bands, const float *coeffs) { check(s2r_set_bus_eq(h_, bus, n_bands, coeffs)); }
    void clear_bus_eq(uint32_t bus) { check(s2r_set_bus_eq(h_, bus, 0, nullptr)); }
    void set_bus_eq_coeffs(uint32_t bus, uint32_t n_bands, const float *coeffs) { check(s2r_set_bus_eq_coeffs(h_, bus, n_bands, coeffs)); }    // the state stays
    void get_bus_eq(uint32_t bus, uint32_t *n_bands, float *coeffs, size_t capacity) const { check(s2r_get_bus_eq(h_, bus, n_bands, coeffs, capacity)); }
    // 4 * n_bands floats: [band][s1_L, s1_R, s2_L, s2_R]
    void bus_eq_state(uint32_t bus, float *state, size_t capacity) { check(s2r_get_bus_eq_state(h_, bus, state, capacity)); }
    void set_bus_eq_state(uint32_t bus, const float *state, size_t count) { check(s2r_set_bus_eq_state(h_, bus, state, count)); }
    static int eq_reference(uint32_t n_bands, const float *coeffs, const float *x_lr, uint32_t frames, float *state, float *out_lr) {
        return s2r_eq_reference(n_bands, coeffs, x_lr, frames, state, out_lr);
    }
    static int eq_design(int kind, double freq_hz, double gain_db, double q, double sample_rate, float coeffs[5]) {
        return s2r_eq_design(kind, freq_hz, gain_db, q, sample_rate, coeffs);
    }
    // per-bus dynamics behind the bus's EQ (build-defined; s2r.h: s2r_set_bus_dynamics): a sidechain compressor keyed by key_bus (the bus
    // itself: a compressor; another: a ducker), curve [S2R_DYN_CURVE_POINTS] gains in [0, 256] (dynamics_curve makes one), a_att and
    // a_rel in [0, 1) (dynamics_coef); in sample_buses and sample_master only
    void set_bus_dynamics(uint32_t bus, uint32_t key_bus, const float *curve, float a_att, float a_rel) { check(s2r_set_bus_dynamics(h_, bus, key_bus, curve, a_att, a_rel)); }
    void clear_bus_dynamics(uint32_t bus) { check(s2r_clear_bus_dynamics(h_, bus)); }
    void set_bus_dynamics_params(uint32_t bus, uint32_t key_bus, const float *curve, float a_att, float a_rel) { check(s2r_set_bus_dynamics_params(h_, bus, key_bus, curve, a_att, a_rel)); }   // the gain stays
    bool get_bus_dynamics(uint32_t bus, uint32_t *key_bus, float *curve, size_t capacity, float *a_att, float *a_rel) const {
        uint32_t present = 0;
        check(s2r_get_bus_dynamics(h_, bus, &present, key_bus, curve, capacity, a_att, a_rel));
        return present != 0;
    }
    float bus_dynamics_state(uint32_t bus) { float y = 0.0f; check(s2r_get_bus_dynamics_state(h_, bus, &y, 1)); return y; }
    void set_bus_dynamics_state(uint32_t bus, float y) { check(s2r_set_bus_dynamics_state(h_, bus, &y, 1)); }
    float bus_dynamics_meter(uint32_t bus) const { float m = 1.0f; check(s2r_get_bus_dynamics_meter(h_, bus, &m)); return m; }
    static int dynamics_reference(const float *curve, float a_att, float a_rel, const float *key_lr, const float *x_lr, uint32_t frames, float *y, float *out_lr,
                                  float *min_gain) {
        return s2r_dynamics_reference(curve, a_att, a_rel, key_lr, x_lr, frames, y, out_lr, min_gain);
    }
    static int dynamics_curve(double threshold_db, double ratio, double knee_db, double makeup_db, float *curve) {
        return s2r_dynamics_curve(threshold_db, ratio, knee_db, makeup_db, curve);
    }
    static float dynamics_coef(double ms, double sample_rate) { return s2r_dynamics_coef(ms, sample_rate); }
    // per-bus room reverb, the last stem writer (build-defined; s2r.h: s2r_set_bus_room): eight damped feedback combs cd[S2R_ROOM_COMBS]
    // and four allpasses ad[S2R_ROOM_ALLPASSES] per channel, delays in frames, the right channel's `spread` longer (room_design makes a
    // set); feedback in [0, 1), damp in [0, 1], g in (-1, 1), gain, dry, wet and cross in [0, 1]; in sample_buses and sample_master only
    void set_bus_room(uint32_t bus, const uint32_t *cd, const uint32_t *ad, uint32_t spread, float feedback, float damp, float g, float gain, float dry, float wet,
                      float cross) {
        check(s2r_set_bus_room(h_, bus, cd, ad, spread, feedback, damp, g, gain, dry, wet, cross));
    }
    void clear_bus_room(uint32_t bus) { check(s2r_clear_bus_room(h_, bus)); }
    void set_bus_room_params(uint32_t bus, float feedback, float damp, float g, float gain, float dry, float wet, float cross) {   // delays and state stay
        check(s2r_set_bus_room_params(h_, bus, feedback, damp, g, gain, dry, wet, cross));
    }
    bool get_bus_room(uint32_t bus, uint32_t *cd, uint32_t *ad, uint32_t *spread, float *levels) const {
        uint32_t present = 0;
        check(s2r_get_bus_room(h_, bus, &present, cd, ad, spread, levels));
        return present != 0;
    }
    void bus_room_state(uint32_t bus, float *state, size_t capacity) { check(s2r_get_bus_room_state(h_, bus, state, capacity)); }
    void set_bus_room_state(uint32_t bus, const float *state, size_t count) { check(s2r_set_bus_room_state(h_, bus, state, count)); }
    static size_t room_state_floats(const uint32_t *cd, const uint32_t *ad, uint32_t spread) { return s2r_room_state_floats(cd, ad, spread); }
    static int room_reference(const uint32_t *cd, const uint32_t *ad, uint32_t spread, float feedback, float damp, float g, float gain, float dry, float wet,
                              float cross, const float *x_lr, uint32_t frames, float *state, float *out_lr) {
        return s2r_room_reference(cd, ad, spread, feedback, damp, g, gain, dry, wet, cross, x_lr, frames, state, out_lr);
    }
    static int room_design(double sample_rate, double size, uint32_t *cd, uint32_t *ad, uint32_t *spread) { return s2r_room_design(sample_rate, size, cd, ad, spread); }
    // per-bus drive behind the dynamics (build-defined; s2r.h: s2r_set_bus_drive): a waveshaper at four times the bus rate — a table
    // curve[S2R_DRIVE_CURVE_POINTS], finite, entry 512 its value at 0 (drive_curve makes one), pre in [0, S2R_DRIVE_MAX_PRE], dry and wet
    // in [0, 1]; the bus comes out S2R_DRIVE_LATENCY frames late; in sample_buses and sample_master only
    void set_bus_drive(uint32_t bus, const float *curve, float pre, float dry, float wet) { check(s2r_set_bus_drive(h_, bus, curve, pre, dry, wet)); }
    void clear_bus_drive(uint32_t bus) { check(s2r_clear_bus_drive(h_, bus)); }
    void set_bus_drive_params(uint32_t bus, const float *curve_or_null, float pre, float dry, float wet) {   // the history stays
        check(s2r_set_bus_drive_params(h_, bus, curve_or_null, pre, dry, wet));
    }
    bool get_bus_drive(uint32_t bus, float *curve, size_t capacity, float *pre, float *dry, float *wet) const {
        uint32_t present = 0;
        check(s2r_get_bus_drive(h_, bus, &present, curve, capacity, pre, dry, wet));
        return present != 0;
    }
    void bus_drive_history(uint32_t bus, float *lr, size_t capacity) { check(s2r_get_bus_drive_history(h_, bus, lr, capacity)); }
    void set_bus_drive_history(uint32_t bus, const float *lr, size_t count) { check(s2r_set_bus_drive_history(h_, bus, lr, count)); }
    static int drive_reference(const float *curve, float pre, float dry, float wet, const float *x_lr, uint32_t frames, float *history, float *out_lr) {
        return s2r_drive_reference(curve, pre, dry, wet, x_lr, frames, history, out_lr);
    }
    static int drive_curve(uint32_t kind, double amount, float *table) { return s2r_drive_curve(kind, amount, table); }
    static int drive_taps(float *h) { return s2r_drive_taps(h); }

    // per-bus flanger behind the drive (build-defined; s2r.h: s2r_set_bus_flanger): one tap base + depth * triangle frames late into the
    // stage's own line signal, fed back — base >= S2R_FLANGER_MIN_DELAY, depth >= 0, fl(base + depth) <= S2R_FLANGER_MAX_DELAY; phase_inc
    // and spread in 2^-32 turns; feedback and cross in [-1, 1] with |feedback| + |cross| <= 1; dry and wet in [0, 1]; in sample_buses and
    // sample_master only
    void set_bus_flanger(uint32_t bus, float base, float depth, uint32_t phase_inc, uint32_t spread, float feedback, float cross, float dry, float wet) {
        check(s2r_set_bus_flanger(h_, bus, base, depth, phase_inc, spread, feedback, cross, dry, wet));
    }
    void clear_bus_flanger(uint32_t bus) { check(s2r_clear_bus_flanger(h_, bus)); }
    void set_bus_flanger_params(uint32_t bus, uint32_t phase_inc, uint32_t spread, float feedback, float cross, float dry, float wet) {   // line and phase stay
        check(s2r_set_bus_flanger_params(h_, bus, phase_inc, spread, feedback, cross, dry, wet));
    }
    bool get_bus_flanger(uint32_t bus, float *base, float *depth, uint32_t *phase_inc, uint32_t *spread, float *feedback, float *cross, float *dry, float *wet) const {
        float b = 0.0f;
        check(s2r_get_bus_flanger(h_, bus, &b, depth, phase_inc, spread, feedback, cross, dry, wet));
        if (base) *base = b;
        return b != 0.0f;
    }
    void bus_flanger_state(uint32_t bus, float *lr, size_t capacity, uint32_t *phase) { check(s2r_get_bus_flanger_state(h_, bus, lr, capacity, phase)); }
    void set_bus_flanger_state(uint32_t bus, const float *lr, size_t count, uint32_t phase) { check(s2r_set_bus_flanger_state(h_, bus, lr, count, phase)); }
    static uint32_t flanger_history_frames(float base, float depth) { return s2r_flanger_history_frames(base, depth); }
    static int flanger_reference(float base, float depth, uint32_t phase_inc, uint32_t spread, float feedback, float cross, float dry, float wet, const float *x_lr,
                                 uint32_t frames, float *history_lr, uint32_t *phase, float *out_lr) {
        return s2r_flanger_reference(base, depth, phase_inc, spread, feedback, cross, dry, wet, x_lr, frames, history_lr, phase, out_lr);
    }
    static constexpr float FLANGER_MIN_DELAY = S2R_FLANGER_MIN_DELAY, FLANGER_MAX_DELAY = S2R_FLANGER_MAX_DELAY;

    // the master section (build-defined; s2r.h: s2r_fill_master): a return level per bus and a master fader, each in [0, 1] and each
    // reaching its target as a ramp across the next sample_master call, and the meters of that call — in sample_master only
    void set_bus_return(uint32_t bus, float level) { check(s2r_set_bus_return(h_, bus, level)); }
    void get_bus_return(uint32_t bus, float *level, float *applied = nullptr) const { check(s2r_get_bus_return(h_, bus, level, applied)); }
    void set_master_fader(float level) { check(s2r_set_master_fader(h_, level)); }
    void get_master_fader(float *level, float *applied = nullptr) const { check(s2r_get_master_fader(h_, level, applied)); }
    void snap_master() { check(s2r_snap_master(h_)); }
    // master_lr: 2 * len floats; stems: nullptr (master only) or what sample_buses writes, stems_capacity floats
    void sample_master(float *master_lr, float *stems, size_t stems_capacity, uint32_t n_buses, size_t len, SampleRateKhz sample_rate) {
        check(s2r_fill_master(h_, master_lr, stems, stems_capacity, n_buses, len, sample_rate.v));
    }
    // (n_buses + 1) * 2 entries per array: bus-major, L then R, the master last; capacity: entries per array
    void meters(uint32_t *n_buses, float *peak, float *energy, size_t capacity) const { check(s2r_get_meters(h_, n_buses, peak, energy, capacity)); }
    static int master_reference(const float *stems, uint32_t n_buses, uint32_t frames, const float *r0, const float *r1, float m0, float m1,
                                float *master_lr, float *peak, float *energy) {
        return s2r_master_reference(stems, n_buses, frames, r0, r1, m0, m1, master_lr, peak, energy);
    }

    // the master limiter (build-defined; s2r.h: s2r_set_master_limiter): a look-ahead limiter behind the master fader, in sample_master
    // only — no sample of master_lr exceeds `ceiling`, and master_lr is delayed by `lookahead` frames (the stems are not)
    void set_master_limiter(float ceiling, uint32_t lookahead, uint32_t hold = 0) { check(s2r_set_master_limiter(h_, ceiling, lookahead, hold)); }
    // ... with the true-peak detector (s2r.h: s2r_set_master_limiter_ex): the gain follows the 4x-interpolated magnitude, master_lr is
    // delayed by lookahead + S2R_LIMITER_TP_LATENCY frames, and xh below is 2 * (lookahead + S2R_LIMITER_TP_HISTORY) floats
    void set_master_limiter_true_peak(float ceiling, uint32_t lookahead, uint32_t hold = 0) {
        check(s2r_set_master_limiter_ex(h_, ceiling, lookahead, hold, S2R_LIMITER_TRUE_PEAK));
    }
    uint32_t get_master_limiter_detector() const { uint32_t d = 0; check(s2r_get_master_limiter_detector(h_, &d)); return d; }
    void clear_master_limiter() { check(s2r_clear_master_limiter(h_)); }
    // a lookahead of 0 means off
    void get_master_limiter(float *ceiling, uint32_t *lookahead, uint32_t *hold) const { check(s2r_get_master_limiter(h_, ceiling, lookahead, hold)); }
    // xh: 2 * lookahead floats; gh: 2 * lookahead + hold floats (checkpoints)
    void limiter_state(float *xh, size_t n_x, float *gh, size_t n_g) { check(s2r_get_limiter_state(h_, xh, n_x, gh, n_g)); }
    void set_limiter_state(const float *xh, size_t n_x, const float *gh, size_t n_g) { check(s2r_set_limiter_state(h_, xh, n_x, gh, n_g)); }
    void limiter_meters(float *min_gain, float *out_peak) const { check(s2r_get_limiter_meters(h_, min_gain, out_peak)); }
    static int limiter_reference(const float *x, uint32_t frames, float ceiling, uint32_t lookahead, uint32_t hold, float *xh, float *gh,
                                 float *y, float *gain) {
        return s2r_limiter_reference(x, frames, ceiling, lookahead, hold, xh, gh, y, gain);
    }

    // the master multiband compressor (build-defined; s2r.h: s2r_set_master_multiband): the master split into n_bands (1 .. 4) bands between
    // the master fader and the limiter, each compressed by its own curve, and added back, in sample_master only.  lp, hp: [n_bands - 1][5];
    // ap: [n_bands - 2][5]; curves: [n_bands][S2R_DYN_CURVE_POINTS]; a_att, a_rel: [n_bands]; an array of no rows may be null
    void set_master_multiband(uint32_t n_bands, const float *lp, const float *hp, const float *ap, const float *curves, const float *a_att, const float *a_rel) {
        check(s2r_set_master_multiband(h_, n_bands, lp, hp, ap, curves, a_att, a_rel));
    }
    // ... the parameters alone, with the band count that is set: the state stays
    void set_master_multiband_params(uint32_t n_bands, const float *lp, const float *hp, const float *ap, const float *curves, const float *a_att,
                                     const float *a_rel) {
        check(s2r_set_master_multiband_params(h_, n_bands, lp, hp, ap, curves, a_att, a_rel));
    }
    void clear_master_multiband() { check(s2r_clear_master_multiband(h_)); }
    // *n_bands is 0 when off; every array may be null
    void get_master_multiband(uint32_t *n_bands, float *lp, float *hp, float *ap, float *curves, float *a_att, float *a_rel) const {
        check(s2r_get_master_multiband(h_, n_bands, lp, hp, ap, curves, a_att, a_rel));
    }
    void reset_master_multiband() { check(s2r_reset_master_multiband(h_)); }
    // state: S2R_MULTIBAND_STATE(n_bands) floats (checkpoints); min_gain: n_bands floats
    void multiband_state(float *state, size_t capacity) { check(s2r_get_multiband_state(h_, state, capacity)); }
    void set_multiband_state(const float *state, size_t count) { check(s2r_set_multiband_state(h_, state, count)); }
    void multiband_meters(float *min_gain, size_t capacity) const { check(s2r_get_multiband_meters(h_, min_gain, capacity)); }
    static int multiband_reference(uint32_t n_bands, const float *lp, const float *hp, const float *ap, const float *curves, const float *a_att,
                                   const float *a_rel, const float *x_lr, uint32_t frames, float *state, float *out_lr, float *bands, float *min_gain) {
        return s2r_multiband_reference(n_bands, lp, hp, ap, curves, a_att, a_rel, x_lr, frames, state, out_lr, bands, min_gain);
    }
    static int multiband_design(double sample_rate, const double *freqs_hz, uint32_t n_splits, float *lp, float *hp, float *ap) {
        return s2r_multiband_design(sample_rate, freqs_hz, n_splits, lp, hp, ap);
    }

    // the loudness and true-peak meters (build-defined; s2r.h: s2r_set_master_loudness): BS.1770 loudness of every bus and the master and
    // the master's true peak, behind the limiter, in sample_master only; master_lr and the stems are the same bits with the meter on or off
    void set_master_loudness(const float coeffs[10], uint32_t hop, uint32_t max_hops) { check(s2r_set_master_loudness(h_, coeffs, hop, max_hops)); }
    void clear_master_loudness() { check(s2r_clear_master_loudness(h_)); }
    // a hop of 0 means off; n_hops: the hop rows stored
    void get_master_loudness(float coeffs[10], uint32_t *hop, uint32_t *max_hops, size_t *n_hops) const { check(s2r_get_master_loudness(h_, coeffs, hop, max_hops, n_hops)); }
    void reset_master_loudness() { check(s2r_reset_master_loudness(h_)); }
    // out: momentary, short-term, integrated in LKFS; programme S2R_MAX_BUSES is the master
    void loudness(uint32_t programme, double out[3]) const { check(s2r_get_loudness(h_, programme, out)); }
    void true_peak(float last[2], float held[2]) const { check(s2r_get_true_peak(h_, last, held)); }
    // state: S2R_LOUDNESS_STATE floats; rows: [n_hops][S2R_LOUDNESS_CHANNELS] (checkpoints)
    void loudness_state(float *state, size_t capacity, uint32_t *pos) { check(s2r_get_loudness_state(h_, state, capacity, pos)); }
    void set_loudness_state(const float *state, size_t count, uint32_t pos) { check(s2r_set_loudness_state(h_, state, count, pos)); }
    void loudness_hops(float *rows, size_t capacity, size_t *n_hops) const { check(s2r_get_loudness_hops(h_, rows, capacity, n_hops)); }
    void set_loudness_hops(const float *rows, size_t n_hops, size_t count) { check(s2r_set_loudness_hops(h_, rows, n_hops, count)); }
    static int loudness_reference(const float coeffs[10], uint32_t hop, const float *stems, uint32_t n_buses, const float *master_lr, uint32_t frames,
                                  float *state, uint32_t *pos, float *rows, size_t rows_capacity, size_t *n_rows, float true_peak[2]) {
        return s2r_loudness_reference(coeffs, hop, stems, n_buses, master_lr, frames, state, pos, rows, rows_capacity, n_rows, true_peak);
    }
    static int loudness_readings(const float *rows, size_t n_hops, uint32_t hop, uint32_t programme, double out[3]) {
        return s2r_loudness_readings(rows, n_hops, hop, programme, out);
    }
    static int loudness_design(double sample_rate, float coeffs[10]) { return s2r_loudness_design(sample_rate, coeffs); }

    // the spectrum meters (build-defined; s2r.h: s2r_set_master_spectrum): a windowed power-of-two FFT of every bus and the master, behind
    // the loudness meters, in sample_master only; master_lr, the stems and the loudness rows are the same bits with the meter on or off
    void set_master_spectrum(uint32_t n_fft, uint32_t hop, const float *window, uint32_t max_rows) { check(s2r_set_master_spectrum(h_, n_fft, hop, window, max_rows)); }
    void clear_master_spectrum() { check(s2r_clear_master_spectrum(h_)); }
    // an n_fft of 0 means off; n_rows: the rows stored; window: n_fft values when window_capacity holds them
    void get_master_spectrum(uint32_t *n_fft, uint32_t *hop, uint32_t *max_rows, size_t *n_rows, float *window = nullptr, size_t window_capacity = 0) const {
        check(s2r_get_master_spectrum(h_, n_fft, hop, max_rows, n_rows, window, window_capacity));
    }
    void reset_master_spectrum() { check(s2r_reset_master_spectrum(h_)); }
    // out_db: n_fft / 2 + 1 values in dB over the last n_avg stored rows; programme S2R_MAX_BUSES is the master
    void spectrum(uint32_t programme, uint32_t n_avg, double *out_db, size_t capacity) const { check(s2r_get_spectrum(h_, programme, n_avg, out_db, capacity)); }
    void spectrum_bands(uint32_t programme, uint32_t n_avg, double sample_rate, uint32_t bands_per_octave, double *out_db, double *centres, size_t capacity,
                        size_t *n_bands) const {
        check(s2r_get_spectrum_bands(h_, programme, n_avg, sample_rate, bands_per_octave, out_db, centres, capacity, n_bands));
    }
    // rows: [n_rows][9][n_fft / 2 + 1]; state: S2R_SPECTRUM_STATE(n_fft) floats (checkpoints)
    void spectrum_rows(float *rows, size_t capacity, size_t *n_rows) const { check(s2r_get_spectrum_rows(h_, rows, capacity, n_rows)); }
    void set_spectrum_rows(const float *rows, size_t n_rows, size_t count) { check(s2r_set_spectrum_rows(h_, rows, n_rows, count)); }
    void spectrum_state(float *state, size_t capacity, uint32_t *pos) { check(s2r_get_spectrum_state(h_, state, capacity, pos)); }
    void set_spectrum_state(const float *state, size_t count, uint32_t pos) { check(s2r_set_spectrum_state(h_, state, count, pos)); }
    static int spectrum_reference(uint32_t n_fft, uint32_t hop, const float *window, const float *stems, uint32_t n_buses, const float *master_lr, uint32_t frames,
                                  float *state, uint32_t *pos, float *rows, size_t rows_capacity, size_t *n_rows) {
        return s2r_spectrum_reference(n_fft, hop, window, stems, n_buses, master_lr, frames, state, pos, rows, rows_capacity, n_rows);
    }
    static int spectrum_readings(const float *rows, size_t n_rows, uint32_t n_fft, const float *window, uint32_t programme, uint32_t n_avg, double *out_db,
                                 size_t capacity) {
        return s2r_spectrum_readings(rows, n_rows, n_fft, window, programme, n_avg, out_db, capacity);
    }
    static int spectrum_band_readings(const float *rows, size_t n_rows, uint32_t n_fft, const float *window, uint32_t programme, uint32_t n_avg, double sample_rate,
                                      uint32_t bands_per_octave, double *out_db, double *centres, size_t capacity, size_t *n_bands) {
        return s2r_spectrum_band_readings(rows, n_rows, n_fft, window, programme, n_avg, sample_rate, bands_per_octave, out_db, centres, capacity, n_bands);
    }
    static int spectrum_window(uint32_t kind, uint32_t n_fft, float *window) { return s2r_spectrum_window(kind, n_fft, window); }
    static int spectrum_twiddles(uint32_t n_fft, float *twiddles) { return s2r_spectrum_twiddles(n_fft, twiddles); }

    // the PCM stage (build-defined; s2r.h: s2r_set_master_pcm): every bus and the master as integers of 8 .. 24 bits, with dither and
    // error-feedback noise shaping, behind the spectrum meters, in fill_master only
    void set_master_pcm(uint32_t bits, uint32_t dither, const float *taps, uint32_t n_taps, uint32_t seed) { check(s2r_set_master_pcm(h_, bits, dither, taps, n_taps, seed)); }
    void clear_master_pcm() { check(s2r_clear_master_pcm(h_)); }
    // any pointer may be null; bits of 0 means off; taps receives S2R_PCM_MAX_TAPS floats
    void get_master_pcm(uint32_t *bits, uint32_t *dither, float *taps, uint32_t *n_taps, uint32_t *seed) const { check(s2r_get_master_pcm(h_, bits, dither, taps, n_taps, seed)); }
    void reset_master_pcm() { check(s2r_reset_master_pcm(h_)); }
    // the [frames][2] samples of a programme (bus b, or S2R_MAX_BUSES for the master) of the last fill_master
    void pcm(uint32_t programme, int32_t *pcm_lr, size_t capacity, size_t *frames) const { check(s2r_get_pcm(h_, programme, pcm_lr, capacity, frames)); }
    void pcm_clips(uint32_t *last, uint32_t *held) const { check(s2r_get_pcm_clips(h_, last, held)); }
    // checkpoints: the S2R_PCM_STATE errors and the frame count
    void pcm_state(float *state, size_t capacity, uint32_t *t) { check(s2r_get_pcm_state(h_, state, capacity, t)); }
    void set_pcm_state(const float *state, size_t count, uint32_t t) { check(s2r_set_pcm_state(h_, state, count, t)); }
    static int pcm_reference(uint32_t bits, uint32_t dither, const float *taps, uint32_t n_taps, uint32_t seed, const float *stems, uint32_t n_buses,
                             const float *master_lr, uint32_t frames, float *state, uint32_t *t, int32_t *pcm, uint32_t *clips) {
        return s2r_pcm_reference(bits, dither, taps, n_taps, seed, stems, n_buses, master_lr, frames, state, t, pcm, clips);
    }
    static int pcm_dither(uint32_t seed, uint32_t t, uint32_t q, uint32_t kind, float *d) { return s2r_pcm_dither(seed, t, q, kind, d); }
    static int pcm_pack(const int32_t *pcm, size_t count, uint32_t bits, uint32_t bytes_per_sample, uint8_t *out) { return s2r_pcm_pack(pcm, count, bits, bytes_per_sample, out); }
    static int pcm_shaper(uint32_t kind, float *taps, uint32_t *n_taps) { return s2r_pcm_shaper(kind, taps, n_taps); }

    // the sample-rate converter (build-defined; s2r.h: s2r_set_master_resampler): every bus and the master resampled by L / M through a
    // polyphase table h[L][T], behind the spectrum meters and in front of the PCM stage, in fill_master only
    void set_master_resampler(uint32_t L, uint32_t M, uint32_t T, const float *table) { check(s2r_set_master_resampler(h_, L, M, T, table)); }
    void clear_master_resampler() { check(s2r_clear_master_resampler(h_)); }
    // any pointer may be null; L of 0 means off; table receives L * T floats
    void get_master_resampler(uint32_t *L, uint32_t *M, uint32_t *T, float *table) const { check(s2r_get_master_resampler(h_, L, M, T, table)); }
    void reset_master_resampler() { check(s2r_reset_master_resampler(h_)); }
    // the [frames][2] output frames of a programme (bus b, or S2R_MAX_BUSES for the master) of the last fill_master
    void resampled(uint32_t programme, float *out_lr, size_t capacity, size_t *frames) const { check(s2r_get_resampled(h_, programme, out_lr, capacity, frames)); }
    // checkpoints: the S2R_RESAMPLER_STATE(T) floats of history and the position
    void resampler_state(float *state, size_t capacity, uint32_t *ph) { check(s2r_get_resampler_state(h_, state, capacity, ph)); }
    void set_resampler_state(const float *state, size_t count, uint32_t ph) { check(s2r_set_resampler_state(h_, state, count, ph)); }
    static int resampler_reference(uint32_t L, uint32_t M, uint32_t T, const float *table, const float *stems, uint32_t n_buses, const float *master_lr,
                                   uint32_t frames, float *state, uint32_t *ph, float *out, size_t capacity, size_t *count) {
        return s2r_resampler_reference(L, M, T, table, stems, n_buses, master_lr, frames, state, ph, out, capacity, count);
    }
    static int resampler_count(uint32_t L, uint32_t M, uint32_t ph, uint32_t frames, size_t *count) { return s2r_resampler_count(L, M, ph, frames, count); }
    static int resampler_design(uint32_t L, uint32_t M, uint32_t T, double beta, double rolloff, float *table) { return s2r_resampler_design(L, M, T, beta, rolloff, table); }

    s2r_synth *handle() { return h_; }

  private:
    void check(int rc) const {
        if (rc != S2R_OK) throw Error(rc, s2r_last_error(h_));
    }
    s2r_synth *h_ = nullptr;
};

}  // namespace s2
