//! `s2_lib::try3::synth`-shaped wrapper over the C ABI of libs2r (include/s2r.h, S2R_ABI_VERSION 4).
//!
//! UNVERIFIED: written without a Rust toolchain (none in the build image); see INTEGRATION.md.
//!
//! The public surface is exactly what `s2_bin` uses today
//! (components/s2_bin/src/main.rs:13,125,132-133,142,147,191,199-205):
//!
//! ```ignore
//! use s2_lib_gpu::synth::{Synth, Note, Velocity};
//! use s2_lib_gpu::units::{SampleRateKhz, Unipolar};
//! let mut synth = Synth::new();
//! synth.note_on(Note(69), Velocity(Unipolar(1.0)));
//! synth.sample(&mut chunk, SampleRateKhz(48_000));
//! synth.note_off(Note(69));
//! ```
//!
//! plus what the boundary adds: a run-time pool size (`with_voices`), several GPUs behind one `Synth`
//! (`with_devices`), events stamped with their 16-frame boundary (`note_events`), the fill in two halves for a caller
//! with two buffers in flight (`sample_begin` / `sample_end`), patch text and patch banks, the stereo copy and the
//! 4x-oversampled fill.

pub mod units {
    /// components/s2_lib/src/try3/units.rs:11
    #[derive(Copy, Clone)]
    pub struct Unipolar<const N: u16>(pub f32);
    /// units.rs:14 — holds Hz despite the name (units.rs:21)
    #[derive(Copy, Clone)]
    pub struct SampleRateKhz(pub u32);
}

pub mod ffi {
    use std::os::raw::{c_char, c_int, c_void};

    /// include/s2r.h `S2R_ABI_VERSION`
    pub const S2R_ABI_VERSION: u32 = 4;
    /// include/s2r.h `S2R_MAX_DEVICES`
    pub const S2R_MAX_DEVICES: usize = 16;

    /// include/s2r.h `s2r_config`
    #[repr(C)]
    pub struct S2rConfig {
        pub struct_size: u32,
        pub total_voices: u32,
        pub shard_begin: u32,
        pub shard_voices: u32,
        pub max_frames: u32,
        pub device: i32,
        pub block_voices: u32,
        pub mix_groups: u32,
        pub reserved0: u32,
        pub shard_interleave: u32,
        pub shard_index: u32,
        pub shard_count: u32,
        pub n_devices: u32,
        pub devices: [i32; S2R_MAX_DEVICES],
    }

    /// include/s2r.h `s2r_adsr` (static_config.rs:38-44)
    #[repr(C)]
    #[derive(Copy, Clone)]
    pub struct S2rAdsr {
        pub attack_ms: f32,
        pub decay_ms: f32,
        pub sustain: f32,
        pub release_ms: f32,
    }

    /// include/s2r.h `s2r_patch` (static_config.rs:4-24 plus the build-defined filter selection)
    #[repr(C)]
    #[derive(Copy, Clone)]
    pub struct S2rPatch {
        pub osc_kind: i32,
        pub osc_gain: f32,
        pub noise: f32,
        pub lpf_freq: f32,
        pub amp_env: S2rAdsr,
        pub mod_env: S2rAdsr,
        pub mod_env_to_osc_freq: f32,
        pub mod_env_to_lpf_freq: f32,
        pub lpf_kind: i32,
        pub lpf_damping: f32,
        pub lpf_q: f32,
    }

    #[repr(C)]
    pub struct S2rSynth {
        _private: [u8; 0],
    }

    /// include/s2r.h `s2r_layer_call`: one call of process::process_layer_buf_simd (process.rs:14-22), st::Layer in place
    #[repr(C)]
    #[derive(Copy, Clone)]
    pub struct S2rLayerCall {
        pub pitch_hz: f32,
        pub offset: u32,
        pub release_offset: u32,
        pub has_release: u8,
        pub program: u8,
        pub _pad: [u8; 2],
        pub phase_accum: f32,
        pub lpf_last: f32,
        pub noise_seed: u32,
        pub filt_x1: f32,
        pub filt_x2: f32,
        pub filt_y1: f32,
        pub filt_y2: f32,
        pub osc_z: f32,
    }

    /// include/s2r.h `s2r_note_event`: `frame` = 0 or the 16-frame boundary inside the next fill
    #[repr(C)]
    #[derive(Copy, Clone)]
    pub struct S2rNoteEvent {
        pub kind: u8, // 0 = note_off, 1 = note_on, 2 = program change (`note` = bank index)
        pub note: u8,
        pub frame: u16,
        pub velocity: f32,
    }

    extern "C" {
        pub fn s2r_abi_version() -> u32;
        pub fn s2r_create(cfg: *const S2rConfig, out: *mut *mut S2rSynth) -> c_int;
        pub fn s2r_destroy(s: *mut S2rSynth);
        pub fn s2r_load_patch(s: *mut S2rSynth, text: *const c_char, len: usize) -> c_int;
        pub fn s2r_set_patch(s: *mut S2rSynth, patch: *const S2rPatch) -> c_int;
        pub fn s2r_get_patch(s: *const S2rSynth, out: *mut S2rPatch) -> c_int;
        pub fn s2r_default_patch(out: *mut S2rPatch);
        pub fn s2r_set_patch_bank(s: *mut S2rSynth, patches: *const S2rPatch, n: u32) -> c_int;
        pub fn s2r_program_change(s: *mut S2rSynth, program: u32) -> c_int;
        pub fn s2r_note_on(s: *mut S2rSynth, note: u8, velocity: f32) -> c_int;
        pub fn s2r_note_off(s: *mut S2rSynth, note: u8) -> c_int;
        pub fn s2r_note_events(s: *mut S2rSynth, events: *const S2rNoteEvent, n: usize) -> c_int;
        pub fn s2r_fill(s: *mut S2rSynth, mono_out: *mut f32, frames: usize, sample_rate_hz: u32) -> c_int;
        pub fn s2r_fill_begin(s: *mut S2rSynth, frames: usize, sample_rate_hz: u32) -> c_int;
        pub fn s2r_fill_end(s: *mut S2rSynth, mono_out: *mut f32, capacity: usize) -> c_int;
        pub fn s2r_fill_pending_frames(s: *const S2rSynth) -> usize;
        pub fn s2r_fills_in_flight(s: *const S2rSynth) -> u32;
        pub fn s2r_fill_stereo(s: *mut S2rSynth, interleaved_lr_out: *mut f32, frames: usize, sample_rate_hz: u32) -> c_int;
        pub fn s2r_fill_oversampled(s: *mut S2rSynth, mono_out: *mut f32, frames: usize, sample_rate_hz: u32) -> c_int;
        pub fn s2r_set_program_pan(s: *mut S2rSynth, program: u32, pan: f32, key_spread: f32) -> c_int;
        pub fn s2r_get_program_pan(s: *const S2rSynth, program: u32, pan: *mut f32, key_spread: *mut f32) -> c_int;
        pub fn s2r_get_voice_pans(s: *mut S2rSynth, pans: *mut f32) -> c_int;
        pub fn s2r_set_voice_pans(s: *mut S2rSynth, pans: *const f32) -> c_int;
        pub fn s2r_fill_panned(s: *mut S2rSynth, interleaved_lr_out: *mut f32, frames: usize, sample_rate_hz: u32) -> c_int;
        pub fn s2r_voice_pan(pan: f32, key_spread: f32, note: u8) -> f32;
        pub fn s2r_pan_gains(p: f32, gl: *mut f32, gr: *mut f32);
        pub fn s2r_set_program_mix(s: *mut S2rSynth, program: u32, level: f32, velocity_sens: f32, bus: u32) -> c_int;
        pub fn s2r_get_program_mix(s: *const S2rSynth, program: u32, level: *mut f32, velocity_sens: *mut f32, bus: *mut u32) -> c_int;
        pub fn s2r_get_voice_mix(s: *mut S2rSynth, gains: *mut f32, buses: *mut u8) -> c_int;
        pub fn s2r_set_voice_mix(s: *mut S2rSynth, gains: *const f32, buses: *const u8) -> c_int;
        pub fn s2r_voice_gain(level: f32, velocity_sens: f32, velocity: f32) -> f32;
        pub fn s2r_fill_buses(s: *mut S2rSynth, out: *mut f32, capacity: usize, n_buses: u32, frames: usize, sample_rate_hz: u32) -> c_int;
        pub fn s2r_set_program_fader(s: *mut S2rSynth, program: u32, fader: f32, pan_shift: f32) -> c_int;
        pub fn s2r_get_program_fader(s: *const S2rSynth, program: u32, fader: *mut f32, pan_shift: *mut f32, applied_fader: *mut f32,
                                     applied_pan_shift: *mut f32) -> c_int;
        pub fn s2r_snap_program_faders(s: *mut S2rSynth) -> c_int;
        pub fn s2r_fader_gains(pan: f32, w: f32, fader: f32, pan_shift: f32, gl: *mut f32, gr: *mut f32);
        pub fn s2r_set_program_send(s: *mut S2rSynth, program: u32, send: f32, send_bus: u32) -> c_int;
        pub fn s2r_get_program_send(s: *const S2rSynth, program: u32, send: *mut f32, send_bus: *mut u32) -> c_int;
        pub fn s2r_get_voice_sends(s: *mut S2rSynth, sends: *mut f32, send_buses: *mut u8) -> c_int;
        pub fn s2r_set_voice_sends(s: *mut S2rSynth, sends: *const f32, send_buses: *const u8) -> c_int;
        pub fn s2r_send_gain(g: f32, send: f32) -> f32;
        pub fn s2r_set_bus_reverb(s: *mut S2rSynth, bus: u32, ir_l: *const f32, ir_r: *const f32, n_taps: u32, dry: f32, wet: f32) -> c_int;
        pub fn s2r_set_bus_reverb_mix(s: *mut S2rSynth, bus: u32, dry: f32, wet: f32) -> c_int;
        pub fn s2r_get_bus_reverb(s: *const S2rSynth, bus: u32, n_taps: *mut u32, dry: *mut f32, wet: *mut f32) -> c_int;
        pub fn s2r_get_bus_reverb_history(s: *mut S2rSynth, bus: u32, lr: *mut f32, capacity: usize) -> c_int;
        pub fn s2r_set_bus_reverb_history(s: *mut S2rSynth, bus: u32, lr: *const f32, count: usize) -> c_int;
        pub fn s2r_reverb_reference(ir: *const f32, n_taps: u32, x_with_history: *const f32, frames: u32, dry: f32, wet: f32,
                                    out: *mut f32) -> c_int;
        pub fn s2r_set_bus_delay(s: *mut S2rSynth, bus: u32, delay_frames: u32, feedback: f32, cross: f32, dry: f32, wet: f32) -> c_int;
        pub fn s2r_set_bus_delay_mix(s: *mut S2rSynth, bus: u32, feedback: f32, cross: f32, dry: f32, wet: f32) -> c_int;
        pub fn s2r_get_bus_delay(s: *const S2rSynth, bus: u32, delay_frames: *mut u32, feedback: *mut f32, cross: *mut f32, dry: *mut f32,
                                 wet: *mut f32) -> c_int;
        pub fn s2r_get_bus_delay_history(s: *mut S2rSynth, bus: u32, lr: *mut f32, capacity: usize) -> c_int;
        pub fn s2r_set_bus_delay_history(s: *mut S2rSynth, bus: u32, lr: *const f32, count: usize) -> c_int;
        pub fn s2r_delay_reference(delay_frames: u32, feedback: f32, cross: f32, dry: f32, wet: f32, x_lr: *const f32, frames: u32,
                                   history_lr: *mut f32, out_lr: *mut f32) -> c_int;
        pub fn s2r_chorus_history_frames(base: f32, depth: f32) -> u32;
        pub fn s2r_set_bus_chorus(s: *mut S2rSynth, bus: u32, voices: u32, base: f32, depth: f32, phase_inc: u32, spread: u32, dry: f32,
                                  wet: f32) -> c_int;
        pub fn s2r_set_bus_chorus_mix(s: *mut S2rSynth, bus: u32, dry: f32, wet: f32) -> c_int;
        pub fn s2r_set_bus_chorus_rate(s: *mut S2rSynth, bus: u32, phase_inc: u32, spread: u32) -> c_int;
        pub fn s2r_get_bus_chorus(s: *const S2rSynth, bus: u32, voices: *mut u32, base: *mut f32, depth: *mut f32, phase_inc: *mut u32,
                                  spread: *mut u32, dry: *mut f32, wet: *mut f32) -> c_int;
        pub fn s2r_get_bus_chorus_state(s: *mut S2rSynth, bus: u32, lr: *mut f32, capacity: usize, phase: *mut u32) -> c_int;
        pub fn s2r_set_bus_chorus_state(s: *mut S2rSynth, bus: u32, lr: *const f32, count: usize, phase: u32) -> c_int;
        pub fn s2r_chorus_reference(voices: u32, base: f32, depth: f32, phase_inc: u32, spread: u32, dry: f32, wet: f32, x_lr: *const f32,
                                    frames: u32, history_lr: *mut f32, phase: *mut u32, out_lr: *mut f32) -> c_int;
        pub fn s2r_flanger_history_frames(base: f32, depth: f32) -> u32;
        pub fn s2r_set_bus_flanger(s: *mut S2rSynth, bus: u32, base: f32, depth: f32, phase_inc: u32, spread: u32, feedback: f32, cross: f32,
                                   dry: f32, wet: f32) -> c_int;
        pub fn s2r_clear_bus_flanger(s: *mut S2rSynth, bus: u32) -> c_int;
        pub fn s2r_set_bus_flanger_params(s: *mut S2rSynth, bus: u32, phase_inc: u32, spread: u32, feedback: f32, cross: f32, dry: f32,
                                          wet: f32) -> c_int;
        pub fn s2r_get_bus_flanger(s: *const S2rSynth, bus: u32, base: *mut f32, depth: *mut f32, phase_inc: *mut u32, spread: *mut u32,
                                   feedback: *mut f32, cross: *mut f32, dry: *mut f32, wet: *mut f32) -> c_int;
        pub fn s2r_get_bus_flanger_state(s: *mut S2rSynth, bus: u32, lr: *mut f32, capacity: usize, phase: *mut u32) -> c_int;
        pub fn s2r_set_bus_flanger_state(s: *mut S2rSynth, bus: u32, lr: *const f32, count: usize, phase: u32) -> c_int;
        pub fn s2r_flanger_reference(base: f32, depth: f32, phase_inc: u32, spread: u32, feedback: f32, cross: f32, dry: f32, wet: f32,
                                     x_lr: *const f32, frames: u32, history_lr: *mut f32, phase: *mut u32, out_lr: *mut f32) -> c_int;
        pub fn s2r_set_bus_eq(s: *mut S2rSynth, bus: u32, n_bands: u32, coeffs: *const f32) -> c_int;
        pub fn s2r_set_bus_eq_coeffs(s: *mut S2rSynth, bus: u32, n_bands: u32, coeffs: *const f32) -> c_int;
        pub fn s2r_get_bus_eq(s: *const S2rSynth, bus: u32, n_bands: *mut u32, coeffs: *mut f32, capacity: usize) -> c_int;
        pub fn s2r_get_bus_eq_state(s: *mut S2rSynth, bus: u32, state: *mut f32, capacity: usize) -> c_int;
        pub fn s2r_set_bus_eq_state(s: *mut S2rSynth, bus: u32, state: *const f32, count: usize) -> c_int;
        pub fn s2r_eq_reference(n_bands: u32, coeffs: *const f32, x_lr: *const f32, frames: u32, state: *mut f32, out_lr: *mut f32) -> c_int;
        pub fn s2r_eq_design(kind: c_int, freq_hz: f64, gain_db: f64, q: f64, sample_rate: f64, coeffs: *mut f32) -> c_int;
        pub fn s2r_set_bus_return(s: *mut S2rSynth, bus: u32, level: f32) -> c_int;
        pub fn s2r_get_bus_return(s: *const S2rSynth, bus: u32, level: *mut f32, applied: *mut f32) -> c_int;
        pub fn s2r_set_master_fader(s: *mut S2rSynth, level: f32) -> c_int;
        pub fn s2r_get_master_fader(s: *const S2rSynth, level: *mut f32, applied: *mut f32) -> c_int;
        pub fn s2r_snap_master(s: *mut S2rSynth) -> c_int;
        pub fn s2r_fill_master(s: *mut S2rSynth, master_lr: *mut f32, stems: *mut f32, stems_capacity: usize, n_buses: u32, frames: usize,
                               sample_rate_hz: u32) -> c_int;
        pub fn s2r_get_meters(s: *const S2rSynth, n_buses: *mut u32, peak: *mut f32, energy: *mut f32, capacity: usize) -> c_int;
        pub fn s2r_master_reference(stems: *const f32, n_buses: u32, frames: u32, r0: *const f32, r1: *const f32, m0: f32, m1: f32,
                                    master_lr: *mut f32, peak: *mut f32, energy: *mut f32) -> c_int;
        pub fn s2r_set_master_limiter(s: *mut S2rSynth, ceiling: f32, lookahead: u32, hold: u32) -> c_int;
        pub fn s2r_clear_master_limiter(s: *mut S2rSynth) -> c_int;
        pub fn s2r_get_master_limiter(s: *const S2rSynth, ceiling: *mut f32, lookahead: *mut u32, hold: *mut u32) -> c_int;
        pub fn s2r_get_limiter_state(s: *mut S2rSynth, xh: *mut f32, n_x: usize, gh: *mut f32, n_g: usize) -> c_int;
        pub fn s2r_set_limiter_state(s: *mut S2rSynth, xh: *const f32, n_x: usize, gh: *const f32, n_g: usize) -> c_int;
        pub fn s2r_get_limiter_meters(s: *const S2rSynth, min_gain: *mut f32, out_peak: *mut f32) -> c_int;
        pub fn s2r_limiter_reference(x: *const f32, frames: u32, ceiling: f32, lookahead: u32, hold: u32, xh: *mut f32, gh: *mut f32,
                                     y: *mut f32, gain: *mut f32) -> c_int;
        pub fn s2r_set_master_limiter_ex(s: *mut S2rSynth, ceiling: f32, lookahead: u32, hold: u32, detector: u32) -> c_int;
        pub fn s2r_get_master_limiter_detector(s: *const S2rSynth, detector: *mut u32) -> c_int;
        pub fn s2r_set_master_multiband(s: *mut S2rSynth, n_bands: u32, lp: *const f32, hp: *const f32, ap: *const f32, curves: *const f32,
                                        a_att: *const f32, a_rel: *const f32) -> c_int;
        pub fn s2r_set_master_multiband_params(s: *mut S2rSynth, n_bands: u32, lp: *const f32, hp: *const f32, ap: *const f32, curves: *const f32,
                                               a_att: *const f32, a_rel: *const f32) -> c_int;
        pub fn s2r_clear_master_multiband(s: *mut S2rSynth) -> c_int;
        pub fn s2r_reset_master_multiband(s: *mut S2rSynth) -> c_int;
        pub fn s2r_get_multiband_state(s: *mut S2rSynth, state: *mut f32, capacity: usize) -> c_int;
        pub fn s2r_set_multiband_state(s: *mut S2rSynth, state: *const f32, count: usize) -> c_int;
        pub fn s2r_get_multiband_meters(s: *const S2rSynth, min_gain: *mut f32, capacity: usize) -> c_int;
        pub fn s2r_get_master_multiband(s: *const S2rSynth, n_bands: *mut u32, lp: *mut f32, hp: *mut f32, ap: *mut f32, curves: *mut f32,
                                        a_att: *mut f32, a_rel: *mut f32) -> c_int;
        pub fn s2r_multiband_reference(n_bands: u32, lp: *const f32, hp: *const f32, ap: *const f32, curves: *const f32, a_att: *const f32,
                                       a_rel: *const f32, x_lr: *const f32, frames: u32, state: *mut f32, out_lr: *mut f32, bands: *mut f32,
                                       min_gain: *mut f32) -> c_int;
        pub fn s2r_multiband_design(sample_rate: f64, freqs_hz: *const f64, n_splits: u32, lp: *mut f32, hp: *mut f32, ap: *mut f32) -> c_int;
        pub fn s2r_set_master_loudness(s: *mut S2rSynth, coeffs: *const f32, hop: u32, max_hops: u32) -> c_int;
        pub fn s2r_clear_master_loudness(s: *mut S2rSynth) -> c_int;
        pub fn s2r_get_master_loudness(s: *const S2rSynth, coeffs: *mut f32, hop: *mut u32, max_hops: *mut u32, n_hops: *mut usize) -> c_int;
        pub fn s2r_reset_master_loudness(s: *mut S2rSynth) -> c_int;
        pub fn s2r_get_loudness(s: *const S2rSynth, programme: u32, out: *mut f64) -> c_int;
        pub fn s2r_get_true_peak(s: *const S2rSynth, last: *mut f32, held: *mut f32) -> c_int;
        pub fn s2r_get_loudness_state(s: *mut S2rSynth, state: *mut f32, capacity: usize, pos: *mut u32) -> c_int;
        pub fn s2r_set_loudness_state(s: *mut S2rSynth, state: *const f32, count: usize, pos: u32) -> c_int;
        pub fn s2r_get_loudness_hops(s: *const S2rSynth, rows: *mut f32, capacity: usize, n_hops: *mut usize) -> c_int;
        pub fn s2r_set_loudness_hops(s: *mut S2rSynth, rows: *const f32, n_hops: usize, count: usize) -> c_int;
        pub fn s2r_loudness_reference(coeffs: *const f32, hop: u32, stems: *const f32, n_buses: u32, master_lr: *const f32, frames: u32,
                                      state: *mut f32, pos: *mut u32, rows: *mut f32, rows_capacity: usize, n_rows: *mut usize,
                                      true_peak: *mut f32) -> c_int;
        pub fn s2r_loudness_readings(rows: *const f32, n_hops: usize, hop: u32, programme: u32, out: *mut f64) -> c_int;
        pub fn s2r_loudness_design(sample_rate: f64, coeffs: *mut f32) -> c_int;
        pub fn s2r_set_master_spectrum(s: *mut S2rSynth, n_fft: u32, hop: u32, window: *const f32, max_rows: u32) -> c_int;
        pub fn s2r_clear_master_spectrum(s: *mut S2rSynth) -> c_int;
        pub fn s2r_get_master_spectrum(s: *const S2rSynth, n_fft: *mut u32, hop: *mut u32, max_rows: *mut u32, n_rows: *mut usize,
                                       window: *mut f32, window_capacity: usize) -> c_int;
        pub fn s2r_reset_master_spectrum(s: *mut S2rSynth) -> c_int;
        pub fn s2r_get_spectrum(s: *const S2rSynth, programme: u32, n_avg: u32, out_db: *mut f64, capacity: usize) -> c_int;
        pub fn s2r_get_spectrum_bands(s: *const S2rSynth, programme: u32, n_avg: u32, sample_rate: f64, bands_per_octave: u32,
                                      out_db: *mut f64, centres: *mut f64, capacity: usize, n_bands: *mut usize) -> c_int;
        pub fn s2r_get_spectrum_rows(s: *const S2rSynth, rows: *mut f32, capacity: usize, n_rows: *mut usize) -> c_int;
        pub fn s2r_set_spectrum_rows(s: *mut S2rSynth, rows: *const f32, n_rows: usize, count: usize) -> c_int;
        pub fn s2r_get_spectrum_state(s: *mut S2rSynth, state: *mut f32, capacity: usize, pos: *mut u32) -> c_int;
        pub fn s2r_set_spectrum_state(s: *mut S2rSynth, state: *const f32, count: usize, pos: u32) -> c_int;
        pub fn s2r_spectrum_reference(n_fft: u32, hop: u32, window: *const f32, stems: *const f32, n_buses: u32, master_lr: *const f32,
                                      frames: u32, state: *mut f32, pos: *mut u32, rows: *mut f32, rows_capacity: usize,
                                      n_rows: *mut usize) -> c_int;
        pub fn s2r_spectrum_readings(rows: *const f32, n_rows: usize, n_fft: u32, window: *const f32, programme: u32, n_avg: u32,
                                     out_db: *mut f64, capacity: usize) -> c_int;
        pub fn s2r_spectrum_band_readings(rows: *const f32, n_rows: usize, n_fft: u32, window: *const f32, programme: u32, n_avg: u32,
                                          sample_rate: f64, bands_per_octave: u32, out_db: *mut f64, centres: *mut f64, capacity: usize,
                                          n_bands: *mut usize) -> c_int;
        pub fn s2r_spectrum_window(kind: u32, n_fft: u32, window: *mut f32) -> c_int;
        pub fn s2r_spectrum_twiddles(n_fft: u32, twiddles: *mut f32) -> c_int;
        pub fn s2r_set_master_pcm(s: *mut S2rSynth, bits: u32, dither: u32, taps: *const f32, n_taps: u32, seed: u32) -> c_int;
        pub fn s2r_clear_master_pcm(s: *mut S2rSynth) -> c_int;
        pub fn s2r_get_master_pcm(s: *const S2rSynth, bits: *mut u32, dither: *mut u32, taps: *mut f32, n_taps: *mut u32, seed: *mut u32) -> c_int;
        pub fn s2r_reset_master_pcm(s: *mut S2rSynth) -> c_int;
        pub fn s2r_get_pcm(s: *const S2rSynth, programme: u32, pcm_lr: *mut i32, capacity: usize, frames: *mut usize) -> c_int;
        pub fn s2r_get_pcm_clips(s: *const S2rSynth, last: *mut u32, held: *mut u32) -> c_int;
        pub fn s2r_get_pcm_state(s: *mut S2rSynth, state: *mut f32, capacity: usize, t: *mut u32) -> c_int;
        pub fn s2r_set_pcm_state(s: *mut S2rSynth, state: *const f32, count: usize, t: u32) -> c_int;
        pub fn s2r_pcm_reference(bits: u32, dither: u32, taps: *const f32, n_taps: u32, seed: u32, stems: *const f32, n_buses: u32,
                                 master_lr: *const f32, frames: u32, state: *mut f32, t: *mut u32, pcm: *mut i32, clips: *mut u32) -> c_int;
        pub fn s2r_pcm_dither(seed: u32, t: u32, q: u32, kind: u32, d: *mut f32) -> c_int;
        pub fn s2r_pcm_pack(pcm: *const i32, count: usize, bits: u32, bytes_per_sample: u32, out: *mut u8) -> c_int;
        pub fn s2r_pcm_shaper(kind: u32, taps: *mut f32, n_taps: *mut u32) -> c_int;
        pub fn s2r_set_master_resampler(s: *mut S2rSynth, l: u32, m: u32, t: u32, table: *const f32) -> c_int;
        pub fn s2r_clear_master_resampler(s: *mut S2rSynth) -> c_int;
        pub fn s2r_get_master_resampler(s: *const S2rSynth, l: *mut u32, m: *mut u32, t: *mut u32, table: *mut f32) -> c_int;
        pub fn s2r_reset_master_resampler(s: *mut S2rSynth) -> c_int;
        pub fn s2r_get_resampled(s: *const S2rSynth, programme: u32, out_lr: *mut f32, capacity: usize, frames: *mut usize) -> c_int;
        pub fn s2r_get_resampler_state(s: *mut S2rSynth, state: *mut f32, capacity: usize, ph: *mut u32) -> c_int;
        pub fn s2r_set_resampler_state(s: *mut S2rSynth, state: *const f32, count: usize, ph: u32) -> c_int;
        pub fn s2r_resampler_reference(l: u32, m: u32, t: u32, table: *const f32, stems: *const f32, n_buses: u32, master_lr: *const f32,
                                       frames: u32, state: *mut f32, ph: *mut u32, out: *mut f32, capacity: usize, count: *mut usize) -> c_int;
        pub fn s2r_resampler_count(l: u32, m: u32, ph: u32, frames: u32, count: *mut usize) -> c_int;
        pub fn s2r_resampler_design(l: u32, m: u32, t: u32, beta: f64, rolloff: f64, table: *mut f32) -> c_int;
        pub fn s2r_shard_voices(s: *const S2rSynth) -> u32;
        pub fn s2r_fill_device(s: *mut S2rSynth, dev_out: *mut f32, frames: usize, sample_rate_hz: u32,
                               hip_stream: *mut c_void) -> c_int;
        pub fn s2r_device_count(s: *const S2rSynth) -> u32;
        pub fn s2r_set_low_latency(s: *mut S2rSynth, enabled: c_int) -> c_int;
        pub fn s2r_set_resident(s: *mut S2rSynth, enabled: c_int) -> c_int;
        pub fn s2r_resident_active(s: *const S2rSynth) -> c_int;
        pub fn s2r_quiesce(s: *mut S2rSynth) -> c_int;
        pub fn s2r_exchange_create(s: *mut S2rSynth, n_ranks: u32, handle_out: *mut c_void, handle_bytes: usize) -> c_int;
        pub fn s2r_exchange_attach(s: *mut S2rSynth, rank: u32, n_ranks: u32, handle: *const c_void, handle_bytes: usize) -> c_int;
        pub fn s2r_process_layers(s: *mut S2rSynth, layers: *mut S2rLayerCall, n_layers: u32, bufs: *mut f32, frames: usize, sample_rate_hz: u32) -> c_int;
        pub fn s2r_set_voice_log(s: *mut S2rSynth, f: Option<extern "C" fn(*mut c_void, u32, u8)>, user: *mut c_void) -> c_int;
        pub fn s2r_build_id() -> *const c_char;
        pub fn s2r_last_error(s: *const S2rSynth) -> *const c_char;
        pub fn s2r_status_string(status: c_int) -> *const c_char;
    }
}

/// Host-only: the pan a note_on gives its voice, and a pan's constant-power gains (gL, gR) — DESIGN.md 4.12.
pub fn voice_pan(pan: f32, key_spread: f32, note: u8) -> f32 {
    unsafe { ffi::s2r_voice_pan(pan, key_spread, note) }
}

pub fn pan_gains(p: f32) -> (f32, f32) {
    let (mut gl, mut gr) = (0.0f32, 0.0f32);
    unsafe { ffi::s2r_pan_gains(p, &mut gl, &mut gr) };
    (gl, gr)
}

/// `S2R_MAX_BUSES`: the most stereo buses one `sample_buses` call writes.
pub const MAX_BUSES: u32 = 8;
/// `S2R_MAX_IR_TAPS`: the longest response of a bus reverb, per channel.
pub const MAX_IR_TAPS: u32 = 65536;
/// `S2R_IR_SEGMENT`: the taps of one segment of the reverb's sum (part of its rule).
pub const IR_SEGMENT: u32 = 256;
/// `S2R_MAX_DELAY_FRAMES`: the longest time of a bus delay, in frames.
pub const MAX_DELAY_FRAMES: u32 = 262144;
/// `S2R_CHORUS_MAX_VOICES`, `S2R_CHORUS_MAX_DELAY`: the most voices of a bus chorus, and the largest `base + depth` (rounded to f32) in
/// frames.
pub const CHORUS_MAX_VOICES: u32 = 8;
pub const CHORUS_MAX_DELAY: f32 = 4095.0;
/// `S2R_FLANGER_MIN_DELAY`, `S2R_FLANGER_MAX_DELAY`: the least `base` of a bus flanger, and the largest `base + depth` (rounded to f32),
/// in frames.
pub const FLANGER_MIN_DELAY: f32 = 32.0;
pub const FLANGER_MAX_DELAY: f32 = 4095.0;
/// `S2R_EQ_MAX_BANDS`: the most biquad bands of a bus EQ, and the kinds of `s2r_eq_kind`.
pub const EQ_MAX_BANDS: u32 = 4;
pub const EQ_PEAK: i32 = 0;
pub const EQ_LOW_SHELF: i32 = 1;
pub const EQ_HIGH_SHELF: i32 = 2;
pub const EQ_LOWPASS: i32 = 3;
pub const EQ_HIGHPASS: i32 = 4;
/// `S2R_METER_BLOCK`: the frames of one block of the meters' energy tree (part of the master section's rule).
pub const METER_BLOCK: u32 = 256;
/// `S2R_LIMITER_MAX_LOOKAHEAD`, `S2R_LIMITER_MAX_HOLD`: the master limiter's longest lookahead and hold in frames, and
/// `S2R_LIMITER_CEILING_LOG2`: its ceiling lies in [2^-20, 2^20].
pub const LIMITER_MAX_LOOKAHEAD: u32 = 1024;
pub const LIMITER_MAX_HOLD: u32 = 4096;
pub const LIMITER_CEILING_LOG2: i32 = 20;

/// Host-only: the gain a note_on of `velocity` gives its voice under a program's level and velocity sensitivity — DESIGN.md 4.13.
pub fn voice_gain(level: f32, velocity_sens: f32, velocity: f32) -> f32 {
    unsafe { ffi::s2r_voice_gain(level, velocity_sens, velocity) }
}

/// Host-only: the gains (gL, gR) of a voice with pan `pan` and gain `w` under a program fader pair — DESIGN.md 4.14.
pub fn fader_gains(pan: f32, w: f32, fader: f32, pan_shift: f32) -> (f32, f32) {
    let (mut gl, mut gr) = (0.0f32, 0.0f32);
    unsafe { ffi::s2r_fader_gains(pan, w, fader, pan_shift, &mut gl, &mut gr) };
    (gl, gr)
}

/// Host-only: the bus reverb's rule for one channel (`s2r_reverb_reference`).  `x_with_history`: `ir.len() - 1`
/// samples of history, oldest first, then the dry samples; returns one output sample per dry sample, or the status.
pub fn reverb_reference(ir: &[f32], x_with_history: &[f32], dry: f32, wet: f32) -> Result<Vec<f32>, i32> {
    assert!(!ir.is_empty() && x_with_history.len() + 1 >= ir.len());
    let frames = x_with_history.len() + 1 - ir.len();
    let mut out = vec![0.0f32; frames];
    let rc = unsafe {
        ffi::s2r_reverb_reference(ir.as_ptr(), ir.len() as u32, x_with_history.as_ptr(), frames as u32, dry, wet, out.as_mut_ptr())
    };
    if rc == 0 { Ok(out) } else { Err(rc) }
}

/// Host-only: the bus delay's rule for both channels (`s2r_delay_reference`).  `x_lr`: L, R pairs; `history_lr`: the
/// line's `2 * delay_frames` floats in front of them, oldest frame first, updated in place to the history after the call; returns one
/// output pair per input pair, or the status.
pub fn delay_reference(delay_frames: u32, feedback: f32, cross: f32, dry: f32, wet: f32, x_lr: &[f32], history_lr: &mut [f32]) -> Result<Vec<f32>, i32> {
    assert!(x_lr.len() % 2 == 0 && history_lr.len() == 2 * delay_frames as usize);
    let mut out = vec![0.0f32; x_lr.len()];
    let rc = unsafe {
        ffi::s2r_delay_reference(delay_frames, feedback, cross, dry, wet, x_lr.as_ptr(), (x_lr.len() / 2) as u32, history_lr.as_mut_ptr(),
                                 out.as_mut_ptr())
    };
    if rc == 0 { Ok(out) } else { Err(rc) }
}

/// `s2r_chorus_history_frames`: the stereo frames of history a chorus of (`base`, `depth`) keeps, or 0 for a pair out of range.
pub fn chorus_history_frames(base: f32, depth: f32) -> u32 {
    unsafe { ffi::s2r_chorus_history_frames(base, depth) }
}

/// An LFO rate in Hz as a `phase_inc`: `round(hz * 2^32 / sample_rate)` modulo 2^32.
pub fn chorus_rate(hz: f64, sample_rate: f64) -> u32 {
    ((hz * 4294967296.0 / sample_rate).round() as u64 & 0xffff_ffff) as u32
}

/// Host-only: the bus chorus's rule for both channels (`s2r_chorus_reference`).  `x_lr`: L, R pairs; `history_lr`: the
/// `2 * chorus_history_frames(base, depth)` floats of input in front of them, oldest frame first, and `phase` the LFO's at the first
/// pair: both updated in place to the state after the call; returns one output pair per input pair, or the status.
pub fn chorus_reference(voices: u32, base: f32, depth: f32, phase_inc: u32, spread: u32, dry: f32, wet: f32, x_lr: &[f32], history_lr: &mut [f32],
                        phase: &mut u32) -> Result<Vec<f32>, i32> {
    let h = chorus_history_frames(base, depth) as usize;
    assert!(x_lr.len() % 2 == 0 && (h == 0 || history_lr.len() == 2 * h));
    let mut out = vec![0.0f32; x_lr.len()];
    let rc = unsafe {
        ffi::s2r_chorus_reference(voices, base, depth, phase_inc, spread, dry, wet, x_lr.as_ptr(), (x_lr.len() / 2) as u32, history_lr.as_mut_ptr(),
                                  phase as *mut u32, out.as_mut_ptr())
    };
    if rc == 0 { Ok(out) } else { Err(rc) }
}

/// `s2r_flanger_history_frames`: the stereo frames of its line signal a flanger of (`base`, `depth`) keeps, or 0 for a pair out of range.
pub fn flanger_history_frames(base: f32, depth: f32) -> u32 {
    unsafe { ffi::s2r_flanger_history_frames(base, depth) }
}

/// Host-only: the bus flanger's rule (`s2r_flanger_reference`).  `x_lr`: L, R pairs; `history_lr`: the
/// `2 * flanger_history_frames(base, depth)` floats of the stage's line signal in front of them, oldest frame first, and `phase` the
/// LFO's at the first pair: both updated in place to the state after the call; returns one output pair per input pair, or the status.
pub fn flanger_reference(base: f32, depth: f32, phase_inc: u32, spread: u32, feedback: f32, cross: f32, dry: f32, wet: f32, x_lr: &[f32],
                         history_lr: &mut [f32], phase: &mut u32) -> Result<Vec<f32>, i32> {
    let h = flanger_history_frames(base, depth) as usize;
    assert!(x_lr.len() % 2 == 0 && (h == 0 || history_lr.len() == 2 * h));
    let mut out = vec![0.0f32; x_lr.len()];
    let rc = unsafe {
        ffi::s2r_flanger_reference(base, depth, phase_inc, spread, feedback, cross, dry, wet, x_lr.as_ptr(), (x_lr.len() / 2) as u32,
                                   history_lr.as_mut_ptr(), phase as *mut u32, out.as_mut_ptr())
    };
    if rc == 0 { Ok(out) } else { Err(rc) }
}

/// Host-only: the bus EQ's rule for both channels (`s2r_eq_reference`).  `coeffs`: `(b0, b1, b2, a1, a2)` per band;
/// `x_lr`: L, R pairs; `state`: `4 * n_bands` floats, `[band][s1_L, s1_R, s2_L, s2_R]`, updated in place to the state after the call;
/// returns one output pair per input pair, or the status.
pub fn eq_reference(coeffs: &[[f32; 5]], x_lr: &[f32], state: &mut [f32]) -> Result<Vec<f32>, i32> {
    assert!(x_lr.len() % 2 == 0 && state.len() == 4 * coeffs.len());
    let mut out = vec![0.0f32; x_lr.len()];
    let rc = unsafe {
        ffi::s2r_eq_reference(coeffs.len() as u32, coeffs.as_ptr() as *const f32, x_lr.as_ptr(), (x_lr.len() / 2) as u32, state.as_mut_ptr(),
                              out.as_mut_ptr())
    };
    if rc == 0 { Ok(out) } else { Err(rc) }
}

/// A band `(b0, b1, b2, a1, a2)` from the usual parameters, by the Audio-EQ-Cookbook formulas with `q` as Q (`s2r_eq_design`): `kind`
/// one of `EQ_PEAK` .. `EQ_HIGHPASS`; computed in f64, divided by a0, rounded once to f32.
pub fn eq_design(kind: i32, freq_hz: f64, gain_db: f64, q: f64, sample_rate: f64) -> Result<[f32; 5], i32> {
    let mut c = [0.0f32; 5];
    let rc = unsafe { ffi::s2r_eq_design(kind, freq_hz, gain_db, q, sample_rate, c.as_mut_ptr()) };
    if rc == 0 { Ok(c) } else { Err(rc) }
}

/// Host-only: the master section's rule (`s2r_master_reference`).  `stems`: `r0.len()` buses of `frames` L, R
/// pairs, bus-major; `r0` / `r1`: the returns' applied and target levels; returns (master, peak, energy) — the meters hold
/// `(n_buses + 1) * 2` entries, bus-major, L then R, the master last — or the status.
pub fn master_reference(stems: &[f32], r0: &[f32], r1: &[f32], m0: f32, m1: f32) -> Result<(Vec<f32>, Vec<f32>, Vec<f32>), i32> {
    let nb = r0.len();
    assert!(nb >= 1 && r1.len() == nb && stems.len() % (2 * nb) == 0);
    let frames = stems.len() / (2 * nb);
    let (mut out, mut peak, mut energy) = (vec![0.0f32; 2 * frames], vec![0.0f32; 2 * (nb + 1)], vec![0.0f32; 2 * (nb + 1)]);
    let rc = unsafe {
        ffi::s2r_master_reference(stems.as_ptr(), nb as u32, frames as u32, r0.as_ptr(), r1.as_ptr(), m0, m1, out.as_mut_ptr(),
                                  peak.as_mut_ptr(), energy.as_mut_ptr())
    };
    if rc == 0 { Ok((out, peak, energy)) } else { Err(rc) }
}

/// `S2R_MULTIBAND_STATE(n_bands)`: 4 floats per crossover section, then the bands' gains; 0 for no band.
pub fn multiband_state_floats(n_bands: usize) -> usize {
    if n_bands == 0 {
        return 0;
    }
    4 * (4 * (n_bands - 1) + (n_bands - 1) * n_bands.saturating_sub(2) / 2) + n_bands
}

/// Host-only: the master multiband compressor's crossover rows (`s2r_multiband_design`) for split frequencies strictly
/// ascending inside (0, sample_rate / 2): (lp, hp, ap), 5 floats per split, ap for the splits behind the first.
pub fn multiband_design(sample_rate: f64, splits_hz: &[f64]) -> Result<(Vec<f32>, Vec<f32>, Vec<f32>), i32> {
    let n = splits_hz.len();
    let (mut lp, mut hp, mut ap) = (vec![0.0f32; 5 * n], vec![0.0f32; 5 * n], vec![0.0f32; 5 * n.saturating_sub(1)]);
    let p = |v: &mut Vec<f32>| if v.is_empty() { std::ptr::null_mut() } else { v.as_mut_ptr() };
    let f = if n == 0 { std::ptr::null() } else { splits_hz.as_ptr() };
    let rc = unsafe { ffi::s2r_multiband_design(sample_rate, f, n as u32, p(&mut lp), p(&mut hp), p(&mut ap)) };
    if rc != 0 {
        return Err(rc);
    }
    Ok((lp, hp, ap))
}

/// Host-only: the master multiband compressor's rule (`s2r_multiband_reference`).  `a_att.len()` bands; `x`: L, R pairs;
/// `state` (`multiband_state_floats` floats) is updated in place.  Returns (out, the bands' minimum gains — infinity for no frames).
#[allow(clippy::too_many_arguments)]
pub fn multiband_reference(lp: &[f32], hp: &[f32], ap: &[f32], curves: &[f32], a_att: &[f32], a_rel: &[f32], x: &[f32], state: &mut [f32]) -> Result<(Vec<f32>, Vec<f32>), i32> {
    let b = a_att.len();
    let frames = x.len() / 2;
    if b == 0 || b > 4 || a_rel.len() != b || curves.len() != 513 * b || lp.len() != 5 * (b - 1) || hp.len() != lp.len() || ap.len() != 5 * b.saturating_sub(2)
        || state.len() != multiband_state_floats(b)
    {
        return Err(-1);
    }
    let p = |v: &[f32]| if v.is_empty() { std::ptr::null() } else { v.as_ptr() };
    let (mut out, mut mn) = (vec![0.0f32; 2 * frames], vec![f32::INFINITY; b]);
    let rc = unsafe {
        ffi::s2r_multiband_reference(b as u32, p(lp), p(hp), p(ap), curves.as_ptr(), a_att.as_ptr(), a_rel.as_ptr(), p(x), frames as u32, state.as_mut_ptr(),
                                     if frames == 0 { std::ptr::null_mut() } else { out.as_mut_ptr() }, std::ptr::null_mut(), mn.as_mut_ptr())
    };
    if rc != 0 {
        return Err(rc);
    }
    Ok((out, mn))
}

/// Host-only: the master limiter's rule (`s2r_limiter_reference`).  `x`: L, R pairs; `xh` (`2 * lookahead`
/// floats) and `gh` (`2 * lookahead + hold` floats) are the state, updated in place; returns (y, gain) or the status.
pub fn limiter_reference(x: &[f32], ceiling: f32, lookahead: u32, hold: u32, xh: &mut [f32], gh: &mut [f32]) -> Result<(Vec<f32>, Vec<f32>), i32> {
    assert!(x.len() % 2 == 0 && xh.len() == 2 * lookahead as usize && gh.len() == 2 * lookahead as usize + hold as usize);
    let frames = x.len() / 2;
    let (mut y, mut gain) = (vec![0.0f32; 2 * frames], vec![0.0f32; frames]);
    let rc = unsafe {
        ffi::s2r_limiter_reference(x.as_ptr(), frames as u32, ceiling, lookahead, hold, xh.as_mut_ptr(), gh.as_mut_ptr(), y.as_mut_ptr(),
                                   gain.as_mut_ptr())
    };
    if rc == 0 { Ok((y, gain)) } else { Err(rc) }
}

/// Host-only: the gain of a voice's aux send, `g * send` in one rounded multiply — DESIGN.md 4.15.
pub fn send_gain(g: f32, send: f32) -> f32 {
    unsafe { ffi::s2r_send_gain(g, send) }
}

pub mod synth {
    use super::ffi;
    use super::units::{SampleRateKhz, Unipolar};
    use std::ffi::CStr;

    /// components/s2_lib/src/try3/synth.rs:7 — the reference's fixed pool size
    pub const NUM_VOICES: u32 = 8;
    /// largest slice `sample` is ever handed by s2_bin (audio_player.rs:21 uses 2048-frame buffers)
    pub const MAX_FRAMES: u32 = 2048;

    /// synth.rs:16
    #[derive(Eq, PartialEq, Copy, Clone)]
    pub struct Note(pub u8);
    /// synth.rs:18
    #[derive(Copy, Clone)]
    pub struct Velocity(pub Unipolar<1>);

    pub struct Synth {
        handle: *mut ffi::S2rSynth,
    }

    // like the reference's Synth (plain data behind &mut), the handle may move between threads
    // but must only be used by one at a time
    unsafe impl Send for Synth {}

    fn fail(handle: *const ffi::S2rSynth, status: i32) -> ! {
        let msg = unsafe {
            if handle.is_null() {
                CStr::from_ptr(ffi::s2r_status_string(status))
            } else {
                CStr::from_ptr(ffi::s2r_last_error(handle))
            }
        };
        // the reference panics in the same situations (process.rs:36,71 `expect("overflow")`)
        panic!("libs2r status {}: {}", status, msg.to_string_lossy());
    }

    impl Synth {
        /// synth.rs:54-59
        pub fn new() -> Synth {
            Synth::with_voices(NUM_VOICES)
        }

        pub fn with_voices(voices: u32) -> Synth {
            Synth::create(voices, &[], 0)
        }

        /// One `Synth` over several GPUs: the pool is dealt out to `devices` in runs of 64 voices, the allocation
        /// policy (synth.rs:61-120) runs once per event on the calling thread, and the shards' partial mixes are
        /// added in shard order on `devices[0]`.  `voices` must be a multiple of 256 x the number of devices.
        pub fn with_devices(voices: u32, devices: &[i32]) -> Synth {
            Synth::create(voices, devices, 64)
        }

        fn create(voices: u32, devices: &[i32], interleave: u32) -> Synth {
            if unsafe { ffi::s2r_abi_version() } != ffi::S2R_ABI_VERSION {
                panic!("libs2r: ABI version mismatch (this shim was written for {})", ffi::S2R_ABI_VERSION);
            }
            assert!(devices.len() <= ffi::S2R_MAX_DEVICES);
            let mut list = [0i32; ffi::S2R_MAX_DEVICES];
            list[..devices.len()].copy_from_slice(devices);
            let cfg = ffi::S2rConfig {
                struct_size: std::mem::size_of::<ffi::S2rConfig>() as u32,
                total_voices: voices,
                shard_begin: 0,
                shard_voices: 0,
                max_frames: MAX_FRAMES,
                device: -1,
                block_voices: 0,
                mix_groups: 0,
                reserved0: 0,
                shard_interleave: if devices.len() > 1 { interleave } else { 0 },
                shard_index: 0,
                shard_count: 1,
                n_devices: devices.len() as u32,
                devices: list,
            };
            let mut handle = std::ptr::null_mut();
            let rc = unsafe { ffi::s2r_create(&cfg, &mut handle) };
            if rc != 0 {
                fail(std::ptr::null(), rc);
            }
            Synth { handle }
        }

        fn check(&self, rc: i32) {
            if rc != 0 {
                fail(self.handle, rc);
            }
        }

        /// Multi-timbral extension: the patch (bank index) the following note_ons use.
        pub fn program_change(&mut self, program: u32) {
            self.check(unsafe { ffi::s2r_program_change(self.handle, program) });
        }

        /// example.synth2 text (the reference has no loader; an empty body is default_config())
        pub fn load_patch(&mut self, text: &str) {
            self.check(unsafe { ffi::s2r_load_patch(self.handle, text.as_ptr() as *const _, text.len()) });
        }

        /// static_config::Layer as a value (synth.rs:10 `config`)
        pub fn set_patch(&mut self, patch: &ffi::S2rPatch) {
            self.check(unsafe { ffi::s2r_set_patch(self.handle, patch) });
        }

        /// A bank of 1..=256 patches; `program_change` picks the one a note_on gives its voice.
        pub fn set_patch_bank(&mut self, patches: &[ffi::S2rPatch]) {
            self.check(unsafe { ffi::s2r_set_patch_bank(self.handle, patches.as_ptr(), patches.len() as u32) });
        }

        /// synth.rs:61-70
        pub fn note_on(&mut self, note: Note, velocity: Velocity) {
            self.check(unsafe { ffi::s2r_note_on(self.handle, note.0, (velocity.0).0) });
        }

        /// synth.rs:72-80
        pub fn note_off(&mut self, note: Note) {
            self.check(unsafe { ffi::s2r_note_off(self.handle, note.0) });
        }

        /// Events stamped with the 16-frame boundary (`frame`) at which s2_bin's loop
        /// (main.rs:138-143) would have applied them; they take effect inside the next `sample`.
        pub fn note_events(&mut self, events: &[ffi::S2rNoteEvent]) {
            self.check(unsafe { ffi::s2r_note_events(self.handle, events.as_ptr(), events.len()) });
        }

        /// synth.rs:154-169 — overwrites `buffer`
        pub fn sample(&mut self, buffer: &mut [f32], sample_rate: SampleRateKhz) {
            self.check(unsafe { ffi::s2r_fill(self.handle, buffer.as_mut_ptr(), buffer.len(), sample_rate.0) });
        }

        /// First half of `sample` for a caller that keeps two buffers in flight, as s2_bin does between its synth and
        /// audio threads (audio_player.rs:56-60, main.rs:135-149): queues a fill of `frames`; at most two may be
        /// queued.
        pub fn sample_begin(&mut self, frames: usize, sample_rate: SampleRateKhz) {
            self.check(unsafe { ffi::s2r_fill_begin(self.handle, frames, sample_rate.0) });
        }

        /// Second half: waits for the OLDEST queued fill and overwrites the front of `buffer` with its frames;
        /// returns how many.  Panics (like a slice length mismatch in the reference would) when `buffer` is shorter
        /// than that fill.
        pub fn sample_end(&mut self, buffer: &mut [f32]) -> usize {
            let frames = unsafe { ffi::s2r_fill_pending_frames(self.handle) };
            self.check(unsafe { ffi::s2r_fill_end(self.handle, buffer.as_mut_ptr(), buffer.len()) });
            frames
        }

        /// The audio callback's mono -> every channel copy (audio_player.rs:224-228) done on the device:
        /// `interleaved` holds L, R pairs with L == R; its length is twice the frame count.
        pub fn sample_stereo(&mut self, interleaved: &mut [f32], sample_rate: SampleRateKhz) {
            assert!(interleaved.len() % 2 == 0);
            self.check(unsafe {
                ffi::s2r_fill_stereo(self.handle, interleaved.as_mut_ptr(), interleaved.len() / 2, sample_rate.0)
            });
        }

        /// Build-defined: rendered at 4 x `sample_rate` and decimated to `buffer.len()` frames.
        pub fn sample_oversampled(&mut self, buffer: &mut [f32], sample_rate: SampleRateKhz) {
            self.check(unsafe {
                ffi::s2r_fill_oversampled(self.handle, buffer.as_mut_ptr(), buffer.len(), sample_rate.0)
            });
        }

        /// Build-defined true stereo (`s2r_fill_panned`, include/s2r.h): pan and key spread, both in [-1, 1], of a bank
        /// program — what a note_on under that program gives its voice.
        pub fn set_program_pan(&mut self, program: u32, pan: f32, key_spread: f32) {
            self.check(unsafe { ffi::s2r_set_program_pan(self.handle, program, pan, key_spread) });
        }

        pub fn get_program_pan(&self, program: u32) -> (f32, f32) {
            let (mut pan, mut spread) = (0.0f32, 0.0f32);
            self.check(unsafe { ffi::s2r_get_program_pan(self.handle, program, &mut pan, &mut spread) });
            (pan, spread)
        }

        /// Every voice's pan, pool order on a handle that renders its whole pool: the checkpoint companion of the state.
        pub fn voice_pans(&mut self) -> Vec<f32> {
            let mut pans = vec![0.0f32; unsafe { ffi::s2r_shard_voices(self.handle) } as usize];
            self.check(unsafe { ffi::s2r_get_voice_pans(self.handle, pans.as_mut_ptr()) });
            pans
        }

        pub fn set_voice_pans(&mut self, pans: &[f32]) {
            assert!(pans.len() == unsafe { ffi::s2r_shard_voices(self.handle) } as usize);
            self.check(unsafe { ffi::s2r_set_voice_pans(self.handle, pans.as_ptr()) });
        }

        /// The panned two-channel mixdown: `interleaved` holds L, R pairs; its length is twice the frame count.
        pub fn sample_panned(&mut self, interleaved: &mut [f32], sample_rate: SampleRateKhz) {
            assert!(interleaved.len() % 2 == 0);
            self.check(unsafe {
                ffi::s2r_fill_panned(self.handle, interleaved.as_mut_ptr(), interleaved.len() / 2, sample_rate.0)
            });
        }

        /// Build-defined voice mixer (`s2r_fill_buses`, include/s2r.h): level and velocity sensitivity (both in [0, 1]) and
        /// output bus (below `MAX_BUSES`) of a bank program — what a note_on under that program gives its voice.
        pub fn set_program_mix(&mut self, program: u32, level: f32, velocity_sens: f32, bus: u32) {
            self.check(unsafe { ffi::s2r_set_program_mix(self.handle, program, level, velocity_sens, bus) });
        }

        pub fn get_program_mix(&self, program: u32) -> (f32, f32, u32) {
            let (mut level, mut sens, mut bus) = (0.0f32, 0.0f32, 0u32);
            self.check(unsafe { ffi::s2r_get_program_mix(self.handle, program, &mut level, &mut sens, &mut bus) });
            (level, sens, bus)
        }

        /// Every voice's gain and bus, pool order on a handle that renders its whole pool: checkpoint companions of the state.
        pub fn voice_mix(&mut self) -> (Vec<f32>, Vec<u8>) {
            let n = unsafe { ffi::s2r_shard_voices(self.handle) } as usize;
            let (mut gains, mut buses) = (vec![0.0f32; n], vec![0u8; n]);
            self.check(unsafe { ffi::s2r_get_voice_mix(self.handle, gains.as_mut_ptr(), buses.as_mut_ptr()) });
            (gains, buses)
        }

        pub fn set_voice_mix(&mut self, gains: &[f32], buses: &[u8]) {
            let n = unsafe { ffi::s2r_shard_voices(self.handle) } as usize;
            assert!(gains.len() == n && buses.len() == n);
            self.check(unsafe { ffi::s2r_set_voice_mix(self.handle, gains.as_ptr(), buses.as_ptr()) });
        }

        /// The panned mixdown onto `n_buses` stereo buses from one render pass: `out` is bus-major, L, R pairs inside a bus;
        /// its length is `2 * frames * n_buses`.
        pub fn sample_buses(&mut self, out: &mut [f32], n_buses: u32, sample_rate: SampleRateKhz) {
            assert!(n_buses >= 1 && out.len() % (2 * n_buses as usize) == 0);
            let frames = out.len() / (2 * n_buses as usize);
            self.check(unsafe { ffi::s2r_fill_buses(self.handle, out.as_mut_ptr(), out.len(), n_buses, frames, sample_rate.0) });
        }

        /// Build-defined live program faders (`s2r_set_program_fader`, include/s2r.h): the target of a program's fader (in
        /// [0, 1]) and pan shift (in [-2, 2]); every voice sounding on the program reaches it as a ramp across the next
        /// `sample_buses` call.
        pub fn set_program_fader(&mut self, program: u32, fader: f32, pan_shift: f32) {
            self.check(unsafe { ffi::s2r_set_program_fader(self.handle, program, fader, pan_shift) });
        }

        /// (fader, pan_shift, applied_fader, applied_pan_shift): the target, and where the last bus fill left the pair.
        pub fn get_program_fader(&self, program: u32) -> (f32, f32, f32, f32) {
            let (mut f, mut sh, mut af, mut ash) = (0.0f32, 0.0f32, 0.0f32, 0.0f32);
            self.check(unsafe { ffi::s2r_get_program_fader(self.handle, program, &mut f, &mut sh, &mut af, &mut ash) });
            (f, sh, af, ash)
        }

        /// applied = target for every program, now: a hard cut, and the middle step of restoring a checkpoint.
        pub fn snap_program_faders(&mut self) {
            self.check(unsafe { ffi::s2r_snap_program_faders(self.handle) });
        }

        /// Build-defined aux sends (`s2r_set_program_send`, include/s2r.h): the send (in [0, 1]) of a bank program and the bus it
        /// feeds (below `MAX_BUSES`) — what a note_on under that program gives its voice: a second feed of gain * send, post-pan and
        /// post-fader, in `sample_buses` only.
        pub fn set_program_send(&mut self, program: u32, send: f32, send_bus: u32) {
            self.check(unsafe { ffi::s2r_set_program_send(self.handle, program, send, send_bus) });
        }

        pub fn get_program_send(&self, program: u32) -> (f32, u32) {
            let (mut send, mut bus) = (0.0f32, 0u32);
            self.check(unsafe { ffi::s2r_get_program_send(self.handle, program, &mut send, &mut bus) });
            (send, bus)
        }

        /// Build-defined per-bus convolution reverb (`s2r_set_bus_reverb`, include/s2r.h): `ir_l.len()` taps per channel (`ir_r`
        /// `None`: `ir_l` for both), a dry and a wet in [0, 1]; replaces any earlier reverb of the bus and zeroes its history.  In
        /// `sample_buses` only.
        pub fn set_bus_reverb(&mut self, bus: u32, ir_l: &[f32], ir_r: Option<&[f32]>, dry: f32, wet: f32) {
            assert!(!ir_l.is_empty() && ir_r.map_or(true, |r| r.len() == ir_l.len()));
            let r = ir_r.map_or(std::ptr::null(), |r| r.as_ptr());
            self.check(unsafe { ffi::s2r_set_bus_reverb(self.handle, bus, ir_l.as_ptr(), r, ir_l.len() as u32, dry, wet) });
        }

        pub fn clear_bus_reverb(&mut self, bus: u32) {
            self.check(unsafe { ffi::s2r_set_bus_reverb(self.handle, bus, std::ptr::null(), std::ptr::null(), 0, 0.0, 0.0) });
        }

        /// Dry and wet alone; taps and history stay.
        pub fn set_bus_reverb_mix(&mut self, bus: u32, dry: f32, wet: f32) {
            self.check(unsafe { ffi::s2r_set_bus_reverb_mix(self.handle, bus, dry, wet) });
        }

        /// (n_taps, dry, wet); n_taps is 0 for a bus without a reverb.
        pub fn get_bus_reverb(&self, bus: u32) -> (u32, f32, f32) {
            let (mut k, mut dry, mut wet) = (0u32, 0.0f32, 0.0f32);
            self.check(unsafe { ffi::s2r_get_bus_reverb(self.handle, bus, &mut k, &mut dry, &mut wet) });
            (k, dry, wet)
        }

        /// The `2 * (n_taps - 1)` floats of the reverb's history, oldest frame first, L then R: checkpoint companion of `voice_sends`.
        pub fn bus_reverb_history(&mut self, bus: u32) -> Vec<f32> {
            let k = self.get_bus_reverb(bus).0 as usize;
            let mut lr = vec![0.0f32; 2 * k.max(1) - 2];
            self.check(unsafe { ffi::s2r_get_bus_reverb_history(self.handle, bus, lr.as_mut_ptr(), lr.len()) });
            lr
        }

        pub fn set_bus_reverb_history(&mut self, bus: u32, lr: &[f32]) {
            self.check(unsafe { ffi::s2r_set_bus_reverb_history(self.handle, bus, lr.as_ptr(), lr.len()) });
        }

        /// Build-defined per-bus feedback delay (`s2r_set_bus_delay`, include/s2r.h) in front of the bus's reverb: `delay_frames` in
        /// 1 ..= MAX_DELAY_FRAMES, feedback and cross in [-1, 1] with |feedback| + |cross| <= 1, dry and wet in [0, 1]; replaces any
        /// earlier delay of the bus and zeroes its history.  In `sample_buses` and `sample_master` only.
        pub fn set_bus_delay(&mut self, bus: u32, delay_frames: u32, feedback: f32, cross: f32, dry: f32, wet: f32) {
            assert!(delay_frames >= 1, "clear_bus_delay removes a delay");
            self.check(unsafe { ffi::s2r_set_bus_delay(self.handle, bus, delay_frames, feedback, cross, dry, wet) });
        }

        pub fn clear_bus_delay(&mut self, bus: u32) {
            self.check(unsafe { ffi::s2r_set_bus_delay(self.handle, bus, 0, 0.0, 0.0, 0.0, 0.0) });
        }

        /// The four levels alone; the delay's time and history stay.
        pub fn set_bus_delay_mix(&mut self, bus: u32, feedback: f32, cross: f32, dry: f32, wet: f32) {
            self.check(unsafe { ffi::s2r_set_bus_delay_mix(self.handle, bus, feedback, cross, dry, wet) });
        }

        /// (delay_frames, feedback, cross, dry, wet); delay_frames is 0 for a bus without a delay.
        pub fn get_bus_delay(&self, bus: u32) -> (u32, f32, f32, f32, f32) {
            let (mut d, mut fb, mut cross, mut dry, mut wet) = (0u32, 0.0f32, 0.0f32, 0.0f32, 0.0f32);
            self.check(unsafe { ffi::s2r_get_bus_delay(self.handle, bus, &mut d, &mut fb, &mut cross, &mut dry, &mut wet) });
            (d, fb, cross, dry, wet)
        }

        /// The `2 * delay_frames` floats of the delay's history, oldest frame first, L then R: checkpoint companion of
        /// `bus_reverb_history`.
        pub fn bus_delay_history(&mut self, bus: u32) -> Vec<f32> {
            let d = self.get_bus_delay(bus).0 as usize;
            let mut lr = vec![0.0f32; 2 * d];
            self.check(unsafe { ffi::s2r_get_bus_delay_history(self.handle, bus, lr.as_mut_ptr(), lr.len()) });
            lr
        }

        pub fn set_bus_delay_history(&mut self, bus: u32, lr: &[f32]) {
            self.check(unsafe { ffi::s2r_set_bus_delay_history(self.handle, bus, lr.as_ptr(), lr.len()) });
        }

        /// Build-defined per-bus chorus (`s2r_set_bus_chorus`, include/s2r.h) in front of the bus's delay: `voices` in
        /// 1 ..= CHORUS_MAX_VOICES, `base >= 1` and `depth >= 0` frames with `base + depth` (rounded to f32) at most CHORUS_MAX_DELAY,
        /// `phase_inc` (`chorus_rate`) and `spread` in 2^-32 turns, dry and wet in [0, 1]; replaces any earlier chorus of the bus and
        /// zeroes its history and phase.  In `sample_buses` and `sample_master` only.
        pub fn set_bus_chorus(&mut self, bus: u32, voices: u32, base: f32, depth: f32, phase_inc: u32, spread: u32, dry: f32, wet: f32) {
            assert!(voices >= 1, "clear_bus_chorus removes a chorus");
            self.check(unsafe { ffi::s2r_set_bus_chorus(self.handle, bus, voices, base, depth, phase_inc, spread, dry, wet) });
        }

        pub fn clear_bus_chorus(&mut self, bus: u32) {
            self.check(unsafe { ffi::s2r_set_bus_chorus(self.handle, bus, 0, 0.0, 0.0, 0, 0, 0.0, 0.0) });
        }

        /// The two levels alone; the chorus's state stays.
        pub fn set_bus_chorus_mix(&mut self, bus: u32, dry: f32, wet: f32) {
            self.check(unsafe { ffi::s2r_set_bus_chorus_mix(self.handle, bus, dry, wet) });
        }

        /// The LFO's step and the channels' spread alone; phase and history stay, so nothing clicks.
        pub fn set_bus_chorus_rate(&mut self, bus: u32, phase_inc: u32, spread: u32) {
            self.check(unsafe { ffi::s2r_set_bus_chorus_rate(self.handle, bus, phase_inc, spread) });
        }

        /// (voices, base, depth, phase_inc, spread, dry, wet); voices is 0 for a bus without a chorus.
        pub fn get_bus_chorus(&self, bus: u32) -> (u32, f32, f32, u32, u32, f32, f32) {
            let (mut v, mut pi, mut sp) = (0u32, 0u32, 0u32);
            let (mut base, mut depth, mut dry, mut wet) = (0.0f32, 0.0f32, 0.0f32, 0.0f32);
            self.check(unsafe { ffi::s2r_get_bus_chorus(self.handle, bus, &mut v, &mut base, &mut depth, &mut pi, &mut sp, &mut dry, &mut wet) });
            (v, base, depth, pi, sp, dry, wet)
        }

        /// The `2 * chorus_history_frames(base, depth)` floats of the chorus's history, oldest frame first, L then R, and the LFO's
        /// phase: checkpoint companion of `bus_delay_history`.
        pub fn bus_chorus_state(&mut self, bus: u32) -> (Vec<f32>, u32) {
            let c = self.get_bus_chorus(bus);
            let mut lr = vec![0.0f32; 2 * super::chorus_history_frames(c.1, c.2) as usize];
            let mut phase = 0u32;
            self.check(unsafe { ffi::s2r_get_bus_chorus_state(self.handle, bus, lr.as_mut_ptr(), lr.len(), &mut phase) });
            (lr, phase)
        }

        pub fn set_bus_chorus_state(&mut self, bus: u32, lr: &[f32], phase: u32) {
            self.check(unsafe { ffi::s2r_set_bus_chorus_state(self.handle, bus, lr.as_ptr(), lr.len(), phase) });
        }

        /// Build-defined per-bus flanger (`s2r_set_bus_flanger`, include/s2r.h) behind the bus's drive and in front of its chorus: one
        /// tap `base + depth * triangle` frames late (`base >= FLANGER_MIN_DELAY`, `depth >= 0`, `base + depth` rounded to f32
        /// `<= FLANGER_MAX_DELAY`) into the stage's own line signal, fed back by `feedback` and into the other channel by `cross` (each
        /// in [-1, 1], `|feedback| + |cross| <= 1`); `phase_inc` (`chorus_rate`) and `spread` in 2^-32 turns, dry and wet in [0, 1];
        /// replaces any earlier flanger of the bus and zeroes its line and phase.  In `sample_buses` and `sample_master` only.
        pub fn set_bus_flanger(&mut self, bus: u32, base: f32, depth: f32, phase_inc: u32, spread: u32, feedback: f32, cross: f32, dry: f32, wet: f32) {
            self.check(unsafe { ffi::s2r_set_bus_flanger(self.handle, bus, base, depth, phase_inc, spread, feedback, cross, dry, wet) });
        }

        pub fn clear_bus_flanger(&mut self, bus: u32) {
            self.check(unsafe { ffi::s2r_clear_bus_flanger(self.handle, bus) });
        }

        /// Everything but `base` and `depth`; line and phase stay, so rate and resonance move without a click.
        pub fn set_bus_flanger_params(&mut self, bus: u32, phase_inc: u32, spread: u32, feedback: f32, cross: f32, dry: f32, wet: f32) {
            self.check(unsafe { ffi::s2r_set_bus_flanger_params(self.handle, bus, phase_inc, spread, feedback, cross, dry, wet) });
        }

        /// (base, depth, phase_inc, spread, feedback, cross, dry, wet); base is 0 for a bus without a flanger.
        pub fn get_bus_flanger(&self, bus: u32) -> (f32, f32, u32, u32, f32, f32, f32, f32) {
            let (mut base, mut depth, mut fb, mut cr, mut dry, mut wet) = (0.0f32, 0.0f32, 0.0f32, 0.0f32, 0.0f32, 0.0f32);
            let (mut pi, mut sp) = (0u32, 0u32);
            self.check(unsafe { ffi::s2r_get_bus_flanger(self.handle, bus, &mut base, &mut depth, &mut pi, &mut sp, &mut fb, &mut cr, &mut dry, &mut wet) });
            (base, depth, pi, sp, fb, cr, dry, wet)
        }

        /// The `2 * flanger_history_frames(base, depth)` floats of the flanger's line, oldest frame first, L then R, and the LFO's
        /// phase: checkpoint companion of `bus_chorus_state`.
        pub fn bus_flanger_state(&mut self, bus: u32) -> (Vec<f32>, u32) {
            let c = self.get_bus_flanger(bus);
            let mut lr = vec![0.0f32; 2 * super::flanger_history_frames(c.0, c.1) as usize];
            let mut phase = 0u32;
            self.check(unsafe { ffi::s2r_get_bus_flanger_state(self.handle, bus, lr.as_mut_ptr(), lr.len(), &mut phase) });
            (lr, phase)
        }

        pub fn set_bus_flanger_state(&mut self, bus: u32, lr: &[f32], phase: u32) {
            self.check(unsafe { ffi::s2r_set_bus_flanger_state(self.handle, bus, lr.as_ptr(), lr.len(), phase) });
        }

        /// Build-defined per-bus parametric EQ (`s2r_set_bus_eq`, include/s2r.h) at the head of the chain, in front of the bus's
        /// chorus: 1 ..= EQ_MAX_BANDS biquad bands `(b0, b1, b2, a1, a2)`, normalised by a0, finite, `|a2| < 1` and `|a1| < 1 + a2`
        /// (`eq_design` makes one); replaces any earlier EQ of the bus and zeroes its state.  In `sample_buses` and `sample_master` only.
        pub fn set_bus_eq(&mut self, bus: u32, coeffs: &[[f32; 5]]) {
            assert!(!coeffs.is_empty(), "clear_bus_eq removes an EQ");
            self.check(unsafe { ffi::s2r_set_bus_eq(self.handle, bus, coeffs.len() as u32, coeffs.as_ptr() as *const f32) });
        }

        pub fn clear_bus_eq(&mut self, bus: u32) {
            self.check(unsafe { ffi::s2r_set_bus_eq(self.handle, bus, 0, std::ptr::null()) });
        }

        /// The coefficients alone, as many bands as the EQ has; the state stays, so a band moves without a restart.
        pub fn set_bus_eq_coeffs(&mut self, bus: u32, coeffs: &[[f32; 5]]) {
            self.check(unsafe { ffi::s2r_set_bus_eq_coeffs(self.handle, bus, coeffs.len() as u32, coeffs.as_ptr() as *const f32) });
        }

        /// The bands of the bus's EQ; empty for a bus without one.
        pub fn get_bus_eq(&self, bus: u32) -> Vec<[f32; 5]> {
            let mut n = 0u32;
            let mut c = [[0.0f32; 5]; super::EQ_MAX_BANDS as usize];
            self.check(unsafe { ffi::s2r_get_bus_eq(self.handle, bus, &mut n, c.as_mut_ptr() as *mut f32, 5 * c.len()) });
            c[..n as usize].to_vec()
        }

        /// The `4 * n_bands` floats of the EQ's state, `[band][s1_L, s1_R, s2_L, s2_R]`: checkpoint companion of `bus_chorus_state`.
        pub fn bus_eq_state(&mut self, bus: u32) -> Vec<f32> {
            let mut st = vec![0.0f32; 4 * self.get_bus_eq(bus).len()];
            self.check(unsafe { ffi::s2r_get_bus_eq_state(self.handle, bus, st.as_mut_ptr(), st.len()) });
            st
        }

        pub fn set_bus_eq_state(&mut self, bus: u32, state: &[f32]) {
            self.check(unsafe { ffi::s2r_set_bus_eq_state(self.handle, bus, state.as_ptr(), state.len()) });
        }

        /// Build-defined master section (`s2r_fill_master`, include/s2r.h): the target of a bus's return level (in [0, 1]), reached
        /// as a ramp across the next `sample_master` call.  In `sample_master` only.
        pub fn set_bus_return(&mut self, bus: u32, level: f32) {
            self.check(unsafe { ffi::s2r_set_bus_return(self.handle, bus, level) });
        }

        /// (level, applied): the target, and where the last master fill left the return.
        pub fn get_bus_return(&self, bus: u32) -> (f32, f32) {
            let (mut level, mut applied) = (0.0f32, 0.0f32);
            self.check(unsafe { ffi::s2r_get_bus_return(self.handle, bus, &mut level, &mut applied) });
            (level, applied)
        }

        pub fn set_master_fader(&mut self, level: f32) {
            self.check(unsafe { ffi::s2r_set_master_fader(self.handle, level) });
        }

        pub fn get_master_fader(&self) -> (f32, f32) {
            let (mut level, mut applied) = (0.0f32, 0.0f32);
            self.check(unsafe { ffi::s2r_get_master_fader(self.handle, &mut level, &mut applied) });
            (level, applied)
        }

        /// applied = target for every return and the master fader, now: a hard cut, and the middle step of restoring a checkpoint.
        pub fn snap_master(&mut self) {
            self.check(unsafe { ffi::s2r_snap_master(self.handle) });
        }

        /// `sample_buses` with the master section behind it: `master` takes `2 * frames` floats; `stems`, when given, what
        /// `sample_buses` writes (`2 * frames * n_buses` floats) — `None`: the stems never cross to the host.
        pub fn sample_master(&mut self, master: &mut [f32], stems: Option<&mut [f32]>, n_buses: u32, sample_rate: SampleRateKhz) {
            assert!(n_buses >= 1 && master.len() % 2 == 0);
            let frames = master.len() / 2;
            let (p, cap) = match stems {
                Some(st) => { assert!(st.len() >= 2 * frames * n_buses as usize); (st.as_mut_ptr(), st.len()) }
                None => (std::ptr::null_mut(), 0),
            };
            self.check(unsafe { ffi::s2r_fill_master(self.handle, master.as_mut_ptr(), p, cap, n_buses, frames, sample_rate.0) });
        }

        /// (peak, energy) of the last successful `sample_master` call: `(n_buses + 1) * 2` entries each, bus-major, L then R, the
        /// master last.
        pub fn meters(&self) -> (Vec<f32>, Vec<f32>) {
            let cap = 2 * (super::MAX_BUSES as usize + 1);
            let (mut n, mut peak, mut energy) = (0u32, vec![0.0f32; cap], vec![0.0f32; cap]);
            self.check(unsafe { ffi::s2r_get_meters(self.handle, &mut n, peak.as_mut_ptr(), energy.as_mut_ptr(), cap) });
            peak.truncate(2 * (n as usize + 1));
            energy.truncate(2 * (n as usize + 1));
            (peak, energy)
        }

        /// Build-defined master limiter (`s2r_set_master_limiter`, include/s2r.h): a look-ahead limiter behind the master fader, in
        /// `sample_master` only.  The master is delayed by `lookahead` frames; the stems are not.
        pub fn set_master_limiter(&mut self, ceiling: f32, lookahead: u32, hold: u32) {
            self.check(unsafe { ffi::s2r_set_master_limiter(self.handle, ceiling, lookahead, hold) });
        }

        /// ... with the true-peak detector (`s2r_set_master_limiter_ex`, detector 1): the gain follows the 4x-interpolated magnitude,
        /// and the master is delayed by `lookahead + 8` frames.
        pub fn set_master_limiter_true_peak(&mut self, ceiling: f32, lookahead: u32, hold: u32) {
            self.check(unsafe { ffi::s2r_set_master_limiter_ex(self.handle, ceiling, lookahead, hold, 1) });
        }

        /// 0: the sample peak (and off); 1: the true peak.
        pub fn get_master_limiter_detector(&self) -> u32 {
            let mut d = 0u32;
            self.check(unsafe { ffi::s2r_get_master_limiter_detector(self.handle, &mut d) });
            d
        }

        pub fn clear_master_limiter(&mut self) {
            self.check(unsafe { ffi::s2r_clear_master_limiter(self.handle) });
        }

        /// (ceiling, lookahead, hold); a lookahead of 0 means off.
        pub fn get_master_limiter(&self) -> (f32, u32, u32) {
            let (mut c, mut l, mut h) = (0.0f32, 0u32, 0u32);
            self.check(unsafe { ffi::s2r_get_master_limiter(self.handle, &mut c, &mut l, &mut h) });
            (c, l, h)
        }

        /// (xh, gh): the limiter's carried input (`2 * lookahead` floats, `2 * (lookahead + 16)` with the true-peak detector) and gains
        /// (`2 * lookahead + hold`), oldest first.
        pub fn limiter_state(&mut self) -> (Vec<f32>, Vec<f32>) {
            let (_, l, h) = self.get_master_limiter();
            let more = if self.get_master_limiter_detector() == 1 { 16usize } else { 0usize };
            let (mut xh, mut gh) = (vec![0.0f32; 2 * (l as usize + more)], vec![0.0f32; 2 * l as usize + h as usize]);
            self.check(unsafe { ffi::s2r_get_limiter_state(self.handle, xh.as_mut_ptr(), xh.len(), gh.as_mut_ptr(), gh.len()) });
            (xh, gh)
        }

        pub fn set_limiter_state(&mut self, xh: &[f32], gh: &[f32]) {
            self.check(unsafe { ffi::s2r_set_limiter_state(self.handle, xh.as_ptr(), xh.len(), gh.as_ptr(), gh.len()) });
        }

        /// (min_gain, out_peak) of the last successful `sample_master` call that ran the limiter.
        pub fn limiter_meters(&self) -> (f32, f32) {
            let (mut g, mut p) = (0.0f32, 0.0f32);
            self.check(unsafe { ffi::s2r_get_limiter_meters(self.handle, &mut g, &mut p) });
            (g, p)
        }

        /// Build-defined master multiband compressor (`s2r_set_master_multiband`, include/s2r.h): the master split into `a_att.len()`
        /// bands (1 .. 4) between the master fader and the limiter, each compressed by its own curve of 513 gains, and added back.
        /// `lp`, `hp`: 5 floats per split; `ap`: 5 floats per split behind the first; empty slices for arrays of no rows.
        pub fn set_master_multiband(&mut self, lp: &[f32], hp: &[f32], ap: &[f32], curves: &[f32], a_att: &[f32], a_rel: &[f32]) {
            let b = a_att.len();
            assert!(a_rel.len() == b && curves.len() == b * 513 && lp.len() + 5 == b * 5 && hp.len() == lp.len() && ap.len() + 10 == (b.max(2)) * 5);
            let p = |v: &[f32]| if v.is_empty() { std::ptr::null() } else { v.as_ptr() };
            self.check(unsafe { ffi::s2r_set_master_multiband(self.handle, b as u32, p(lp), p(hp), p(ap), curves.as_ptr(), a_att.as_ptr(), a_rel.as_ptr()) });
        }

        /// ... the parameters alone, with the band count that is set: the state stays.
        pub fn set_master_multiband_params(&mut self, lp: &[f32], hp: &[f32], ap: &[f32], curves: &[f32], a_att: &[f32], a_rel: &[f32]) {
            let b = a_att.len();
            assert!(a_rel.len() == b && curves.len() == b * 513 && lp.len() + 5 == b * 5 && hp.len() == lp.len() && ap.len() + 10 == (b.max(2)) * 5);
            let p = |v: &[f32]| if v.is_empty() { std::ptr::null() } else { v.as_ptr() };
            self.check(unsafe { ffi::s2r_set_master_multiband_params(self.handle, b as u32, p(lp), p(hp), p(ap), curves.as_ptr(), a_att.as_ptr(), a_rel.as_ptr()) });
        }

        pub fn clear_master_multiband(&mut self) {
            self.check(unsafe { ffi::s2r_clear_master_multiband(self.handle) });
        }

        /// Filters and gains as right after a set; the parameters stay.
        pub fn reset_master_multiband(&mut self) {
            self.check(unsafe { ffi::s2r_reset_master_multiband(self.handle) });
        }

        /// The band count that is set; 0 when the stage is off.
        pub fn master_multiband_bands(&self) -> usize {
            let mut b = 0u32;
            let null = std::ptr::null_mut();
            self.check(unsafe { ffi::s2r_get_master_multiband(self.handle, &mut b, null, null, null, null, null, null) });
            b as usize
        }

        /// (lp, hp, ap, curves, a_att, a_rel) as they are set; `None` when the stage is off.
        #[allow(clippy::type_complexity)]
        pub fn get_master_multiband(&self) -> Option<(Vec<f32>, Vec<f32>, Vec<f32>, Vec<f32>, Vec<f32>, Vec<f32>)> {
            let b = self.master_multiband_bands();
            if b == 0 {
                return None;
            }
            let (mut lp, mut hp, mut ap) = (vec![0.0f32; 5 * (b - 1)], vec![0.0f32; 5 * (b - 1)], vec![0.0f32; 5 * b.saturating_sub(2)]);
            let (mut curves, mut att, mut rel) = (vec![0.0f32; 513 * b], vec![0.0f32; b], vec![0.0f32; b]);
            let p = |v: &mut Vec<f32>| if v.is_empty() { std::ptr::null_mut() } else { v.as_mut_ptr() };
            self.check(unsafe {
                ffi::s2r_get_master_multiband(self.handle, std::ptr::null_mut(), p(&mut lp), p(&mut hp), p(&mut ap), curves.as_mut_ptr(), att.as_mut_ptr(), rel.as_mut_ptr())
            });
            Some((lp, hp, ap, curves, att, rel))
        }

        /// The stage's state (checkpoints): 4 floats per section — 0, 4, 9, 15 sections for 1 .. 4 bands —, then the bands' gains.  The
        /// band count is the handle's; with the stage off the library refuses the call.
        pub fn multiband_state(&mut self) -> Vec<f32> {
            let b = self.master_multiband_bands();
            let mut st = vec![0.0f32; multiband_state_floats(b).max(1)];
            self.check(unsafe { ffi::s2r_get_multiband_state(self.handle, st.as_mut_ptr(), st.len()) });
            st.truncate(multiband_state_floats(b));
            st
        }

        pub fn set_multiband_state(&mut self, state: &[f32]) {
            self.check(unsafe { ffi::s2r_set_multiband_state(self.handle, state.as_ptr(), state.len()) });
        }

        /// Every band's minimum gain over the last successful `sample_master` call that ran the stage.
        pub fn multiband_meters(&self) -> Vec<f32> {
            let b = self.master_multiband_bands();
            let mut g = vec![0.0f32; 4];
            self.check(unsafe { ffi::s2r_get_multiband_meters(self.handle, g.as_mut_ptr(), g.len()) });
            g.truncate(b);
            g
        }

        /// Every voice's send and send bus: checkpoint companions of `voice_mix`.
        pub fn voice_sends(&mut self) -> (Vec<f32>, Vec<u8>) {
            let n = unsafe { ffi::s2r_shard_voices(self.handle) } as usize;
            let (mut sends, mut buses) = (vec![0.0f32; n], vec![0u8; n]);
            self.check(unsafe { ffi::s2r_get_voice_sends(self.handle, sends.as_mut_ptr(), buses.as_mut_ptr()) });
            (sends, buses)
        }

        pub fn set_voice_sends(&mut self, sends: &[f32], send_buses: &[u8]) {
            let n = unsafe { ffi::s2r_shard_voices(self.handle) } as usize;
            assert!(sends.len() == n && send_buses.len() == n);
            self.check(unsafe { ffi::s2r_set_voice_sends(self.handle, sends.as_ptr(), send_buses.as_ptr()) });
        }

        /// For the reference's own call pattern — `sample()` per 16 frames from the audio callback (main.rs:138-147): keeps a
        /// resident render kernel on the device between calls, so that a fill is a command in mapped host memory, not a
        /// launch.  Small pools only (one workgroup: at most 256 voices); same samples either way.
        pub fn set_low_latency(&mut self, enabled: bool) {
            self.check(unsafe { ffi::s2r_set_low_latency(self.handle, if enabled { 1 } else { 0 }) });
        }

        /// The throughput caller's form of the same idea (`s2r_set_resident`, include/s2r.h): the shard's whole render grid
        /// stays on the device between fills — a fill is a posted command, not a launch — for `sample`, `sample_stereo` and
        /// `sample_begin` / `sample_end`; every shard of a `with_devices` Synth gets one.  Same samples either way.
        pub fn set_resident(&mut self, enabled: bool) {
            self.check(unsafe { ffi::s2r_set_resident(self.handle, if enabled { 1 } else { 0 }) });
        }

        /// stops any resident kernel of this Synth and waits for it (before the caller synchronises the whole device)
        pub fn quiesce(&mut self) {
            self.check(unsafe { ffi::s2r_quiesce(self.handle) });
        }

        /// One process per GPU without a collective in the step: rank 0 creates the exchange (the ranks' partial rows meet in
        /// a block of its device memory and its last workgroup adds them in rank order) and hands the 64 handle bytes to the
        /// other ranks, which `exchange_attach`.  Every rank then drives its shard's Synth with the same events and the same
        /// `sample` / `sample_begin` / `sample_end` calls; rank 0's buffers receive the mix.
        pub fn exchange_create(&mut self, n_ranks: u32) -> [u8; 64] {
            let mut h = [0u8; 64];
            self.check(unsafe { ffi::s2r_exchange_create(self.handle, n_ranks, h.as_mut_ptr() as *mut _, h.len()) });
            h
        }

        pub fn exchange_attach(&mut self, rank: u32, n_ranks: u32, handle: &[u8; 64]) {
            self.check(unsafe { ffi::s2r_exchange_attach(self.handle, rank, n_ranks, handle.as_ptr() as *const _, handle.len()) });
        }

        /// which sources the loaded libs2r was built from (`s2r_build_id`)
        pub fn build_id() -> String {
            unsafe { CStr::from_ptr(ffi::s2r_build_id()) }.to_string_lossy().into_owned()
        }

        /// how many GPUs render this Synth
        pub fn device_count(&self) -> u32 {
            unsafe { ffi::s2r_device_count(self.handle) }
        }

        /// `log::debug!("using new voice index {} for note {}", …)` of `next_voice` (synth.rs:118) through the `log` facade's
        /// place: `f(voice_index, note)` per note_on.  `None` switches it off.
        pub fn set_voice_log(&mut self, f: Option<extern "C" fn(*mut std::os::raw::c_void, u32, u8)>) {
            self.check(unsafe { ffi::s2r_set_voice_log(self.handle, f, std::ptr::null_mut()) });
        }

        /// process::process_layer_buf_simd (process.rs:14-49) for layers the caller keeps itself, `layers.len()` of them side
        /// by side: this Synth is the workspace (its patch is the `sc::Layer`, its voices are replaced), `bufs` is
        /// `[layers.len()][frames]`, every `S2rLayerCall`'s state fields are advanced in place.
        pub fn process_layers(&mut self, layers: &mut [ffi::S2rLayerCall], bufs: &mut [f32], frames: usize, sample_rate: SampleRateKhz) {
            assert!(bufs.len() >= layers.len() * frames);
            self.check(unsafe { ffi::s2r_process_layers(self.handle, layers.as_mut_ptr(), layers.len() as u32, bufs.as_mut_ptr(), frames, sample_rate.0) });
        }
    }

    impl Drop for Synth {
        fn drop(&mut self) {
            unsafe { ffi::s2r_destroy(self.handle) }
        }
    }
}
