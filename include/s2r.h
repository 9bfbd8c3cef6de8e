/*
 * s2r.h — C ABI of libs2r: the MI355X (gfx950) voice-render path behind s2_lib's
 * buffer-fill API.
 *
 * This is the drop-in boundary.  Each entry point names the reference interface it
 * replaces (paths relative to /root/reference/components/s2_lib/src/try3/).  The
 * reference's public surface is `synth::Synth::{new, note_on, note_off, sample}`
 * (synth.rs:53-80,154-169) as used by s2_bin (components/s2_bin/src/main.rs:132-147,
 * 198-205); rust/s2_lib_gpu/src/lib.rs wraps this header back into exactly those
 * signatures, include/s2_synth.hpp does the same for C++.
 *
 * Conventions
 *   - every function returns an s2r_status (0 = ok, < 0 = error); nothing unwinds or
 *     aborts across the boundary (the reference panics instead: process.rs:36,71);
 *   - a handle is NOT thread-safe: one caller thread at a time, like `&mut Synth`;
 *   - s2r_fill OVERWRITES the caller's buffer (synth.rs:201-202) and returns when it is
 *     complete; no allocation happens inside fill;
 *   - note events take effect at the next fill boundary (s2_bin applies MIDI between
 *     `sample` calls: main.rs:140-147);
 *   - the library needs a gfx950 device: s2r_create fails with S2R_ERR_NO_DEVICE
 *     otherwise.  There is no CPU fallback.
 */
#ifndef S2R_H
#define S2R_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Changes when a struct layout or an existing signature changes.  Entry points added since 4.0 without touching either:
 * s2r_set_low_latency, s2r_low_latency_active, s2r_build_id, s2r_set_resident, s2r_resident_active, s2r_quiesce,
 * s2r_exchange_create, s2r_exchange_attach, s2r_voice_pool_set_threads, s2r_voice_pool_resolve, s2r_set_program_pan,
 * s2r_get_program_pan, s2r_get_voice_pans, s2r_set_voice_pans, s2r_fill_panned, s2r_voice_pan, s2r_pan_gains,
 * s2r_set_program_mix, s2r_get_program_mix, s2r_get_voice_mix, s2r_set_voice_mix, s2r_voice_gain, s2r_fill_buses,
 * s2r_set_program_fader, s2r_get_program_fader, s2r_snap_program_faders, s2r_fader_gains, s2r_set_program_send,
 * s2r_get_program_send, s2r_get_voice_sends, s2r_set_voice_sends, s2r_send_gain, s2r_set_bus_reverb, s2r_set_bus_reverb_mix,
 * s2r_get_bus_reverb, s2r_get_bus_reverb_history, s2r_set_bus_reverb_history, s2r_reverb_reference, s2r_set_bus_return,
 * s2r_get_bus_return, s2r_set_master_fader, s2r_get_master_fader, s2r_snap_master, s2r_fill_master, s2r_get_meters,
 * s2r_master_reference, s2r_set_master_limiter, s2r_clear_master_limiter, s2r_get_master_limiter, s2r_get_limiter_state,
 * s2r_set_limiter_state, s2r_get_limiter_meters, s2r_limiter_reference, s2r_set_bus_delay, s2r_set_bus_delay_mix,
 * s2r_get_bus_delay, s2r_get_bus_delay_history, s2r_set_bus_delay_history, s2r_delay_reference, s2r_chorus_history_frames,
 * s2r_set_bus_chorus, s2r_set_bus_chorus_mix, s2r_set_bus_chorus_rate, s2r_get_bus_chorus, s2r_get_bus_chorus_state,
 * s2r_set_bus_chorus_state, s2r_chorus_reference, s2r_set_bus_eq, s2r_set_bus_eq_coeffs, s2r_get_bus_eq, s2r_get_bus_eq_state,
 * s2r_set_bus_eq_state, s2r_eq_reference, s2r_eq_design, s2r_set_bus_dynamics, s2r_clear_bus_dynamics, s2r_set_bus_dynamics_params,
 * s2r_get_bus_dynamics, s2r_get_bus_dynamics_state, s2r_set_bus_dynamics_state, s2r_get_bus_dynamics_meter, s2r_dynamics_reference,
 * s2r_dynamics_curve, s2r_dynamics_coef, s2r_set_bus_room, s2r_clear_bus_room, s2r_set_bus_room_params, s2r_get_bus_room,
 * s2r_get_bus_room_state, s2r_set_bus_room_state, s2r_room_state_floats, s2r_room_reference, s2r_room_design, s2r_set_bus_drive,
 * s2r_clear_bus_drive, s2r_set_bus_drive_params, s2r_get_bus_drive, s2r_get_bus_drive_history, s2r_set_bus_drive_history,
 * s2r_drive_reference, s2r_drive_taps, s2r_drive_curve, s2r_flanger_history_frames, s2r_set_bus_flanger, s2r_clear_bus_flanger,
 * s2r_set_bus_flanger_params, s2r_get_bus_flanger, s2r_get_bus_flanger_state, s2r_set_bus_flanger_state, s2r_flanger_reference,
 * s2r_set_master_loudness, s2r_clear_master_loudness, s2r_get_master_loudness, s2r_reset_master_loudness, s2r_get_loudness,
 * s2r_get_true_peak, s2r_get_loudness_state, s2r_set_loudness_state, s2r_get_loudness_hops, s2r_set_loudness_hops,
 * s2r_loudness_reference, s2r_loudness_readings, s2r_loudness_design, s2r_set_master_spectrum, s2r_clear_master_spectrum,
 * s2r_get_master_spectrum, s2r_reset_master_spectrum, s2r_get_spectrum, s2r_get_spectrum_bands, s2r_get_spectrum_rows,
 * s2r_set_spectrum_rows, s2r_get_spectrum_state, s2r_set_spectrum_state, s2r_spectrum_reference, s2r_spectrum_readings,
 * s2r_spectrum_band_readings, s2r_spectrum_window, s2r_spectrum_twiddles, s2r_set_master_pcm, s2r_clear_master_pcm,
 * s2r_get_master_pcm, s2r_reset_master_pcm, s2r_get_pcm, s2r_get_pcm_clips, s2r_get_pcm_state, s2r_set_pcm_state,
 * s2r_pcm_reference, s2r_pcm_dither, s2r_pcm_pack, s2r_pcm_shaper, s2r_set_master_resampler, s2r_clear_master_resampler,
 * s2r_get_master_resampler, s2r_reset_master_resampler, s2r_get_resampled, s2r_get_resampler_state, s2r_set_resampler_state,
 * s2r_resampler_reference, s2r_resampler_count, s2r_resampler_design, s2r_set_master_limiter_ex, s2r_get_master_limiter_detector,
 * s2r_limiter_tp_reference, s2r_set_master_multiband, s2r_set_master_multiband_params, s2r_clear_master_multiband,
 * s2r_get_master_multiband, s2r_reset_master_multiband, s2r_get_multiband_state, s2r_set_multiband_state, s2r_get_multiband_meters,
 * s2r_multiband_reference, s2r_multiband_design. */
#define S2R_ABI_VERSION 4

typedef enum {
    S2R_OK = 0,
    S2R_ERR_INVALID = -1,          /* bad argument / null handle */
    S2R_ERR_NO_DEVICE = -2,        /* no usable gfx950 device */
    S2R_ERR_HIP = -3,              /* a HIP runtime call failed; see s2r_last_error */
    S2R_ERR_PATCH_SYNTAX = -4,     /* .synth2 text rejected */
    S2R_ERR_PATCH_RANGE = -5,      /* value outside its unit's range (units.rs:55-65) */
    S2R_ERR_TOO_MANY_FRAMES = -6,  /* frames > max_frames given at create */
    S2R_ERR_OFFSET_OVERFLOW = -7,  /* a voice's frame offset would pass u32::MAX: the
                                      reference panics here (process.rs:36 "overflow") */
    S2R_ERR_OUT_OF_MEMORY = -8
} s2r_status;

/* static_config.rs:26-32 (declaration order) */
typedef enum { S2R_OSC_SQUARE = 0, S2R_OSC_SAW = 1, S2R_OSC_TRIANGLE = 2, S2R_OSC_SINE = 3,
               /* build-defined alias-suppressed shapes (the reference has only the naive ones above and links to the
                * literature, notes.md:32,79): differentiated polynomial waveforms, DESIGN.md 4.10 gives the op sequence */
               S2R_OSC_DPW_SAW = 4, S2R_OSC_DPW_SQUARE = 5, S2R_OSC_DPW_TRIANGLE = 6 } s2r_osc_kind;

/* static_config.rs:38-44  sc::Adsr  (Ms, Ms, Unipolar<1>, Ms) */
typedef struct { float attack_ms, decay_ms, sustain, release_ms; } s2r_adsr;

/* static_config.rs:4-24  sc::Layer — the patch.  ONE patch is shared by all voices, as in
 * the reference (synth.rs:10). */
typedef struct {
    int32_t osc_kind;              /* s2r_osc_kind          sc::Oscillator.kind */
    float osc_gain;                /* Unipolar<1>           sc::Oscillator.gain */
    float noise;                   /* Unipolar<1>           sc::Layer.noise */
    float lpf_freq;                /* Hz                    sc::LowPassFilter.freq */
    s2r_adsr amp_env;
    s2r_adsr mod_env;
    float mod_env_to_osc_freq;     /* Bipolar<10>           sc::Modulations */
    float mod_env_to_lpf_freq;     /* Bipolar<10> */
    /* Which filter the layer runs at the modulated cutoff.  The reference's live path is the
     * one-pole of filters.rs (S2R_FILT_ONEPOLE, the default); dsp_filters.rs:25-180 holds four
     * more that nothing in the reference calls yet — here they are selectable per patch. */
    int32_t lpf_kind;              /* s2r_filter_kind */
    float lpf_damping;             /* Unipolar<10>          SecondOrder*Filter.damping_factor
                                      (dsp_filters.rs:95 "sqrt(2) is neutral"), LP2/HP2 only */
    float lpf_q;                   /* Unipolar<10>          SecondOrderBandPassFilter.quality_factor
                                      (dsp_filters.rs:194 "3 is neutral"), BP2 only; must be > 0 */
} s2r_patch;

typedef enum {
    S2R_FILT_ONEPOLE = 0,          /* filters.rs:16-34          LowPassFilter */
    S2R_FILT_LP1 = 1,              /* dsp_filters.rs:25-45      FirstOrderLowPassFilter */
    S2R_FILT_HP1 = 2,              /* dsp_filters.rs:60-80      FirstOrderHighPassFilter */
    S2R_FILT_LP2 = 3,              /* dsp_filters.rs:99-130     SecondOrderLowPassFilter */
    S2R_FILT_HP2 = 4,              /* dsp_filters.rs:149-180    SecondOrderHighPassFilter */
    S2R_FILT_BP2 = 5,              /* dsp_filters.rs:199-230    SecondOrderBandPassFilter (center = the cutoff) */
    /* build-defined (the reference only names an SVF, notes.md:63): trapezoidal state-variable
     * filter at the modulated cutoff, resonance lpf_q (> 0); DESIGN.md 4.6 gives the op sequence */
    S2R_FILT_SVF_LP = 6, S2R_FILT_SVF_BP = 7, S2R_FILT_SVF_HP = 8
} s2r_filter_kind;

#define S2R_MAX_DEVICES 16
typedef struct {
    uint32_t struct_size;          /* = sizeof(s2r_config) */
    uint32_t total_voices;         /* size of the voice pool; the reference fixes it at
                                      NUM_VOICES = 8 (synth.rs:7) */
    uint32_t shard_begin;          /* first pool index rendered by THIS handle */
    uint32_t shard_voices;         /* voices rendered by this handle; 0 => total_voices.
                                      Voice allocation always runs over the whole pool, so
                                      every shard's handle must see the same event stream */
    uint32_t max_frames;           /* largest `frames` a fill will be asked for */
    int32_t device;                /* HIP device ordinal; -1 => current device */
    uint32_t block_voices;         /* voices per workgroup: 64..1024, multiple of 64;
                                      0 => 256.  Part of the mix-tree spec */
    uint32_t mix_groups;           /* >= 1: second-level grouping of the block partials so a
                                      1-GPU run reproduces the G-GPU summation order; 0 => 1 */
    uint32_t reserved0;            /* must be 0 */
    /* Round-robin sharding (0 => off: this handle renders the contiguous range above).  G > 0: the
     * pool is dealt out in runs of G consecutive voices to shard_count handles, and this one
     * (shard_index) renders every shard_count-th run — its local voice l is pool voice
     * ((l / G) * shard_count + shard_index) * G + l % G; shard_begin is ignored and shard_voices is
     * total_voices / shard_count.  G is a multiple of 16 that divides block_voices, and
     * total_voices a multiple of G * shard_count.  The allocation policy sweeps the pool in index
     * order (synth.rs:101-120 picks the oldest voice, first index on ties), so contiguous shards take
     * a burst of note-ons one GPU at a time; dealt-out shards share it. */
    uint32_t shard_interleave;
    uint32_t shard_index;
    uint32_t shard_count;
    /* Device list.  n_devices <= 1: the handle renders on `device`.  n_devices = N > 1: ONE handle
     * renders the pool on devices[0..N) — the pool is cut into N shards (contiguous ranges when shard_interleave is
     * 0, else dealt out in runs of shard_interleave voices), shard k lives on devices[k] (an ordinal may repeat), the
     * allocation policy of synth.rs:61-120 runs ONCE per event on the calling thread and the event is routed to the
     * shard that holds the chosen voice (the shards' kernels are launched by the calling thread too, shard after
     * shard, each on its device's stream); every fill each shard leaves its partial mix in row k of a buffer on
     * devices[0] (a peer-to-peer write over xGMI, 4 KiB) and devices[0] adds the rows in shard order rooted at +0.0
     * (synth.rs:176,195) — with contiguous shards the very association one device produces with mix_groups = N.
     * shard_begin / shard_voices / shard_index / shard_count must be 0 (or shard_count 1) then; total_voices must be
     * a multiple of N * block_voices. */
    uint32_t n_devices;
    int32_t devices[S2R_MAX_DEVICES];
} s2r_config;

/* One voice's complete state, for checkpoint/resume and tests.
 * synth.rs:23-30 (Voice) + state.rs:10-21 (st::Layer). */
typedef struct {
    uint8_t note;                  /* Voice.note */
    uint8_t started;               /* current_frame_offset.is_some() */
    uint8_t released;              /* release_frame_offset.is_some() */
    uint8_t program;               /* patch bank index the voice was started with */
    uint32_t current_frame_offset;
    uint32_t release_frame_offset;
    float pitch_hz;                /* note_to_pitch(note), synth.rs:208-212 */
    float phase_accum;             /* OscillatorState (None == 0.0, oscillators.rs:483) */
    float lpf_last;                /* LowPassFilterState.last */
    uint32_t noise_seed;           /* NoiseState.seed (always 0 in the reference, synth.rs:68) */
    float velocity;                /* stored, never used in rendering (synth.rs:18,26) */
    float filt_x1, filt_x2, filt_y1, filt_y2;   /* dsp_filters.rs:12-17,82-89 filter states */
    float osc_z;                   /* DPW oscillators: the differentiator's memory; NaN = none yet (a fresh voice) */
} s2r_voice_state;

typedef struct s2r_synth s2r_synth;

/* Synth::new (synth.rs:54-59): default_config() patch, all voices idle. */
int s2r_create(const s2r_config *cfg, s2r_synth **out);
void s2r_destroy(s2r_synth *s);

/* The `.synth2` patch text (example.synth2:1-3 sketches `synth <ident> { }`; the reference
 * ships no loader — grammar in DESIGN.md).  An empty body == Synth::default_config()
 * (synth.rs:125-152). */
int s2r_load_patch(s2r_synth *s, const char *text, size_t len);
int s2r_set_patch(s2r_synth *s, const s2r_patch *patch);
int s2r_get_patch(const s2r_synth *s, s2r_patch *out);

/* Patch bank ("per-voice patches"; build-defined, the reference has one patch per
 * Synth).  A bank of 1..S2R_MAX_BANK patches; the current program (MIDI program change) selects
 * the patch a note_on gives its voice, and the voice keeps it until it is restarted.
 * s2r_set_patch / s2r_load_patch / s2r_get_patch address patch 0; a fresh handle has a bank of
 * one.  A voice whose program lies past a later, smaller bank renders with patch 0. */
#define S2R_MAX_BANK 256u
int s2r_set_patch_bank(s2r_synth *s, const s2r_patch *patches, uint32_t n);
uint32_t s2r_patch_bank_size(const s2r_synth *s);
int s2r_program_change(s2r_synth *s, uint32_t program);      /* S2R_ERR_INVALID if program >= bank size */
void s2r_default_patch(s2r_patch *out);                      /* synth.rs:125-152 */

/* Synth::note_on(Note, Velocity) (synth.rs:61-70) incl. next_voice (synth.rs:101-120).
 * Optionally reports the chosen pool index. */
int s2r_note_on(s2r_synth *s, uint8_t note, float velocity);
int s2r_note_on_ex(s2r_synth *s, uint8_t note, float velocity, uint32_t *voice_index_out);
/* Synth::note_off(Note) (synth.rs:72-96): last active voice holding `note`. */
int s2r_note_off(s2r_synth *s, uint8_t note);

/* A batch of note_on / note_off calls applied in order — what s2_bin's
 * apply_all_midi_messages loop does between two sample() calls (main.rs:170-187), in one
 * crossing of the boundary.
 *
 * `frame` = 0: the event takes effect before the next fill (like s2r_note_on/off).
 * `frame` = a multiple of 16 below the next fill's length: the event takes effect INSIDE the
 * next fill at that frame, exactly as if the caller had split the fill there — s2_bin's
 * apply-MIDI-every-16-frames loop (main.rs:138-143) reproduced inside one launch.  Events
 * must be submitted in non-decreasing frame order. */
typedef enum { S2R_NOTE_OFF = 0, S2R_NOTE_ON = 1,
               S2R_PROGRAM_CHANGE = 2   /* `note` = patch bank index for the note_ons that follow */
} s2r_note_kind;
typedef struct { uint8_t kind; uint8_t note; uint16_t frame; float velocity; } s2r_note_event;
int s2r_note_events(s2r_synth *s, const s2r_note_event *events, size_t n);

/* Synth::sample(&mut [f32], SampleRateKhz) (synth.rs:154-169).  `sample_rate_hz` is what
 * the reference calls SampleRateKhz but holds Hz (units.rs:14).  Full 16-frame chunks take
 * the x16 code path, a tail of frames % 16 the scalar path, restarting per call
 * (synth.rs:158, process.rs:25-48).  Output = the mix of this handle's shard, root-added to
 * +0.0 (synth.rs:176). */
int s2r_fill(s2r_synth *s, float *mono_out, size_t frames, uint32_t sample_rate_hz);
/* s2r_fill in two halves, for a caller that keeps TWO buffers in flight the way s2_bin does (its synth thread fills one
 * buffer while the audio thread plays the other: audio_player.rs:56-60 pre-sends two, main.rs:135-149 refills whichever
 * comes back).  s2r_fill_begin applies the events handed over so far and queues the fill; s2r_fill_end waits for the
 * OLDEST fill begun and not yet ended and copies its `frames` samples to mono_out.  At most two fills may be in flight;
 * between a begin and its end the caller may hand over the next buffer's events and begin that fill.  s2r_fill is
 * begin + end.  (How a begun fill is launched is the library's business and bit-neutral: ONE handle per device and process —
 * the first created whose grid is at most one workgroup per compute unit — runs its render kernels on a stream of their own
 * beside a second stream's chain heads and mixes, which wait for each other's workgroups inside the kernels and therefore
 * need the device's compute units to themselves; every other handle takes one launch per fill in which no kernel waits for
 * another.  A fill that fails on the device comes back from s2r_fill_end as an error ONCE, its buffer zeroed, and the handle
 * refuses events and fills from then on: DESIGN.md 4.2.) */
int s2r_fill_begin(s2r_synth *s, size_t frames, uint32_t sample_rate_hz);
/* `capacity` = floats `mono_out` can take: S2R_ERR_INVALID (and nothing is consumed) when it is smaller than the
 * `frames` the oldest fill was begun with — s2r_fill_pending_frames says how many that is (0: none in flight). */
int s2r_fill_end(s2r_synth *s, float *mono_out, size_t capacity);
size_t s2r_fill_pending_frames(const s2r_synth *s);
uint32_t s2r_fills_in_flight(const s2r_synth *s);
/* The audio callback's mono -> every channel copy (s2_bin/src/audio_player.rs:224-228),
 * done on device: interleaved L,R with L == R. */
int s2r_fill_stereo(s2r_synth *s, float *interleaved_lr_out, size_t frames, uint32_t sample_rate_hz);

/* BUILD-DEFINED true stereo (the reference has the copy above and nothing else; DESIGN.md 4.12 gives the op sequence).
 * Every program of the bank has a `pan` and a `key_spread`, both in [-1, 1], both 0 by default, held beside the bank (not in
 * s2r_patch).  A note_on gives its voice the pan p = s2r_voice_pan(pan, key_spread, note) of the program current at that
 * note_on — exactly as it gives it its patch — and the voice keeps p until it is restarted; a voice never started has p = 0;
 * changing a program's pan affects later note_ons only.  s2r_set_patch_bank keeps the pans of the programs that survive and
 * gives new ones 0 / 0.
 *   s2r_set_program_pan: S2R_ERR_INVALID if program >= bank size, S2R_ERR_PATCH_RANGE for a value outside [-1, 1] or NaN.
 *   s2r_get_voice_pans / s2r_set_voice_pans: every shard voice's p, shard_voices entries in local order — the companion of
 *   s2r_export_state / s2r_import_state for checkpoint / resume; the setter is range-checked like the program's (nothing is
 *   changed when one entry is refused).  Single-device handles (a device-list handle: S2R_ERR_INVALID).
 *   s2r_fill_panned: s2r_fill with every voice placed in the stereo field.  Synchronous; overwrites 2 * frames floats,
 *   interleaved L, R: channel c of frame i is the mix tree of DESIGN.md 4.3 over x_c[v][i] = row[v][i] * g_c[v] (one rounded
 *   multiply, denormals kept), row = what s2r_render_voices returns and (gL, gR) = s2r_pan_gains(p of voice v).  Like
 *   s2r_fill a handle that renders a shard returns that shard's root-added mix.  Voice state advances exactly as under
 *   s2r_fill; events with a frame inside the fill take effect there (the fill is rendered segment after segment).  The
 *   voices' rows pass through a device buffer allocated ONCE, by the first panned fill, and never per call after that:
 *   shard_voices * min(round_up(max_frames, 16), max(16, round_down(256 MiB / (4 * shard_voices), 16))) floats — at most
 *   256 MiB, which is 65 536 voices x 1024 frames unsliced (16 frames per voice beyond four million voices); a longer fill is
 *   rendered in slices of that many frames.  It stops
 *   resident kernels like every other entry point that touches the device.  Single-device handles without an exchange
 *   attached (S2R_ERR_INVALID otherwise; the handle stays usable). */
int s2r_set_program_pan(s2r_synth *s, uint32_t program, float pan, float key_spread);
int s2r_get_program_pan(const s2r_synth *s, uint32_t program, float *pan, float *key_spread);
int s2r_get_voice_pans(s2r_synth *s, float *pans);
int s2r_set_voice_pans(s2r_synth *s, const float *pans);
int s2r_fill_panned(s2r_synth *s, float *interleaved_lr_out, size_t frames, uint32_t sample_rate_hz);

/* BUILD-DEFINED voice mixer (the reference has neither; DESIGN.md 4.13 gives the op sequence): a level, a velocity sensitivity
 * and an output bus per bank program, and a fill that writes up to S2R_MAX_BUSES stereo buses from one render pass.
 * Every program of the bank has a `level` in [0, 1] (default 1), a `velocity_sens` in [0, 1] (default 0) and a `bus` in
 * [0, S2R_MAX_BUSES) (default 0), held beside the bank like pan / key_spread (not in s2r_patch).  A note_on gives its voice the
 * gain w = s2r_voice_gain(level, velocity_sens, velocity) and the bus of the program current at that note_on (a
 * S2R_PROGRAM_CHANGE inside a batch included; an event inside a fill takes effect at its frame, as its pan does); the voice keeps
 * both until it is restarted; a voice never started has w = 1 and bus 0; changing a program's mix affects later note_ons only (the program FADERS below reach sounding voices).
 * With the defaults w == 1.0f exactly.  s2r_set_patch_bank keeps the values of the programs that survive and gives new ones the
 * defaults.
 * ONLY s2r_fill_buses applies them: s2r_fill, s2r_fill_stereo, s2r_fill_panned, s2r_fill_oversampled, s2r_fill_begin / _end,
 * s2r_fill_device and s2r_render_voices ignore level, velocity and bus and return exactly what they returned before (the
 * reference stores a velocity and never uses it).
 *   s2r_set_program_mix: S2R_ERR_PATCH_RANGE for a level or sensitivity outside [0, 1] or NaN or a bus >= S2R_MAX_BUSES (checked
 *   before the handle is looked at; nothing is changed), S2R_ERR_INVALID if program >= bank size.
 *   s2r_get_voice_mix / s2r_set_voice_mix: every shard voice's w and bus, shard_voices entries each in local order: the
 *   companions of s2r_export_state and s2r_get_voice_pans for checkpoint / resume.  The setter refuses a gain outside [0, 1] or
 *   NaN and a bus >= S2R_MAX_BUSES with S2R_ERR_PATCH_RANGE and changes nothing then.  Single-device handles.
 *   s2r_fill_buses: s2r_fill_panned onto n_buses (1 .. S2R_MAX_BUSES) stereo buses.  Synchronous; overwrites
 *   2 * frames * n_buses floats, bus-major, L, R interleaved inside a bus: out[(b * frames + i) * 2 + c] is the mix tree of
 *   DESIGN.md 4.3 over x[v][i] = row[v][i] * gb_c[v] (one rounded multiply, denormals kept) with
 *   gb_c[v] = (min(bus of v, n_buses - 1) == b) ? s2r_pan_gains(pan of v)_c * w[v] : +0.0f (the product rounded once, on the
 *   host).  A voice booked on a bus >= n_buses sounds on the LAST bus; an off-bus voice is a term with gain +0.0, not a skipped
 *   one (what s2r_fill_panned does at hard left or right).  `capacity` is the number of floats `out` can take: a smaller one
 *   than 2 * frames * n_buses returns S2R_ERR_INVALID and consumes nothing, like n_buses == 0 or > S2R_MAX_BUSES.  State,
 *   events inside the fill, the rows buffer (shared with s2r_fill_panned: allocated by whichever of the two comes first) and
 *   the restrictions are s2r_fill_panned's: single-device handles without an exchange attached, no s2r_fill_begin in flight;
 *   resident kernels are stopped.  The first bus fill also allocates, once, the workgroups' partial rows
 *   (n_blocks * S2R_MAX_BUSES * 2 * slice floats) and a pinned output of 2 * S2R_MAX_BUSES * max_frames floats. */
#define S2R_MAX_BUSES 8u
int s2r_set_program_mix(s2r_synth *s, uint32_t program, float level, float velocity_sens, uint32_t bus);
int s2r_get_program_mix(const s2r_synth *s, uint32_t program, float *level, float *velocity_sens, uint32_t *bus);
int s2r_get_voice_mix(s2r_synth *s, float *gains, uint8_t *buses);
int s2r_set_voice_mix(s2r_synth *s, const float *gains, const uint8_t *buses);
int s2r_fill_buses(s2r_synth *s, float *out, size_t capacity, uint32_t n_buses, size_t frames, uint32_t sample_rate_hz);

/* BUILD-DEFINED live program faders (the reference has none; DESIGN.md 4.14 gives the op sequence): the mixer's channel volume
 * and pan control (MIDI CC7 / CC11 / CC10).  Every program of the bank has a `fader` in [0, 1] (default 1) and a `pan_shift` in
 * [-2, 2] (default 0; 2 takes a hard-left voice hard right), held beside the bank like level / pan, in two copies: the TARGET
 * the caller last set and the APPLIED pair where the last bus fill left it (both (1, 0) on a fresh handle).  They act on every
 * voice SOUNDING on the program — a voice follows the program it was started with (s2r_voice_state.program), not the current
 * one; a voice whose program lies past a later, smaller bank follows program 0, as it renders with patch 0 — and they move as a
 * ramp across ONE s2r_fill_buses call of N frames: with (G0_L, G0_R) = s2r_fader_gains(pan of v, w of v, applied pair) and
 * (G1_L, G1_R) the same under the target pair, d_c = (G1_c - G0_c) / (float)N (IEEE division) and at frame i of the CALL the
 * voice's gain is g_c[v][i] = G0_c + (float)i * d_c (the product rounded, then the sum; no fma), which takes the place of
 * s2r_fill_buses' constant gain: gb_c[v][i] = (min(bus of v, n_buses - 1) == b) ? g_c[v][i] : +0.0f.  A voice whose program did
 * not move has d == +0 and its terms are the static fill's, bit for bit; with every pair at (1, 0) the bus fill is exactly what
 * it was without faders.  When the call returns S2R_OK applied becomes target for every program; a call that fails leaves
 * applied alone.  A note_on inside the fill gives its voice its new program's G0, G1 and d from its frame on; i keeps counting
 * from the start of the call.  ONLY s2r_fill_buses applies or commits faders: every other fill ignores them, s2r_fill_panned
 * included.  s2r_set_patch_bank keeps the pairs of the programs that survive and gives new ones (1, 0).
 *   s2r_set_program_fader sets the target: S2R_ERR_PATCH_RANGE for a value outside its range or NaN (checked before the handle
 *   is looked at; nothing is changed), S2R_ERR_INVALID if program >= bank size.  The first call that leaves (1, 0) reads the
 *   voices' programs back from the device once (resident kernels are stopped).
 *   s2r_get_program_fader: target and applied pair; any pointer may be NULL.
 *   s2r_snap_program_faders: applied = target for every program, now — a hard cut, and the way to restore a checkpoint: set
 *   the applied values, snap, then set the targets.
 *   Single-device handles (a device-list handle: S2R_ERR_INVALID from all three, like s2r_set_voice_mix; it takes no bus fill
 *   either).  A handle with an exchange attached takes them, and refuses the bus fill as before. */
int s2r_set_program_fader(s2r_synth *s, uint32_t program, float fader, float pan_shift);
int s2r_get_program_fader(const s2r_synth *s, uint32_t program, float *fader, float *pan_shift, float *applied_fader, float *applied_pan_shift);
int s2r_snap_program_faders(s2r_synth *s);

/* BUILD-DEFINED aux sends (the reference has none; DESIGN.md 4.15 gives the op sequence): a second, scaled feed from each
 * program to another bus of s2r_fill_buses — "some of the strings, some of the lead" on a bus that the caller's reverb or delay
 * consumes.  Every program of the bank has a `send` in [0, 1] (default 0) and a `send_bus` in [0, S2R_MAX_BUSES) (default 0),
 * held beside the bank like level / bus.  A note_on gives its voice the send s and the send bus sb of the program current at
 * that note_on (a S2R_PROGRAM_CHANGE inside a batch included; an event inside a fill takes effect at its frame, as its gain and
 * bus do); the voice keeps both until it is restarted; a voice never started has s = 0, sb = 0.  s2r_set_patch_bank keeps the
 * values of the programs that survive and gives new ones (0, 0).
 * In s2r_fill_buses, with g_c[v] the voice's gain as above (a_c * w, or (a_c * w) * fader): h_c[v] = g_c[v] * s[v] (one rounded
 * multiply: the send is post-pan and post-fader), and the gain of voice v on bus b is
 *   gb_c[v] = ((min(bus of v, n_buses - 1) == b) ? g_c[v] : +0.0f) + ((min(sb of v, n_buses - 1) == b) ? h_c[v] : +0.0f)
 * (one rounded add): the send bus folds onto the last bus of the call as the main bus does, and a voice whose send lands on its
 * own main bus has the gain g + h there.  With s = 0 gb is the main term bit for bit: a fill whose voices all have send 0 is the
 * fill without sends.  Under moving faders base and step are formed the same way from (G0, G0 * s) and (d, d * s):
 * g[i] = (sel(G0) + sel(G0 * s)) + (float)i * (sel(d) + sel(d * s)); the next fill starts from the static G1 * s, which the last
 * ramp frame approaches up to rounding.  ONLY s2r_fill_buses applies sends; every other fill ignores them.
 *   s2r_set_program_send: S2R_ERR_PATCH_RANGE for a send outside [0, 1] or NaN or a bus >= S2R_MAX_BUSES (checked before the
 *   handle is looked at; nothing is changed), S2R_ERR_INVALID if program >= bank size.
 *   s2r_get_program_send: either pointer may be NULL.
 *   s2r_get_voice_sends / s2r_set_voice_sends: every shard voice's s and sb, shard_voices entries each in local order: the
 *   checkpoint companions of s2r_get_voice_mix / s2r_set_voice_mix.  The setter refuses a send outside [0, 1] or NaN and a bus
 *   >= S2R_MAX_BUSES with S2R_ERR_PATCH_RANGE and changes nothing then.
 *   Single-device handles (a device-list handle: S2R_ERR_INVALID from all four; it takes no bus fill either). */
int s2r_set_program_send(s2r_synth *s, uint32_t program, float send, uint32_t send_bus);
int s2r_get_program_send(const s2r_synth *s, uint32_t program, float *send, uint32_t *send_bus);
int s2r_get_voice_sends(s2r_synth *s, float *sends, uint8_t *send_buses);
int s2r_set_voice_sends(s2r_synth *s, const float *sends, const uint8_t *send_buses);

/* BUILD-DEFINED per-bus convolution reverb (the reference has no effects; DESIGN.md 4.16 gives the op sequence): the effect at the end
 * of the send -> effect -> return chain, computed on the device the bus signal is already on.  A bus b in [0, S2R_MAX_BUSES) may carry
 * a reverb: K taps (1 .. S2R_MAX_IR_TAPS) per channel, ir_l[k] and ir_r[k] (left feeds left, right feeds right; ir_r NULL: ir_l for
 * both), a `dry` and a `wet` in [0, 1], and a history of K - 1 stereo frames that carries from call to call, +0.0 right after the reverb
 * is set.  With x_c[i] what s2r_fill_buses writes for bus b, channel c, frame i of a call of N frames WITHOUT a reverb (the dry signal, bit
 * for bit: the bus combine's, or, on a bus that carries a delay — below —, the delay's output y), h_c[j] (j = 1 .. K - 1) the dry sample j frames before frame 0 of the call, and xs(i - k) = i >= k ? x_c[i - k] : h_c[k - i]:
 *   P_s = ((+0.0 + ir[256 s] * xs(i - 256 s)) + ir[256 s + 1] * xs(i - 256 s - 1)) + ...   for the taps of segment s = 0 .. ceil(K / 256) - 1
 *   in index order (S2R_IR_SEGMENT = 256 taps; the last segment ends at tap K - 1), every product rounded, then every sum;
 *   r = ((+0.0 + P_0) + P_1) + ...;   y = (dry * x_c[i]) + (wet * r)   (two rounded products, one rounded sum; binary32, no fma,
 *   denormals kept) — and y is what the call writes to out[(b * N + i) * 2 + c].  Non-finite bus samples are outside the contract.
 * After a call that returns S2R_OK the history is the last K - 1 frames of (old history, then x_c[0 .. N)): calls of any lengths
 * concatenate.  The reverb runs once per call over all N frames, after every event segment and rows slice of the call has been mixed.  A
 * reverb on a bus >= the call's n_buses is idle in that call (no output, history untouched); voices folded onto the last bus of a call
 * are part of that bus's dry signal.  ONLY s2r_fill_buses applies reverbs; every other fill ignores them.  A reverb is a property of
 * the bus: s2r_set_patch_bank, program changes and s2r_import_state leave it alone.  A s2r_fill_buses call refused before any launch
 * (capacity, bus count, frames) leaves every history untouched.  A handle on which no reverb was ever set launches what it launched
 * before.  Taps, history, the segments' partial sums and a staging buffer for the dry buses live in device memory allocated when a
 * reverb is set (S2R_ERR_OUT_OF_MEMORY when that fails), never inside a fill, and released with the handle.
 *   s2r_set_bus_reverb: replaces any earlier reverb of the bus and zeroes its history; n_taps == 0 removes it (the bus then returns the
 *   dry signal bit for bit, -0.0 included).  S2R_ERR_PATCH_RANGE for a dry or wet outside [0, 1] or NaN, n_taps > S2R_MAX_IR_TAPS,
 *   bus >= S2R_MAX_BUSES or a tap that is not finite (checked before the handle is looked at; nothing is changed); S2R_ERR_INVALID for
 *   a NULL ir_l with n_taps > 0.
 *   s2r_set_bus_reverb_mix: dry and wet alone; taps and history stay.  s2r_get_bus_reverb: n_taps is 0 for a bus without one; any
 *   pointer may be NULL.
 *   s2r_get_bus_reverb_history / s2r_set_bus_reverb_history: the 2 * (K - 1) floats of the history, oldest frame first, L then R inside
 *   a frame: the checkpoint companions of s2r_get_voice_sends / s2r_set_voice_sends.  S2R_ERR_INVALID for a capacity below, or a
 *   count other than, 2 * (K - 1), and — like s2r_set_bus_reverb_mix — on a bus without a reverb.
 *   Single-device handles (a device-list handle: S2R_ERR_INVALID from all five).
 *   s2r_reverb_reference: the rule above for ONE channel on the host (no device, no handle): x_with_history holds K - 1 samples of
 *   history, oldest first, then `frames` dry samples; out receives `frames` samples.  Range checks as above; S2R_ERR_INVALID for a NULL
 *   pointer or n_taps == 0. */
#define S2R_MAX_IR_TAPS 65536u
#define S2R_IR_SEGMENT 256u
int s2r_set_bus_reverb(s2r_synth *s, uint32_t bus, const float *ir_l, const float *ir_r, uint32_t n_taps, float dry, float wet);
int s2r_set_bus_reverb_mix(s2r_synth *s, uint32_t bus, float dry, float wet);
int s2r_get_bus_reverb(const s2r_synth *s, uint32_t bus, uint32_t *n_taps, float *dry, float *wet);
int s2r_get_bus_reverb_history(s2r_synth *s, uint32_t bus, float *lr, size_t capacity);
int s2r_set_bus_reverb_history(s2r_synth *s, uint32_t bus, const float *lr, size_t count);
int s2r_reverb_reference(const float *ir, uint32_t n_taps, const float *x_with_history, uint32_t frames, float dry, float wet, float *out);

/* BUILD-DEFINED per-bus feedback delay with cross-feed ("ping-pong"; the reference has no effects): the other
 * time-based effect of a send bus, computed on the device between the bus combine and the reverbs: combine -> delay -> reverb ->
 * master -> limiter.  A bus b in [0, S2R_MAX_BUSES) may carry a delay: D frames (1 .. S2R_MAX_DELAY_FRAMES), the same for both
 * channels; a `feedback` and a `cross` in [-1, 1] with |feedback| + |cross| <= 1 (evaluated in double from the two floats); a `dry`
 * and a `wet` in [0, 1]; and a history of D stereo frames of the line signal W that carries from call to call, +0.0 right after the
 * delay is set.  With x_c[n] what the bus combine writes for bus b, channel c, frame n of a call of N frames, and W_c[n] for n < 0
 * the history:
 *   t = W_c[n - D]          u = W_(1-c)[n - D]
 *   p = feedback * t        q = cross * u
 *   s = x_c[n] + p          W_c[n] = s + q
 *   y_c[n] = (dry * x_c[n]) + (wet * t)
 * binary32 throughout, every product and every sum rounded on its own (no fma), denormals kept, no add skipped for a zero
 * coefficient: s + q with s = -0.0 and q = +0.0 is +0.0, and the rule says so.  y is the bus's signal from there on: a reverb on the
 * same bus takes y as its dry signal, the stems and the master section see what the reverb, or without one the delay, wrote.
 * Non-finite bus samples are outside the contract.  After a call that returns S2R_OK the history is the last D frames of (old
 * history, then W[0 .. N)): calls of any lengths concatenate.  The delay runs once per call over all N frames, after every event
 * segment and rows slice of the call has been mixed.  A delay on a bus >= the call's n_buses is idle in that call (no output, history
 * untouched).  A bus without a delay passes through bit for bit, -0.0 included.  A refused or failed call leaves every history
 * untouched.  ONLY s2r_fill_buses and s2r_fill_master apply delays; every other fill ignores them.  A delay is a property of the
 * bus: s2r_set_patch_bank, program changes and s2r_import_state leave it alone.  A handle on which no delay was ever set launches
 * what it launched before and allocates nothing for one.  The two copies of the history and a staging buffer for the combined buses
 * live in device memory allocated when a delay is set (S2R_ERR_OUT_OF_MEMORY when that fails, and the earlier delay is kept), never
 * inside a fill, and released with the handle.
 *   s2r_set_bus_delay: replaces any earlier delay of the bus and zeroes its history; delay_frames == 0 removes it (the bus then
 *   returns the combine's signal bit for bit).  S2R_ERR_PATCH_RANGE for a NaN, a value outside its range, |feedback| + |cross| > 1,
 *   delay_frames > S2R_MAX_DELAY_FRAMES or bus >= S2R_MAX_BUSES (checked before the handle is looked at; nothing is changed).
 *   s2r_set_bus_delay_mix: the four levels alone; D and the history stay.  S2R_ERR_INVALID on a bus without a delay.
 *   s2r_get_bus_delay: delay_frames is 0 for a bus without one; any pointer may be NULL.
 *   s2r_get_bus_delay_history / s2r_set_bus_delay_history: the 2 * D floats of the history, oldest frame first, L then R inside a
 *   frame: the checkpoint companions of the reverb's pair.  S2R_ERR_INVALID for a capacity below, or a count other than, 2 * D, and
 *   on a bus without a delay.
 *   Single-device handles (a NULL or a device-list handle: S2R_ERR_INVALID from all five).
 *   s2r_delay_reference: the rule above for BOTH channels on the host (no device, no handle; the cross-feed couples the channels):
 *   x_lr is [frames][2]; history_lr is [delay_frames][2], oldest frame first, and is updated in place to the history after the call;
 *   out_lr, [frames][2], may be NULL.  Range checks as above (and delay_frames >= 1); S2R_ERR_INVALID for a NULL history_lr or a
 *   NULL x_lr with frames > 0. */
#define S2R_MAX_DELAY_FRAMES 262144u
int s2r_set_bus_delay(s2r_synth *s, uint32_t bus, uint32_t delay_frames, float feedback, float cross, float dry, float wet);
int s2r_set_bus_delay_mix(s2r_synth *s, uint32_t bus, float feedback, float cross, float dry, float wet);
int s2r_get_bus_delay(const s2r_synth *s, uint32_t bus, uint32_t *delay_frames, float *feedback, float *cross, float *dry, float *wet);
int s2r_get_bus_delay_history(s2r_synth *s, uint32_t bus, float *lr, size_t capacity);
int s2r_set_bus_delay_history(s2r_synth *s, uint32_t bus, const float *lr, size_t count);
int s2r_delay_reference(uint32_t delay_frames, float feedback, float cross, float dry, float wet, const float *x_lr, uint32_t frames,
                        float *history_lr, float *out_lr);

/* BUILD-DEFINED per-bus chorus (an ensemble: a modulated multi-voice delay; the reference has no effects), computed on
 * the device in front of the bus's delay: combine -> chorus -> delay -> reverb -> master -> limiter.  A bus b in [0, S2R_MAX_BUSES)
 * may carry a chorus: V voices (1 .. S2R_CHORUS_MAX_VOICES); a `base` >= 1 and a `depth` >= 0 in frames, finite, with
 * fl(base + depth) <= S2R_CHORUS_MAX_DELAY (the sum rounded to binary32); a `phase_inc` and a `spread`, any uint32_t, in units of
 * 2^-32 turns: the LFO's step per frame, round(hz * 2^32 / sample_rate), and the right channel's lead over the left; a `dry` and a
 * `wet` in [0, 1].  Its state: a `phase` (uint32_t), and a history of H = floor(fl(base + depth)) + 1 stereo frames of the INPUT;
 * 0 and +0.0 right after the chorus is set.  With x_c[n] what the bus combine writes for bus b, channel c (0 left, 1 right), frame n
 * of a call of N frames, and x_c[n] for n < 0 the history, for voice v = 0 .. V - 1:
 *   off = (uint32)(((uint64)v << 32) / V) + c * spread         (mod 2^32)
 *   p   = phase + off + phase_inc * (uint32)n                  (mod 2^32: uint32 arithmetic throughout)
 *   q   = p >> 8                                               (0 .. 2^24 - 1)
 *   h   = q < 2^23 ? q : 2^24 - q                              (0 .. 2^23: a triangle)
 *   m   = (float)h * 2^-23                                     (exact, in [0, 1])
 *   d   = base + (depth * m)                                   (the product rounded, then the sum)
 *   i   = (uint32)d                                            (d >= 1: truncation is floor)
 *   f   = d - (float)i                                         (exact, in [0, 1))
 *   a   = x_c[n - i]      bb = x_c[n - i - 1]
 *   e   = bb - a          g = f * e          tap_v = a + g
 * then acc = tap_0, acc = acc + tap_v in voice order, and y_c[n] = (dry * x_c[n]) + (wet * acc): binary32 throughout, every product
 * and every sum rounded on its own (no fma), denormals kept, no operation skipped for a zero coefficient or for f == 0 (a + g may
 * turn a -0.0 into +0.0, and the rule says so).  1 / V is the caller's business: it goes into `wet`.  Rounding is monotonic, so
 * depth * m <= depth, d <= fl(base + depth) and i + 1 <= H: no tap leaves the history.  Non-finite bus samples are outside the
 * contract.  After a call that returns S2R_OK the history is the last H frames of (old history, then x[0 .. N)) and the phase is
 * phase + phase_inc * N (mod 2^32): calls of any lengths concatenate.  y is the bus's signal from there on: a delay on the same bus
 * takes it as its x, otherwise a reverb as its dry signal, otherwise the stems and the master section.  The chorus runs once per
 * call over all N frames, after every event segment and rows slice of the call has been mixed.  A chorus on a bus >= the call's
 * n_buses is idle in that call (no output, state untouched).  A bus without a chorus passes through bit for bit, -0.0 included.  A
 * refused or failed call leaves history and phase untouched.  ONLY s2r_fill_buses and s2r_fill_master apply choruses; every other
 * fill ignores them.  A chorus is a property of the bus: s2r_set_patch_bank, program changes and s2r_import_state leave it alone.  A
 * handle on which no chorus was ever set launches what it launched before and allocates nothing for one.  The two copies of the
 * history and a staging buffer for the combined buses live in device memory allocated when a chorus is set (S2R_ERR_OUT_OF_MEMORY
 * when that fails, and the earlier chorus is kept), never inside a fill, and released with the handle.
 *   s2r_chorus_history_frames: H for a (base, depth) in range, 0 otherwise; needs no handle.
 *   s2r_set_bus_chorus: replaces any earlier chorus of the bus, zeroes its history and its phase; voices == 0 removes it (the other
 *   values are then not looked at).  S2R_ERR_PATCH_RANGE for a NaN, a value outside its range, voices > S2R_CHORUS_MAX_VOICES or
 *   bus >= S2R_MAX_BUSES (checked before the handle is looked at; nothing is changed).
 *   s2r_set_bus_chorus_mix: dry and wet alone.  s2r_set_bus_chorus_rate: phase_inc and spread alone — the phase and the history stay,
 *   so the LFO bends without a click.  S2R_ERR_INVALID on a bus without a chorus.
 *   s2r_get_bus_chorus: voices is 0 for a bus without one; any pointer may be NULL.
 *   s2r_get_bus_chorus_state / s2r_set_bus_chorus_state: the 2 * H floats of the history, oldest frame first, L then R inside a
 *   frame, and the phase: the checkpoint companions of the delay's pair.  S2R_ERR_INVALID for a capacity below, or a count other
 *   than, 2 * H, a NULL lr, and on a bus without a chorus; `phase` may be NULL in the getter.
 *   Single-device handles (a NULL or a device-list handle: S2R_ERR_INVALID from all six).
 *   s2r_chorus_reference: the rule above for both channels on the host (no device, no handle): x_lr is [frames][2]; history_lr is
 *   [H][2], oldest frame first, and *phase the phase: both are updated in place to the state after the call; out_lr, [frames][2], may
 *   be NULL.  Range checks as above (and voices >= 1); S2R_ERR_INVALID for a NULL history_lr or phase, or a NULL x_lr with frames > 0. */
#define S2R_CHORUS_MAX_VOICES 8u
#define S2R_CHORUS_MAX_DELAY  4095.0f
uint32_t s2r_chorus_history_frames(float base, float depth);
int s2r_set_bus_chorus(s2r_synth *s, uint32_t bus, uint32_t voices, float base, float depth, uint32_t phase_inc, uint32_t spread, float dry,
                       float wet);
int s2r_set_bus_chorus_mix(s2r_synth *s, uint32_t bus, float dry, float wet);
int s2r_set_bus_chorus_rate(s2r_synth *s, uint32_t bus, uint32_t phase_inc, uint32_t spread);
int s2r_get_bus_chorus(const s2r_synth *s, uint32_t bus, uint32_t *voices, float *base, float *depth, uint32_t *phase_inc, uint32_t *spread,
                       float *dry, float *wet);
int s2r_get_bus_chorus_state(s2r_synth *s, uint32_t bus, float *lr, size_t capacity, uint32_t *phase);
int s2r_set_bus_chorus_state(s2r_synth *s, uint32_t bus, const float *lr, size_t count, uint32_t phase);
int s2r_chorus_reference(uint32_t voices, float base, float depth, uint32_t phase_inc, uint32_t spread, float dry, float wet, const float *x_lr,
                         uint32_t frames, float *history_lr, uint32_t *phase, float *out_lr);

/* BUILD-DEFINED per-bus parametric equaliser (the reference has no effects), computed on the device at the head of
 * the chain: combine -> eq -> chorus -> delay -> reverb -> master -> limiter.  A bus b in [0, S2R_MAX_BUSES) may carry an EQ of
 * n_bands (1 .. S2R_EQ_MAX_BANDS) biquad bands, cascaded in band order.  A band is five binary32 coefficients (b0, b1, b2, a1, a2),
 * already divided by a0, all finite, inside the stability triangle: |a2| < 1 and |a1| < 1 + a2, evaluated in binary64 from the
 * binary32 values.  Both channels use the same coefficients.  The state is (s1, s2) per band and channel, 4 * n_bands floats per bus,
 * laid out [band][s1_L, s1_R, s2_L, s2_R]; +0.0 right after the EQ is set.  Transposed direct form II: per channel c and band k, with
 * x the previous band's y at the same frame (for band 0: what the bus combine writes for bus b, channel c):
 *   y   = fl(fl(b0 * x) + s1)
 *   s1' = fl(fl(fl(b1 * x) - fl(a1 * y)) + s2)
 *   s2' = fl(fl(b2 * x) - fl(a2 * y))
 * binary32 throughout, every product and every sum rounded on its own (no fma), denormals kept, no operation skipped for a zero
 * coefficient.  The last band's y is the bus's signal from there on: a chorus on the same bus takes it as its x, otherwise a delay,
 * otherwise a reverb as its dry signal, otherwise the stems and the master section.  Non-finite bus samples are outside the
 * contract.  After a call that returns S2R_OK the state is what the last frame left: calls of any lengths concatenate.  The EQ runs
 * once per call over all N frames, after every event segment and rows slice of the call has been mixed.  An EQ on a bus >= the
 * call's n_buses is idle in that call (no output, state untouched).  A bus without an EQ passes through bit for bit, -0.0 included;
 * a unit band (1, 0, 0, 0, 0) does NOT: y = fl(x + s1) with s1 = +0.0 turns a -0.0 into +0.0, and the rule says so.  A refused or
 * failed call leaves the state untouched.  ONLY s2r_fill_buses and s2r_fill_master apply EQs; every other fill ignores them.  An EQ
 * is a property of the bus: s2r_set_patch_bank, program changes and s2r_import_state leave it alone.  A handle on which no EQ was
 * ever set launches what it launched before and allocates nothing for one.  The two copies of the state and a staging buffer for the
 * combined buses live in device memory allocated when an EQ is set (S2R_ERR_OUT_OF_MEMORY when that fails, and the earlier EQ is
 * kept), never inside a fill, and released with the handle.
 *   s2r_set_bus_eq: coeffs is [n_bands][5]; replaces any earlier EQ of the bus and zeroes its state; n_bands == 0 removes it (coeffs
 *   is then not looked at).  S2R_ERR_PATCH_RANGE for bus >= S2R_MAX_BUSES, n_bands > S2R_EQ_MAX_BANDS, a coefficient that is not
 *   finite or a band outside the stability triangle (checked before the handle is looked at; nothing is changed); S2R_ERR_INVALID
 *   for a NULL coeffs with n_bands > 0.
 *   s2r_set_bus_eq_coeffs: the coefficients alone — the state stays, so a band moves between calls without a restart.  The same
 *   range checks; S2R_ERR_INVALID on a bus without an EQ or when n_bands is not the EQ's.
 *   s2r_get_bus_eq: *n_bands is 0 for a bus without one; coeffs receives 5 * n_bands floats when it is not NULL (S2R_ERR_INVALID
 *   for a capacity below that); n_bands may be NULL.
 *   s2r_get_bus_eq_state / s2r_set_bus_eq_state: the 4 * n_bands floats of the state: the checkpoint companions of the chorus's
 *   pair.  S2R_ERR_INVALID for a capacity below, or a count other than, 4 * n_bands, a NULL buffer, and on a bus without an EQ.
 *   Single-device handles (a NULL or a device-list handle: S2R_ERR_INVALID from all five).
 *   s2r_eq_reference: the rule above for both channels on the host (no device, no handle): x_lr is [frames][2]; state is
 *   [n_bands][4] as above, updated in place to the state after the call; out_lr, [frames][2], may be NULL.  Range checks as above
 *   (and n_bands >= 1); S2R_ERR_INVALID for a NULL coeffs or state, or a NULL x_lr with frames > 0.
 *   s2r_eq_design: a band from the usual parameters, by the Audio-EQ-Cookbook (R. Bristow-Johnson) formulas with q as Q (DESIGN.md
 *   4.21 writes them out): computed in binary64, divided by a0, then rounded once to binary32.  gain_db is looked at by the peak and
 *   the shelves only (but must not be a NaN).  S2R_ERR_PATCH_RANGE for a NaN, a kind that is none of the five, freq_hz outside
 *   (0, sample_rate / 2), q <= 0, |gain_db| > 48 or a result that fails the setter's checks; S2R_ERR_INVALID for a NULL coeffs.
 *   Device parity is always against the stored binary32 coefficients, never against this function. */
#define S2R_EQ_MAX_BANDS 4u
typedef enum { S2R_EQ_PEAK = 0, S2R_EQ_LOW_SHELF = 1, S2R_EQ_HIGH_SHELF = 2, S2R_EQ_LOWPASS = 3, S2R_EQ_HIGHPASS = 4 } s2r_eq_kind;
int s2r_set_bus_eq(s2r_synth *s, uint32_t bus, uint32_t n_bands, const float *coeffs);
int s2r_set_bus_eq_coeffs(s2r_synth *s, uint32_t bus, uint32_t n_bands, const float *coeffs);
int s2r_get_bus_eq(const s2r_synth *s, uint32_t bus, uint32_t *n_bands, float *coeffs, size_t capacity);
int s2r_get_bus_eq_state(s2r_synth *s, uint32_t bus, float *state, size_t capacity);
int s2r_set_bus_eq_state(s2r_synth *s, uint32_t bus, const float *state, size_t count);
int s2r_eq_reference(uint32_t n_bands, const float *coeffs, const float *x_lr, uint32_t frames, float *state, float *out_lr);
int s2r_eq_design(int kind, double freq_hz, double gain_db, double q, double sample_rate, float coeffs[5]);

/* BUILD-DEFINED per-bus dynamics (the reference has no effects): a sidechain compressor behind the bus's EQ, computed on
 * the device: combine -> eq -> dynamics -> chorus -> delay -> reverb -> master -> limiter.  A bus b in [0, S2R_MAX_BUSES) may carry
 * dynamics: a key bus k in [0, S2R_MAX_BUSES) (k == b: the ordinary compressor; k != b: a ducker, an external sidechain), a transfer
 * curve of S2R_DYN_CURVE_POINTS gains — 32 octaves of level from 2^-24 to 2^8, 16 linear segments each, and the end point: breakpoint
 * j sits at the level 2^(-24 + j / 16) * (1 + (j mod 16) / 16), integer division — and two retention coefficients a_att and a_rel in
 * [0, 1).  The state is one gain y per bus, both channels linked: curve[0], the gain at silence, right after a set.  With x_b the
 * bus's and x_k the key bus's signal, both as they ENTER the dynamics stage (behind the EQs, in front of every bus's dynamics,
 * whatever the key bus itself carries), for frame n:
 *   p = max(|x_kL[n]|, |x_kR[n]|)
 *   t = curve[0] if p < 2^-24; curve[512] if p >= 2^8; otherwise, with u the bits of p and lo the bits of 2^-24,
 *       i = (u - lo) >> 19, f = (float)((u - lo) & 0x7ffff) * 2^-19 (both exact), t = fl(curve[i] + fl(f * fl(curve[i + 1] - curve[i])))
 *   a = (t < y) ? a_att : a_rel;   y = fl(t + fl(a * fl(y - t)))
 *   out_c[n] = fl(x_bc[n] * y) for both channels
 * binary32 throughout, every operation rounded on its own (no fma), denormals kept, nothing skipped for a zero.  No transcendental
 * function: the curve holds gains, makeup included.  With a == 0 the new y is t exactly.  From a finite y >= 0 the rule keeps y >= 0
 * (every curve entry is >= 0 and a < 1).  The meter of a call is min over n of y[n], the gain reduction a compressor shows.
 * Non-finite bus samples are outside the contract.  After a call that returns S2R_OK the state is what the last frame left: calls
 * of any lengths concatenate.  The stage runs once per call over all N frames, after every event segment and rows slice has been
 * mixed.  Dynamics whose bus OR key bus is >= the call's n_buses are idle in that call: the bus passes, the state stays.  A bus
 * without dynamics passes bit for bit, -0.0 included.  A refused or failed call leaves the state untouched.  ONLY s2r_fill_buses
 * and s2r_fill_master apply dynamics; s2r_set_patch_bank, program changes and s2r_import_state leave them alone.  A handle on which
 * none were ever set launches what it launched before and allocates nothing for them; device memory is allocated when dynamics are
 * set (S2R_ERR_OUT_OF_MEMORY when that fails, and the earlier dynamics are kept), never inside a fill.
 *   s2r_set_bus_dynamics: replaces any earlier dynamics of the bus and resets y to curve[0].  S2R_ERR_PATCH_RANGE for a bus or a key
 *   >= S2R_MAX_BUSES, a curve entry that is not finite or outside [0, 2^8], a coefficient outside [0, 1) or a NaN (checked before
 *   the handle is looked at; nothing is changed); S2R_ERR_INVALID for a NULL curve.
 *   s2r_clear_bus_dynamics removes them (S2R_OK on a bus without).
 *   s2r_set_bus_dynamics_params: the same arguments, y stays: a threshold moves between calls without a restart.  S2R_ERR_INVALID
 *   on a bus without dynamics.
 *   s2r_get_bus_dynamics: *present is 0 for a bus without; curve receives S2R_DYN_CURVE_POINTS floats when it is not NULL
 *   (S2R_ERR_INVALID for a capacity below that); any pointer may be NULL.
 *   s2r_get_bus_dynamics_state / s2r_set_bus_dynamics_state: the one float y.  S2R_ERR_INVALID for a capacity below, or a count
 *   other than, 1, a NULL buffer, and on a bus without dynamics; S2R_ERR_PATCH_RANGE for a y to restore that is not finite or < 0.
 *   s2r_get_bus_dynamics_meter: the minimum of y over the last successful call in which the bus's dynamics ran; 1.0 before any.
 *   Single-device handles (a NULL or a device-list handle: S2R_ERR_INVALID from all seven).
 *   s2r_dynamics_reference: the rule on the host (no device, no handle): key_lr and x_lr are [frames][2]; a NULL key_lr keys the
 *   bus by itself; *y is updated in place; out_lr, [frames][2], and min_gain may be NULL; *min_gain is written when frames > 0.
 *   Range checks as above, and of *y as the state setter's; S2R_ERR_INVALID for a NULL curve or y, or a NULL x_lr with frames > 0.
 *   s2r_dynamics_curve: the table of a soft-knee compressor, in binary64: at each breakpoint level l_j, with L = 20 log10(l_j),
 *   o = L - threshold_db and W = knee_db: G = 0 when 2 o < -W; G = (1 / ratio - 1) (o + W / 2)^2 / (2 W) when W > 0 and 2 |o| <= W;
 *   G = (1 / ratio - 1) o otherwise; the entry is 10^((G + makeup_db) / 20) rounded once to binary32.  ratio in [1, inf], inf the
 *   limiter's curve.  S2R_ERR_PATCH_RANGE for a NaN, ratio < 1, knee_db < 0 or an entry the setter would refuse; S2R_ERR_INVALID
 *   for a NULL curve.  Expanders and gates are curves the caller supplies.
 *   s2r_dynamics_coef: (float)exp(-1 / (ms * 0.001 * sample_rate)), 0 for ms == 0; a NaN for ms < 0, sample_rate <= 0 or a NaN.
 *   Device parity is always against the stored table and coefficients, never against the two design functions. */
#define S2R_DYN_CURVE_POINTS 513u
int s2r_set_bus_dynamics(s2r_synth *s, uint32_t bus, uint32_t key_bus, const float *curve, float a_att, float a_rel);
int s2r_clear_bus_dynamics(s2r_synth *s, uint32_t bus);
int s2r_set_bus_dynamics_params(s2r_synth *s, uint32_t bus, uint32_t key_bus, const float *curve, float a_att, float a_rel);
int s2r_get_bus_dynamics(const s2r_synth *s, uint32_t bus, uint32_t *present, uint32_t *key_bus, float *curve, size_t capacity, float *a_att, float *a_rel);
int s2r_get_bus_dynamics_state(s2r_synth *s, uint32_t bus, float *state, size_t capacity);
int s2r_set_bus_dynamics_state(s2r_synth *s, uint32_t bus, const float *state, size_t count);
int s2r_get_bus_dynamics_meter(const s2r_synth *s, uint32_t bus, float *min_gain);
int s2r_dynamics_reference(const float *curve, float a_att, float a_rel, const float *key_lr, const float *x_lr, uint32_t frames, float *y, float *out_lr,
                           float *min_gain);
int s2r_dynamics_curve(double threshold_db, double ratio, double knee_db, double makeup_db, float *curve);
float s2r_dynamics_coef(double ms, double sample_rate);

/* BUILD-DEFINED per-bus room reverb (the reference has no effects): the algorithmic reverb of Schroeder and Moorer in
 * the form Freeverb made standard — eight parallel feedback combs with a one-pole low-pass in the loop, then four allpasses in
 * series —, computed on the device as the last stem writer:
 * combine -> eq -> dynamics -> chorus -> delay -> reverb -> room -> master -> limiter.  A bus b in [0, S2R_MAX_BUSES) may carry a
 * room: comb delays cd[S2R_ROOM_COMBS], allpass delays ad[S2R_ROOM_ALLPASSES] and a spread, all in frames — the right channel's lines
 * are `spread` frames longer than the left's, D_Li = cd[i], D_Ri = cd[i] + spread, E_Lj = ad[j], E_Rj = ad[j] + spread, every one of
 * them in [S2R_ROOM_MIN_DELAY, S2R_ROOM_MAX_DELAY] —, feedback in [0, 1), damp in [0, 1], g in (-1, 1), gain, dry, wet and cross in
 * [0, 1]; d1 = fl(1 - damp), computed once at the set.  State, all +0.0 right after a set: per channel c and comb i a line C_ci of
 * D_ci frames and one filter value f_ci; per channel and allpass j a line A_cj of E_cj frames.  For frame n of a call of N frames,
 * with x the bus as it enters the stage (negative indices are history):
 *   in = fl(fl(xL[n] + xR[n]) * gain)
 *   per channel c:  acc = +0.0
 *     for i = 0..7:   o = C_ci[n - D_ci];  f_ci = fl(fl(o * d1) + fl(f_ci * damp));  C_ci[n] = fl(in + fl(f_ci * feedback));  acc = fl(acc + o)
 *     for j = 0..3:   b = A_cj[n - E_cj];  y = fl(b - acc);  A_cj[n] = fl(acc + fl(b * g));  acc = y
 *     v_c = acc
 *   out_c[n] = fl(fl(dry * x_c[n]) + fl(fl(wet * v_c) + fl(cross * v_(1-c))))
 * binary32 throughout, every operation rounded on its own (no fma), denormals kept, nothing skipped for a zero coefficient.  The rule
 * claims no bound on the output: feedback < 1 keeps every loop's gain under one in exact arithmetic, and no more is claimed.
 * Non-finite bus samples are outside the contract.  After a call that returns S2R_OK each line holds its last D frames and each f its
 * last value: calls of any lengths concatenate.  The stage runs once per call over all N frames, after every event segment and rows
 * slice has been mixed.  A room on a bus >= the call's n_buses is idle in that call, its state untouched.  A bus without a room
 * passes bit for bit, -0.0 included.  A refused or failed call leaves the state where it was.  ONLY s2r_fill_buses and
 * s2r_fill_master apply it.  A handle on which none was ever set launches what it launched before and allocates nothing for it;
 * device memory is allocated when a room is set (S2R_ERR_OUT_OF_MEMORY when that fails, and the earlier room is kept), never in a fill.
 * The state as one flat float array (the checkpoint): for c = L, R: for each comb its line, oldest frame first, and then its f; then
 * for each allpass its line.  s2r_room_state_floats gives the count: 2 * (sum cd + sum ad + 8) + 12 * spread; 0 out of range.
 *   s2r_set_bus_room: replaces any earlier room of the bus and zeroes the state.  S2R_ERR_PATCH_RANGE for a bus >= S2R_MAX_BUSES, a
 *   delay or a level outside its range or a NaN (checked before the handle is looked at; nothing is changed); S2R_ERR_INVALID for a
 *   NULL cd or ad.
 *   s2r_clear_bus_room removes it (S2R_OK on a bus without).
 *   s2r_set_bus_room_params: the seven levels alone; delays and state stay, so room size (feedback) and damping move between calls
 *   with no restart.  S2R_ERR_INVALID on a bus without a room.
 *   s2r_get_bus_room: *present is 0 for a bus without; cd and ad receive 8 and 4 delays, levels[7] receives feedback, damp, g, gain,
 *   dry, wet, cross; any pointer may be NULL.
 *   s2r_get_bus_room_state / s2r_set_bus_room_state: the flat array above.  S2R_ERR_INVALID for a capacity below, or a count other
 *   than, s2r_room_state_floats, a NULL buffer, and on a bus without a room; S2R_ERR_PATCH_RANGE for a value to restore that is not
 *   finite.
 *   Single-device handles (a NULL or a device-list handle: S2R_ERR_INVALID from all six).
 *   s2r_room_reference: the rule on the host (no device, no handle): x_lr and out_lr are [frames][2]; state, the flat array, is
 *   updated in place; out_lr may be NULL.  Range checks as above, and of the state as the state setter's; S2R_ERR_INVALID for a NULL
 *   cd, ad or state, or a NULL x_lr with frames > 0.
 *   s2r_room_design: the public Freeverb tunings — combs 1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617; allpasses 556, 441, 341,
 *   225; spread 23, at 44.1 kHz — each times sample_rate / 44100 * size in binary64, rounded to nearest.  S2R_ERR_PATCH_RANGE when a
 *   result leaves the range or an argument is not a finite number > 0; S2R_ERR_INVALID for a NULL pointer.  Device parity is always
 *   against the stored delays, never against this function. */
#define S2R_ROOM_COMBS 8u
#define S2R_ROOM_ALLPASSES 4u
#define S2R_ROOM_MIN_DELAY 64u
#define S2R_ROOM_MAX_DELAY 8192u
int s2r_set_bus_room(s2r_synth *s, uint32_t bus, const uint32_t *cd, const uint32_t *ad, uint32_t spread, float feedback, float damp, float g, float gain,
                     float dry, float wet, float cross);
int s2r_clear_bus_room(s2r_synth *s, uint32_t bus);
int s2r_set_bus_room_params(s2r_synth *s, uint32_t bus, float feedback, float damp, float g, float gain, float dry, float wet, float cross);
int s2r_get_bus_room(const s2r_synth *s, uint32_t bus, uint32_t *present, uint32_t *cd, uint32_t *ad, uint32_t *spread, float *levels);
int s2r_get_bus_room_state(s2r_synth *s, uint32_t bus, float *state, size_t capacity);
int s2r_set_bus_room_state(s2r_synth *s, uint32_t bus, const float *state, size_t count);
size_t s2r_room_state_floats(const uint32_t *cd, const uint32_t *ad, uint32_t spread);
int s2r_room_reference(const uint32_t *cd, const uint32_t *ad, uint32_t spread, float feedback, float damp, float g, float gain, float dry, float wet,
                       float cross, const float *x_lr, uint32_t frames, float *state, float *out_lr);
int s2r_room_design(double sample_rate, double size, uint32_t *cd, uint32_t *ad, uint32_t *spread);

/* BUILD-DEFINED per-bus drive (the reference has no effects): a waveshaper — overdrive, saturation, a clipper, a
 * wavefolder — behind the dynamics, oversampled so that the harmonics it makes above the bus rate's Nyquist do not fold back:
 * combine -> eq -> dynamics -> drive -> chorus -> delay -> reverb -> room -> master -> limiter.  The bus goes up to
 * S2R_DRIVE_OVERSAMPLE = 4 times its rate through the interpolator g, through a table there, and back down through the decimator h.
 * h[0 .. 64] is the library's one prototype, S2R_DRIVE_TAPS = 65 taps: the design of s2r_fill_oversampled's decimator — a
 * Blackman-windowed sinc, cutoff 0.115 cycles per oversampled sample, unit DC gain, computed in binary64 and rounded once — and
 * symmetric on bits; s2r_drive_taps reports it; g[k] = 4 h[k], exact.  The two filters' delays add up to 64 oversampled samples:
 * S2R_DRIVE_LATENCY = 16 frames.  A bus b in [0, S2R_MAX_BUSES) may carry a drive: a table curve[S2R_DRIVE_CURVE_POINTS = 1025], finite
 * — entry 512 is the curve's value at 0, entry 512 +- i its value at +- i / 512 —, pre in [0, S2R_DRIVE_MAX_PRE], dry and wet in
 * [0, 1].  State: the bus's last S2R_DRIVE_HISTORY = 32 input frames, [32][2], oldest first, L then R, +0.0 right after a set.  For
 * frame n of a call and channel c, with x the bus as it enters the stage (negative indices are history), every sum from +0.0 in the
 * index order written:
 *   m = 4 q + p, p = 0..3:   u[m] = sum over j = 0.. while p + 4 j <= 64 of  fl(g[p + 4 j] * x_c[q - j])
 *   t = fl(pre * u[m]);  a = fl(min(|t|, 1) * 512);  i = min((uint32)a, 511);  fr = fl(a - (float)i)
 *   s = (t < 0) ? -1 : +1;  c0 = curve[512 + s * i];  c1 = curve[512 + s * (i + 1)]
 *   w[m] = fl(c0 + fl(fr * fl(c1 - c0)))
 *   v[n] = sum over k = 0..64 of fl(h[k] * w[4 n - k])
 *   out_c[n] = fl(fl(dry * x_c[n - 16]) + fl(wet * v[n]))
 * binary32 throughout, every operation rounded on its own (no fma), denormals kept, nothing skipped for a zero coefficient.
 * Non-finite bus samples are outside the contract.  The table is indexed by sign and magnitude, so that a small signal keeps its
 * relative precision.  v[n] reads w[4 n - 64 .. 4 n], that is x[n - 32 .. n]: a frame depends on 33 input frames and on nothing the
 * stage wrote.  The dry path is delayed by S2R_DRIVE_LATENCY with the wet: a bus with a drive is 16 frames late against a bus without
 * one, and nothing compensates the others.  After a call that returns S2R_OK the state is the last 32 frames of history ++ call: calls
 * of any lengths concatenate.  The stage runs once per call over all its frames, after every event segment and rows slice has been
 * mixed.  A drive on a bus >= the call's n_buses is idle in that call, its state untouched.  A bus without a drive passes bit for bit,
 * -0.0 included.  A refused or failed call leaves the state where it was.  ONLY s2r_fill_buses and s2r_fill_master apply it.  A handle
 * on which none was ever set launches what it launched before and allocates nothing for it; device memory is allocated when a drive is
 * set (S2R_ERR_OUT_OF_MEMORY when that fails, and the earlier drive is kept), never in a fill.
 *   s2r_set_bus_drive: replaces any earlier drive of the bus and zeroes the history.  S2R_ERR_PATCH_RANGE for a bus >= S2R_MAX_BUSES,
 *   a level outside its range, a NaN or a table entry that is not finite (checked before the handle is looked at; nothing is
 *   changed); S2R_ERR_INVALID for a NULL curve.
 *   s2r_clear_bus_drive removes it (S2R_OK on a bus without).
 *   s2r_set_bus_drive_params: the levels, and the table unless curve is NULL; the history stays, so a curve or a level moves between
 *   calls with no restart.  S2R_ERR_INVALID on a bus without a drive.
 *   s2r_get_bus_drive: *present is 0 for a bus without; curve, when not NULL, receives the table (S2R_ERR_INVALID for a capacity
 *   below S2R_DRIVE_CURVE_POINTS on a bus with a drive); any pointer may be NULL.
 *   s2r_get_bus_drive_history / s2r_set_bus_drive_history: the state above, 64 floats.  S2R_ERR_INVALID for a capacity below, or a
 *   count other than, 64, a NULL buffer, and on a bus without a drive; S2R_ERR_PATCH_RANGE for a value to restore that is not finite.
 *   Single-device handles (a NULL or a device-list handle: S2R_ERR_INVALID from all six).
 *   s2r_drive_reference: the rule on the host (no device, no handle): x_lr and out_lr are [frames][2]; history, [32][2], is updated in
 *   place; out_lr may be NULL.  Range checks as above, and of the history as its setter's; S2R_ERR_INVALID for a NULL curve or
 *   history, or a NULL x_lr with frames > 0.
 *   s2r_drive_taps: h[65].  S2R_ERR_INVALID for NULL.
 *   s2r_drive_curve: a table by design, with u = i / 512 - 1, in binary64 and rounded once — S2R_DRIVE_LINEAR: u, exact, whatever the
 *   amount; S2R_DRIVE_TANH: tanh(a u) / tanh(a); S2R_DRIVE_HARD: clamp(a u) to [-1, 1]; S2R_DRIVE_CUBIC: 1.5 v - 0.5 v^3 with v =
 *   clamp(a u); S2R_DRIVE_FOLD: the triangle of period 4 and height 1 through 0 at a u, 1 - |((a u + 1) mod 4) - 2|, the mod in [0, 4).
 *   S2R_ERR_PATCH_RANGE for another kind or, but for the linear kind, an amount outside [S2R_DRIVE_MIN_AMOUNT, S2R_DRIVE_MAX_AMOUNT]
 *   or a NaN; S2R_ERR_INVALID for a NULL table.  tanh is the host's.  Device parity is always against the stored table, never against
 *   this function. */
#define S2R_DRIVE_OVERSAMPLE 4u
#define S2R_DRIVE_TAPS 65u
#define S2R_DRIVE_LATENCY 16u
#define S2R_DRIVE_HISTORY 32u
#define S2R_DRIVE_CURVE_POINTS 1025u
#define S2R_DRIVE_MAX_PRE 1024.0f
#define S2R_DRIVE_MIN_AMOUNT 0.015625
#define S2R_DRIVE_MAX_AMOUNT 64.0
typedef enum { S2R_DRIVE_LINEAR = 0, S2R_DRIVE_TANH = 1, S2R_DRIVE_HARD = 2, S2R_DRIVE_CUBIC = 3, S2R_DRIVE_FOLD = 4 } s2r_drive_kind;
int s2r_set_bus_drive(s2r_synth *s, uint32_t bus, const float *curve, float pre, float dry, float wet);
int s2r_clear_bus_drive(s2r_synth *s, uint32_t bus);
int s2r_set_bus_drive_params(s2r_synth *s, uint32_t bus, const float *curve, float pre, float dry, float wet);
int s2r_get_bus_drive(const s2r_synth *s, uint32_t bus, uint32_t *present, float *curve, size_t capacity, float *pre, float *dry, float *wet);
int s2r_get_bus_drive_history(s2r_synth *s, uint32_t bus, float *lr, size_t capacity);
int s2r_set_bus_drive_history(s2r_synth *s, uint32_t bus, const float *lr, size_t count);
int s2r_drive_reference(const float *curve, float pre, float dry, float wet, const float *x_lr, uint32_t frames, float *history, float *out_lr);
int s2r_drive_taps(float *h);
int s2r_drive_curve(uint32_t kind, double amount, float *table);

/* BUILD-DEFINED per-bus flanger (the reference has no effects): a modulated feedback comb — one tap at a
 * triangle-modulated fractional delay into the stage's OWN line signal, fed back — behind the drive and in front of the chorus:
 * combine -> eq -> dynamics -> drive -> flanger -> chorus -> delay -> reverb -> room -> master -> limiter.  A bus b in
 * [0, S2R_MAX_BUSES) may carry a flanger: a `base` and a `depth` in frames, finite, with base >= S2R_FLANGER_MIN_DELAY = 32,
 * depth >= 0 and fl(base + depth) <= S2R_FLANGER_MAX_DELAY = 4095 (the sum rounded to binary32); a `phase_inc` and a `spread`, any
 * uint32_t, in 2^-32 turns — the LFO's step per frame and the right channel's lead, the chorus's units (s2r_set_bus_chorus); a
 * `feedback` and a `cross`, each in [-1, 1], with |feedback| + |cross| <= 1 (in double, from the two floats, as the bus delay's);
 * a `dry` and a `wet` in [0, 1].  State: a `phase` (uint32_t) and a history of H = floor(fl(base + depth)) + 1 stereo frames of the
 * line signal w — not of the input —, oldest frame first, L then R; 0 and +0.0 right after a set.  With x_c[n] what the stage in front
 * writes for channel c (0 left, 1 right), frame n of a call of N frames, and w_c[n] for n < 0 the history, per frame, first for both
 * channels
 *   p    = phase + c * spread + phase_inc * (uint32)n        (mod 2^32)
 *   q    = p >> 8;   h = q < 2^23 ? q : 2^24 - q;   m = (float)h * 2^-23         (exact: the chorus's triangle)
 *   d    = fl(base + fl(depth * m))
 *   i    = (uint32)d;   f = d - (float)i                      (32 <= i <= H - 1; f exact, in [0, 1))
 *   a    = w_c[n - i];   bb = w_c[n - i - 1];   tap_c = fl(a + fl(f * fl(bb - a)))
 * then for both channels
 *   w_c[n] = fl(x_c[n] + fl(fl(feedback * tap_c) + fl(cross * tap_(1-c))))
 *   y_c[n] = fl(fl(dry * x_c[n]) + fl(wet * tap_c))
 * binary32 throughout, every product and sum rounded on its own (no fma), denormals kept, nothing skipped for a zero coefficient or
 * for f == 0.  Non-finite bus samples are outside the contract.  No tap leaves the history (d <= fl(base + depth) by monotonic
 * rounding, so i <= H - 1) and none is younger than 32 frames (d >= base >= 32).  After a call that returns S2R_OK the history is the
 * last H frames of (old history, then w[0 .. N)) and the phase is phase + phase_inc * N: calls of any lengths concatenate.  The stage
 * runs once per call over all N frames, after every event segment and rows slice has been mixed.  A flanger on a bus >= the call's
 * n_buses is idle in that call (no output, state untouched).  A bus without a flanger passes through bit for bit, -0.0 included.  A
 * refused or failed call leaves history and phase untouched.  ONLY s2r_fill_buses and s2r_fill_master apply it; every other fill
 * ignores it.  A handle on which none was ever set launches what it launched before and allocates nothing for one; device memory is
 * allocated when a flanger is set (S2R_ERR_OUT_OF_MEMORY when that fails, and the earlier flanger is kept), never in a fill.
 *   s2r_flanger_history_frames: H for a (base, depth) in range, 0 otherwise; needs no handle.
 *   s2r_set_bus_flanger: replaces any earlier flanger of the bus, zeroes its history and its phase.  S2R_ERR_PATCH_RANGE for a value
 *   outside its range, a NaN or bus >= S2R_MAX_BUSES (checked before the handle is looked at; nothing is changed).
 *   s2r_clear_bus_flanger removes it (S2R_OK on a bus without).
 *   s2r_set_bus_flanger_params: everything but the two values that fix H; history and phase stay, so rate and resonance move
 *   without a click.  S2R_ERR_INVALID on a bus without a flanger.
 *   s2r_get_bus_flanger: base is 0 for a bus without one; any pointer may be NULL.
 *   s2r_get_bus_flanger_state / s2r_set_bus_flanger_state: the 2 * H floats of the history and the phase.  S2R_ERR_INVALID for a
 *   capacity below, or a count other than, 2 * H, a NULL lr, and on a bus without a flanger; `phase` may be NULL in the getter.
 *   Single-device handles (a NULL or a device-list handle: S2R_ERR_INVALID from all six).
 *   s2r_flanger_reference: the rule above on the host (no device, no handle): x_lr is [frames][2]; history_lr, [H][2], and *phase are
 *   updated in place; out_lr may be NULL.  Range checks as above; S2R_ERR_INVALID for a NULL history_lr or phase, or a NULL x_lr
 *   with frames > 0. */
#define S2R_FLANGER_MIN_DELAY 32.0f
#define S2R_FLANGER_MAX_DELAY 4095.0f
uint32_t s2r_flanger_history_frames(float base, float depth);
int s2r_set_bus_flanger(s2r_synth *s, uint32_t bus, float base, float depth, uint32_t phase_inc, uint32_t spread, float feedback, float cross,
                        float dry, float wet);
int s2r_clear_bus_flanger(s2r_synth *s, uint32_t bus);
int s2r_set_bus_flanger_params(s2r_synth *s, uint32_t bus, uint32_t phase_inc, uint32_t spread, float feedback, float cross, float dry, float wet);
int s2r_get_bus_flanger(const s2r_synth *s, uint32_t bus, float *base, float *depth, uint32_t *phase_inc, uint32_t *spread, float *feedback,
                        float *cross, float *dry, float *wet);
int s2r_get_bus_flanger_state(s2r_synth *s, uint32_t bus, float *lr, size_t capacity, uint32_t *phase);
int s2r_set_bus_flanger_state(s2r_synth *s, uint32_t bus, const float *lr, size_t count, uint32_t phase);
int s2r_flanger_reference(float base, float depth, uint32_t phase_inc, uint32_t spread, float feedback, float cross, float dry, float wet,
                          const float *x_lr, uint32_t frames, float *history_lr, uint32_t *phase, float *out_lr);

/* BUILD-DEFINED master section (the reference's Synth::sample returns one stream; DESIGN.md 4.17 gives the op sequence): the last stage
 * of the chain send -> effect -> return -> master, on the device the bus signals are already on.  Every bus b in [0, S2R_MAX_BUSES) has
 * a `return` level in [0, 1] (default 1) and the handle a master fader in [0, 1] (default 1); each is a target / applied pair like the
 * program faders.  In a s2r_fill_master call of N frames over n_buses buses, with y_b,c[i] what s2r_fill_buses would write for bus b,
 * channel c, frame i (reverbs included), (R0_b, R1_b) the bus's applied and target return and (M0, M1) the master's pair:
 *   r_b[i] = R0_b + (float)i * ((R1_b - R0_b) / (float)N), m[i] likewise from M0 and M1 (i counts from the start of the call);
 *   t_c[i] = ((+0.0 + r_0[i] * y_0,c[i]) + r_1[i] * y_1,c[i]) + ... in bus order over b < n_buses;  out[2 i + c] = m[i] * t_c[i];
 * binary32, every operation rounded on its own, no fma, denormals kept.  A pair that did not move has a step of +0: its gain is R0
 * exactly.  A return of 0 mutes its bus.  METERS of the call: the buses on y_b,c (post-effect, pre-return: what the stems hold), the
 * master on out.  peak = max_i |v[i]|.  energy: q[i] = v[i] * v[i], rounded; the frames in blocks of S2R_METER_BLOCK, frames past N
 * counting +0.0; every block reduced by the adjacent-pair tree s[j] = s[2 j] + s[2 j + 1], eight levels; the block sums added in block
 * order from +0.0.  Non-finite bus samples are outside the contract.  When the call returns S2R_OK applied becomes target for every bus
 * and the master, and the call commits the program faders and moves the reverb histories exactly as s2r_fill_buses does; a refused or
 * failed call leaves returns, master fader, meters, faders and histories untouched.  ONLY s2r_fill_master applies returns, the master
 * fader and the meters: s2r_fill_buses and every other fill ignore them.  They belong to the buses and the handle: s2r_set_patch_bank,
 * program changes and s2r_import_state leave them alone.  Single-device handles; a handle with an exchange attached takes the setters
 * and refuses the fill, as it does s2r_fill_buses.  A handle on which s2r_fill_master was never called launches what it launched before.
 *   s2r_set_bus_return / s2r_set_master_fader set the target: S2R_ERR_PATCH_RANGE for a level outside [0, 1] or NaN or a bus >=
 *   S2R_MAX_BUSES (checked before the handle is looked at; nothing is changed).  The getters: target and applied; any pointer may be
 *   NULL.  s2r_snap_master: applied = target for every bus and the master, now — a hard cut, and the way to restore a checkpoint: set
 *   the applied values, snap, set the targets.
 *   s2r_fill_master: synchronous; writes 2 * frames floats to master_lr and — when `stems` is not NULL — what s2r_fill_buses writes to
 *   `stems`, same layout, same capacity check.  stems NULL: master only, and the stems never cross to the host.  Restrictions, events
 *   inside the call, rows slices and frames == 0 are s2r_fill_buses'.  The first call allocates a device buffer of 2 * S2R_MAX_BUSES *
 *   max_frames floats and a pinned row of meter partials per S2R_METER_BLOCK frames of max_frames.
 *   s2r_get_meters: the meters of the last successful s2r_fill_master: (n_buses + 1) * 2 entries per array — bus-major, L then R, the
 *   master last; S2R_ERR_INVALID before the first successful master fill or when `capacity` (entries per array) is too small; either
 *   array pointer and n_buses may be NULL.
 *   s2r_master_reference: the rule above on the host (no device, no handle): stems [n_buses][frames][2], r0 / r1 [n_buses]; writes
 *   master_lr [frames][2] and the meters in s2r_get_meters' layout; any output pointer may be NULL.  S2R_ERR_PATCH_RANGE for a level
 *   out of range, S2R_ERR_INVALID for n_buses outside 1 .. S2R_MAX_BUSES or a NULL input. */
#define S2R_METER_BLOCK 256u
int s2r_set_bus_return(s2r_synth *s, uint32_t bus, float level);
int s2r_get_bus_return(const s2r_synth *s, uint32_t bus, float *level, float *applied);
int s2r_set_master_fader(s2r_synth *s, float level);
int s2r_get_master_fader(const s2r_synth *s, float *level, float *applied);
int s2r_snap_master(s2r_synth *s);
int s2r_fill_master(s2r_synth *s, float *master_lr, float *stems, size_t stems_capacity, uint32_t n_buses, size_t frames, uint32_t sample_rate_hz);
int s2r_get_meters(const s2r_synth *s, uint32_t *n_buses, float *peak, float *energy, size_t capacity);
int s2r_master_reference(const float *stems, uint32_t n_buses, uint32_t frames, const float *r0, const float *r1, float m0, float m1,
                         float *master_lr, float *peak, float *energy);

/* BUILD-DEFINED master limiter (the reference has none; DESIGN.md 4.18 gives the op sequence): a look-ahead peak limiter behind the
 * master fader, in s2r_fill_master only, on the device the master is already on.  Off by default, and a handle on which it was never
 * set launches exactly what it launched before.  Parameters: `ceiling` C, finite, in [2^-S2R_LIMITER_CEILING_LOG2,
 * 2^S2R_LIMITER_CEILING_LOG2]; `lookahead` L in frames, 1 .. S2R_LIMITER_MAX_LOOKAHEAD; `hold` H in frames, 0 .. S2R_LIMITER_MAX_HOLD;
 * W = L + 1, G = 2 L + H.  STATE carried from call to call: xh, the last L stereo frames of the limiter's input, oldest first,
 * initially +0.0; gh, the last G values of g, oldest first, initially 1.0.  A call of N frames, x[n] what s2r_fill_master writes to
 * master_lr without a limiter (x[n], g[n] for n < 0 from xh, gh):
 *   1. p[n] = max(|x_L[n]|, |x_R[n]|);  g[n] = p[n] > C ? C / p[n] : 1.0f           (one gain for both channels)
 *   2. m[n] = min over k = 0 .. L + H of g[n - k], n in [-L, N)                      (any order: a minimum has one value)
 *   3. acc[n] = (((+0.0 + m[n]) + m[n - 1]) + ...) + m[n - L], W terms, newest first; s[n] = acc[n] / (float)W
 *   4. s'[n] = min(s[n], g[n - L])
 *   5. y_c[n] = min(max(x_c[n - L] * s'[n], -C), C)
 * binary32, every operation rounded on its own, no fma, denormals kept, the division correctly rounded.  The output is the input
 * delayed by L frames — in every bit under a signal that never exceeds C — and no output sample exceeds C in magnitude; the gain
 * reaches its minimum at the frame the peak comes out, stays for H frames more and recovers along a line of W frames.  After the call
 * xh and gh are the last L and G entries of history followed by call (also when N is shorter than either).  Non-finite input is
 * outside the contract.  THE STEMS ARE NOT DELAYED: with a limiter set the stems of a master fill lead its master by L frames.  The
 * master section's meters keep their rule: the master entry of s2r_get_meters is over x, before the limiter.  The limiter's own meters
 * of a call: min_gain = min_n s'[n], out_peak = max_n,c |y_c[n]|.  s2r_fill_buses and every other fill ignore the limiter;
 * s2r_set_patch_bank, program changes and s2r_import_state leave it alone.  A refused or failed call leaves state and meters as they
 * were.  Single-device handles (a device list refuses every entry); a handle with an exchange attached takes the setters and refuses
 * the fill.  The first master fill that finds a limiter set allocates a device buffer of 2 * max_frames floats, the two copies of the
 * state and a pinned pair of meter partials per 256 frames of max_frames.
 *   s2r_set_master_limiter: S2R_ERR_PATCH_RANGE for a NaN or a ceiling outside its range, lookahead 0 or too long, hold too long
 *   (checked before the handle is looked at; nothing is changed).  Resets xh and gh to their initial values when lookahead or hold
 *   differ from the present ones or the limiter was off; a call that changes the ceiling alone keeps the state (gh holds gains, not
 *   levels).  s2r_clear_master_limiter: off; the master fill returns what it returned before, with no delay.
 *   s2r_get_master_limiter: any pointer may be NULL; a lookahead of 0 means off (ceiling and hold are then 0).
 *   s2r_get_limiter_state / s2r_set_limiter_state (checkpoints): xh as 2 * L floats (frames, L then R), gh as G floats.  The setter
 *   takes exactly n_x == 2 * L and n_g == G, the getter capacities of at least that many; S2R_ERR_INVALID otherwise, with the limiter
 *   off or for a NULL buffer.
 *   s2r_get_limiter_meters: of the last successful s2r_fill_master that ran the limiter; S2R_ERR_INVALID before any such fill; either
 *   pointer may be NULL.
 *   s2r_limiter_reference: the rule above on the host (no device, no handle): x [frames][2], xh [lookahead][2] and gh [G] updated in
 *   place, y [frames][2] and gain [frames] (s') written; y and gain may be NULL, y may be x.  S2R_ERR_PATCH_RANGE as the setter's,
 *   S2R_ERR_INVALID for a NULL x (with frames > 0), xh or gh. */
#define S2R_LIMITER_MAX_LOOKAHEAD 1024u
#define S2R_LIMITER_MAX_HOLD 4096u
#define S2R_LIMITER_CEILING_LOG2 20
int s2r_set_master_limiter(s2r_synth *s, float ceiling, uint32_t lookahead, uint32_t hold);
int s2r_clear_master_limiter(s2r_synth *s);
int s2r_get_master_limiter(const s2r_synth *s, float *ceiling, uint32_t *lookahead, uint32_t *hold);
int s2r_get_limiter_state(s2r_synth *s, float *xh, size_t n_x, float *gh, size_t n_g);
int s2r_set_limiter_state(s2r_synth *s, const float *xh, size_t n_x, const float *gh, size_t n_g);
int s2r_get_limiter_meters(const s2r_synth *s, float *min_gain, float *out_peak);
int s2r_limiter_reference(const float *x, uint32_t frames, float ceiling, uint32_t lookahead, uint32_t hold, float *xh, float *gh,
                          float *y, float *gain);

/* BUILD-DEFINED true-peak detector of the master limiter (DESIGN.md 4.30 gives the op sequence).  The limiter above bounds the samples
 * it is given; with `detector` S2R_LIMITER_TRUE_PEAK it takes the magnitude of step 1 from the 4x interpolation of its input through
 * the drive's prototype g = 4 h (s2r_drive_taps) — the interpolator and the operation sequence of the loudness meter's true peak —, so
 * that what the meter reads and what the converter makes of the master stay near the ceiling.  S2R_LIMITER_SAMPLE_PEAK, the default
 * and what s2r_set_master_limiter sets, is the rule above: the same kernel, bits and launches.  With C, L, H, W = L + 1, G = 2 L + H
 * as above: STATE carried from call to call: xh, the last L + S2R_LIMITER_TP_HISTORY stereo frames of the limiter's input, oldest
 * first, initially +0.0; gh, the last G values of g, oldest first, initially 1.0.  A call of N frames (x[n], g[n] for n < 0 from xh,
 * gh):
 *   1'. for channel c and phase p in 0 .. 3: u_{p,c}[n] = sum over j of g4[p + 4 j] * x_c[n - j], from +0.0 in ascending j, while
 *       p + 4 j < S2R_DRIVE_TAPS (17 terms for phase 0, 16 for the others), g4 = 4 h;
 *       d[n] = max(|x_L[n - 8]|, |x_R[n - 8]|, |u_{p,c}[n]| over all p and c)           (any order: a maximum has one value)
 *       g[n] = d[n] > C ? C / d[n] : 1.0f
 *   2. - 4. as above, over this g
 *   5'. y_c[n] = min(max(x_c[n - L - 8] * s'[n], -C), C)
 * binary32, every operation rounded on its own, no fma, denormals kept, the division correctly rounded.  The interpolator is centred
 * S2R_LIMITER_TP_LATENCY = 8 frames back, so g[n - L] is centred on x[n - L - 8]: the master comes out L + 8 frames late — in every
 * bit under an input whose d never exceeds C.  No output sample exceeds C in magnitude.  Every frame, xh and gh are independent of how
 * a stream is cut into calls, calls shorter than 8 or 16 frames included.  THE TRUE PEAK OF THE OUTPUT IS NOT BOUNDED EXACTLY: the
 * gain moves inside the interpolator's span, so the interpolation of the product is not the product of the interpolation.  What was
 * measured (float64, tools/limiter_tp_truth.py, profiles/truth/limiter_tp_deviation.json): at most 1.0026 C by the project's meter on
 * an fs/4 sine at 45 degrees, noise and a naive square at (48, 0) and (16, 8), where the sample-peak rule reads 1.24 to 1.43 C.  A
 * lookahead of a few frames leaves more (1.0083 C at (5, 3)).  The interpolator's passband ends near 0.29 of the rate, as the
 * meter's.  The stems are not delayed; meters, refusals and allocations as above.
 *   s2r_set_master_limiter_ex: s2r_set_master_limiter with the detector.  S2R_ERR_PATCH_RANGE also for a detector above 1, checked
 *   with the other ranges before the handle is looked at.  Another detector resets the state as another lookahead or hold does.
 *   s2r_get_master_limiter_detector: the detector (0 with the limiter off); S2R_ERR_INVALID for a NULL pointer.
 *   s2r_get_limiter_state / s2r_set_limiter_state: with the true-peak detector xh is 2 * (L + 16) floats; gh is G floats.
 *   s2r_limiter_tp_reference: the rule on the host, as s2r_limiter_reference: xh [L + 16][2] and gh [G] updated in place. */
#define S2R_LIMITER_SAMPLE_PEAK 0u
#define S2R_LIMITER_TRUE_PEAK 1u
#define S2R_LIMITER_TP_LATENCY 8u
#define S2R_LIMITER_TP_HISTORY 16u
int s2r_set_master_limiter_ex(s2r_synth *s, float ceiling, uint32_t lookahead, uint32_t hold, uint32_t detector);
int s2r_get_master_limiter_detector(const s2r_synth *s, uint32_t *detector);
int s2r_limiter_tp_reference(const float *x, uint32_t frames, float ceiling, uint32_t lookahead, uint32_t hold, float *xh, float *gh,
                             float *y, float *gain);

/* BUILD-DEFINED master multiband compressor (the reference has none; DESIGN.md 4.31 gives the op sequence): the master insert, behind
 * the master kernel (returns, bus-order sum, master fader) and in front of the limiter, in s2r_fill_master only.  It splits the master
 * into B = n_bands (1 .. S2R_MULTIBAND_MAX_BANDS) frequency bands, gives each band a gain of its own by the rule of the bus dynamics,
 * and adds the bands in band order.  Off by default, no latency, the stems untouched; the limiter, both meters, the converter and the
 * PCM stage see the processed master; a handle on which it was never set launches what it launched before and allocates nothing.
 * A SECTION is one band of s2r_eq_reference with its own (s1, s2) per channel: transposed direct form II, the nine rounded operations
 * of the bus EQ, no fma, denormals kept, nothing skipped for a zero, both channels the same five coefficients (b0, b1, b2, a1, a2).
 * Split k (0 .. B - 2) owns four sections: LPa_k and LPb_k with the coefficients lp[k], HPa_k and HPb_k with hp[k]; for k >= 1 there
 * is also an allpass row ap[k - 1].  Per channel:
 *   1. r_0 = x;  for k = 0 .. B - 2: band_k = LPb_k(LPa_k(r_k)), r_{k+1} = HPb_k(HPa_k(r_k));  band_{B-1} = r_{B-1}
 *   2. band j <= B - 3 then passes, in ascending k, through an allpass section AP_{j,k} for k = j + 1 .. B - 2, each with a state of
 *      its own and the coefficients ap[k - 1]                                  (S(B) = 4 (B-1) + (B-1)(B-2)/2 sections: 0, 4, 9, 15)
 *   3. band j has a curve of S2R_DYN_CURVE_POINTS gains, a_att[j], a_rel[j] and a gain y_j shared by both channels; per frame
 *      p = max(|band_jL|, |band_jR|), then steps 2 and 3 of the bus dynamics verbatim (the table lookup, t < y ? a_att : a_rel,
 *      y = t + (a * (y - t))), then o_jc = band_jc * y_j
 *   4. out_c = o_0c, then out_c = out_c + o_jc for j = 1 .. B - 1 in band order (no zero in front: B = 1 is the bus dynamics keyed by
 *      itself, in every bit)
 * binary32, every operation rounded on its own.  STATE, S2R_MULTIBAND_STATE(B) = 4 S(B) + B floats: [section][s1_L, s1_R, s2_L, s2_R]
 * in the order LPa_0, LPb_0, HPa_0, HPb_0, LPa_1, ..., then AP_{0,1}, AP_{0,2}, AP_{1,2}, then the B gains.  Right after a set the
 * filters hold +0.0 and y_j = curves[j][0].  Calls of any lengths concatenate; a refused or failed call leaves the state untouched.
 * The meter of a call is min over n of y_j[n] per band; s2r_get_meters stays what the master kernel measured, in front of the stage.
 *   s2r_set_master_multiband: lp and hp are [B - 1][5], ap [B - 2][5] (NULL is accepted for an array of no rows), curves
 *   [B][S2R_DYN_CURVE_POINTS], a_att and a_rel [B].  S2R_ERR_PATCH_RANGE for n_bands outside 1 .. 4, coefficients as s2r_set_bus_eq
 *   refuses them, curves and retention coefficients as s2r_set_bus_dynamics does — all before the handle is looked at;
 *   S2R_ERR_INVALID for a NULL or device-list handle or a NULL array that has rows.  A refusal changes nothing.
 *   s2r_set_master_multiband_params: the same arguments with the n_bands that is set (another: S2R_ERR_INVALID); the state stays.
 *   s2r_clear_master_multiband: off.  s2r_get_master_multiband: *n_bands is 0 when off; every array may be NULL.
 *   s2r_reset_master_multiband: the state right after a set; the parameters stay.
 *   s2r_get_multiband_state / s2r_set_multiband_state: S2R_MULTIBAND_STATE(B) floats (a capacity of at least that; a count of exactly
 *   that, every float finite, the gains >= 0: else S2R_ERR_PATCH_RANGE).  The setter and s2r_set_master_multiband_params leave the
 *   meters of the last fill as they are; a set, a reset and a fresh handle that is given a checkpoint hold none.
 *   s2r_get_multiband_meters: min_gain [B] of the last successful master fill that ran the stage; S2R_ERR_INVALID before one.
 *   s2r_multiband_reference: the rule on the host: state [S2R_MULTIBAND_STATE(B)] in place; out_lr [frames][2], bands
 *   [B][frames][2] (the band signals in front of the gains) and min_gain [B] (written when frames > 0) may each be NULL.
 *   s2r_multiband_design: n_splits (0 .. 3) second-order Butterworth (Q = 1/sqrt 2) cookbook low-pass, high-pass and allpass rows at
 *   freqs_hz, binary64, rounded once: lp, hp [n_splits][5], ap [n_splits - 1][5] for splits 1 ..; two low-passes and two high-passes
 *   in series are a fourth-order Linkwitz-Riley split, whose two bands add to that allpass.  S2R_ERR_PATCH_RANGE unless the
 *   frequencies ascend strictly inside (0, sample_rate / 2). */
#define S2R_MULTIBAND_MAX_BANDS 4u
#define S2R_MULTIBAND_SECTIONS(B) (4u * ((B) - 1u) + ((B) - 1u) * ((B) - 2u) / 2u)
#define S2R_MULTIBAND_STATE(B) (4u * S2R_MULTIBAND_SECTIONS(B) + (B))
int s2r_set_master_multiband(s2r_synth *s, uint32_t n_bands, const float *lp, const float *hp, const float *ap, const float *curves,
                             const float *a_att, const float *a_rel);
int s2r_set_master_multiband_params(s2r_synth *s, uint32_t n_bands, const float *lp, const float *hp, const float *ap, const float *curves,
                                    const float *a_att, const float *a_rel);
int s2r_clear_master_multiband(s2r_synth *s);
int s2r_get_master_multiband(const s2r_synth *s, uint32_t *n_bands, float *lp, float *hp, float *ap, float *curves, float *a_att, float *a_rel);
int s2r_reset_master_multiband(s2r_synth *s);
int s2r_get_multiband_state(s2r_synth *s, float *state, size_t capacity);
int s2r_set_multiband_state(s2r_synth *s, const float *state, size_t count);
int s2r_get_multiband_meters(const s2r_synth *s, float *min_gain, size_t capacity);
int s2r_multiband_reference(uint32_t n_bands, const float *lp, const float *hp, const float *ap, const float *curves, const float *a_att,
                            const float *a_rel, const float *x_lr, uint32_t frames, float *state, float *out_lr, float *bands, float *min_gain);
int s2r_multiband_design(double sample_rate, const double *freqs_hz, uint32_t n_splits, float *lp, float *hp, float *ap);

/* BUILD-DEFINED loudness and true-peak meters (the reference has none; DESIGN.md 4.26 gives the op sequence): ITU-R BS.1770 / EBU R128
 * momentary, short-term and gated integrated loudness of every bus and of the master, and the master's true peak, behind the master
 * limiter, in s2r_fill_master only, on the device the stems and the master are already on.  Off by default, and a handle on which the
 * meter was never set launches exactly what it launched before; master_lr and the stems are the same bits with the meter on or off.
 * PROGRAMMES: P = S2R_LOUDNESS_PROGRAMMES = S2R_MAX_BUSES + 1 = 9.  Programme b < 8 is bus b as the stems hold it — post-effect,
 * pre-return, as for s2r_get_meters —, programme 8 the master as the caller receives it, behind the limiter when one is set.  18
 * channels, channel q = 2 p + c.  A bus at or past the call's n_buses is fed +0.0 for every frame of the call: its filters run on
 * zeros, and the hop position is common to all programmes.
 * PARAMETERS: `coeffs`, two biquads (b0, b1, b2, a1, a2), finite: the K-weighting pre-filter, a high shelf and then a high-pass
 * (s2r_loudness_design); `hop`, the frames of 100 ms, 16 .. S2R_LOUDNESS_MAX_HOP; `max_hops`, the hop rows the handle keeps for the
 * integrated value, 30 .. S2R_LOUDNESS_MAX_HOPS: a sliding window, whose oldest row drops when a new one would exceed it.
 * STATE carried from call to call, S2R_LOUDNESS_STATE = 122 floats and `pos`: the filters' values [18][2][2] (channel, stage,
 * (s1, s2)), the partial hop sums e[18], the last 16 master frames [16][2], oldest first, L then R; pos < hop, the frames of the hop
 * under way.  All +0.0 / 0 right after a set or a reset.
 * DEVICE RULE, binary32, every operation rounded on its own, no fma, denormals kept.  For each channel q and each frame n of the
 * call, in frame order, v[n] the channel's sample:
 *   1. y1 = stage 1 on v[n], y2 = stage 2 on y1; a stage with x its input and its own (s1, s2) is one band of s2r_eq_reference:
 *      y = (b0 * x) + s1;   s1' = ((b1 * x) - (a1 * y)) + s2;   s2' = (b2 * x) - (a2 * y)
 *   2. z = y2 * y2;   e_q = e_q + z
 *   3. after the frame pos = pos + 1; when pos == hop the 18 values e_q become one HOP ROW, every e_q = +0.0 and pos = 0.
 * The hop sum is sequential, so every reading is independent of how a stream is cut into calls.
 * TRUE PEAK, master only: with g[k] = 4 h[k] the drive's interpolator (s2r_drive_taps, S2R_DRIVE_OVERSAMPLE = 4) and x_c[n] for n < 0
 * from the state, u_p[n] = sum over j with p + 4 j < S2R_DRIVE_TAPS of g[p + 4 j] * x_c[n - j], from +0.0 in ascending j, p = 0 .. 3;
 * tp_c of a call = max over its frames of |x_c[n]| and the four |u_p[n]|.  The handle keeps the maximum since the last reset.  The
 * prototype's passband ends near 0.29 of the sample rate: PEAKS OF CONTENT ABOVE THAT ARE UNDERESTIMATED.
 * HOST RULE, binary64 (s2r_loudness_readings), over hop rows [n_hops][18] and one programme p, with t_i = (double)row_i[2 p] +
 * (double)row_i[2 p + 1]: block j >= 3 has the mean square m_j = (((t_(j-3) + t_(j-2)) + t_(j-1)) + t_j) / (4.0 * hop) and the
 * loudness l_j = -0.691 + 10 log10(m_j).  out[0], momentary: l of the last block.  out[1], short-term: the same over the last 30
 * hops, summed in order from 0.0, divided by 30.0 * hop.  out[2], integrated, BS.1770's two gates: keep the blocks with l_j > -70; the
 * relative threshold is the loudness of the mean of their m_j (summed in order from 0.0), minus 10; the reading is the loudness of
 * the mean of the m_j of the blocks with l_j above both.  A reading is -inf where there are too few hops or nothing passes.
 * A refused or failed call leaves state, rows and readings as they were; s2r_fill_buses and every other fill ignore the meter.
 * Single-device handles (a device list refuses every entry).  The first master fill that finds the meter set allocates a device
 * buffer of 2 * max_frames floats, the two copies of the state and pinned rows for max_frames / 16 + 1 hops.
 *   s2r_set_master_loudness: S2R_ERR_PATCH_RANGE for a coefficient that is not finite, hop or max_hops out of range (checked before
 *   the handle is looked at; nothing is changed); S2R_ERR_INVALID for NULL coeffs.  Resets state, rows and the held true peak.
 *   s2r_clear_master_loudness: off.  s2r_get_master_loudness: any pointer may be NULL; a hop of 0 means off; n_hops the stored rows.
 *   s2r_reset_master_loudness: state, rows and held true peak cleared, parameters kept; S2R_ERR_INVALID with the meter off.
 *   s2r_get_loudness: out[3] = momentary, short-term, integrated of `programme` (< 9, else S2R_ERR_PATCH_RANGE) over the stored rows.
 *   s2r_get_true_peak: last[2] of the last successful master fill with the meter (0 before one), held[2] since the last reset; L, R.
 *   s2r_get_loudness_state / s2r_set_loudness_state (checkpoints): the 122 floats and pos.  The getter takes a capacity of at least
 *   122, the setter exactly 122 and a pos below hop (S2R_ERR_PATCH_RANGE).  s2r_get_loudness_hops / s2r_set_loudness_hops: the stored
 *   rows, oldest first, [n_hops][18]; the getter takes a capacity in floats, the setter exactly count == 18 * n_hops, n_hops <=
 *   max_hops (S2R_ERR_PATCH_RANGE past it).  S2R_ERR_INVALID for a wrong size, a NULL buffer or with the meter off.
 *   s2r_loudness_reference: the device rule on the host (no device, no handle).  stems [n_buses][frames][2] (NULL with n_buses 0),
 *   master_lr [frames][2]; state[122] and *pos updated in place; the call's hop rows written to rows[0 .. 18 * *n_rows), which holds
 *   rows_capacity floats (checked before anything is changed); true_peak[2] the call's (may be NULL).  S2R_ERR_PATCH_RANGE as the
 *   setter's, for n_buses > 8 or *pos >= hop; S2R_ERR_INVALID for a NULL or a capacity too small.
 *   s2r_loudness_readings: the host rule.  S2R_ERR_PATCH_RANGE for a hop out of range or programme >= 9, S2R_ERR_INVALID for NULL.
 *   s2r_loudness_design: BS.1770's pre-filter at any rate, by the bilinear form with K = tan(pi f0 / sample_rate), binary64, rounded
 *   once.  Stage 1, a high shelf: f0 = 1681.974450955533 Hz, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G / 20),
 *   Vb = Vh^0.4996667741545416; a0 = 1 + K / Q + K^2, b0 = (Vh + Vb K / Q + K^2) / a0, b1 = 2 (K^2 - Vh) / a0, b2 = (Vh - Vb K / Q +
 *   K^2) / a0, a1 = 2 (K^2 - 1) / a0, a2 = (1 - K / Q + K^2) / a0.  Stage 2, a high-pass: f0 = 38.13547087602444 Hz, Q =
 *   0.5003270373238773; b = (1, -2, 1), a1 and a2 as above.  At 48 kHz this is the table BS.1770 prints.  S2R_ERR_PATCH_RANGE for
 *   a sample_rate that is a NaN or outside [S2R_LOUDNESS_MIN_RATE, S2R_LOUDNESS_MAX_RATE], S2R_ERR_INVALID for NULL coeffs. */
#define S2R_LOUDNESS_PROGRAMMES 9u
#define S2R_LOUDNESS_CHANNELS 18u
#define S2R_LOUDNESS_STATE 122u
#define S2R_LOUDNESS_MIN_HOP 16u
#define S2R_LOUDNESS_MAX_HOP (1u << 20)
#define S2R_LOUDNESS_MIN_HOPS 30u
#define S2R_LOUDNESS_MAX_HOPS (1u << 18)
#define S2R_LOUDNESS_MIN_RATE 8000.0
#define S2R_LOUDNESS_MAX_RATE 768000.0
int s2r_set_master_loudness(s2r_synth *s, const float coeffs[10], uint32_t hop, uint32_t max_hops);
int s2r_clear_master_loudness(s2r_synth *s);
int s2r_get_master_loudness(const s2r_synth *s, float coeffs[10], uint32_t *hop, uint32_t *max_hops, size_t *n_hops);
int s2r_reset_master_loudness(s2r_synth *s);
int s2r_get_loudness(const s2r_synth *s, uint32_t programme, double out[3]);
int s2r_get_true_peak(const s2r_synth *s, float last[2], float held[2]);
int s2r_get_loudness_state(s2r_synth *s, float *state, size_t capacity, uint32_t *pos);
int s2r_set_loudness_state(s2r_synth *s, const float *state, size_t count, uint32_t pos);
int s2r_get_loudness_hops(const s2r_synth *s, float *rows, size_t capacity, size_t *n_hops);
int s2r_set_loudness_hops(s2r_synth *s, const float *rows, size_t n_hops, size_t count);
int s2r_loudness_reference(const float coeffs[10], uint32_t hop, const float *stems, uint32_t n_buses, const float *master_lr,
                           uint32_t frames, float *state, uint32_t *pos, float *rows, size_t rows_capacity, size_t *n_rows,
                           float true_peak[2]);
int s2r_loudness_readings(const float *rows, size_t n_hops, uint32_t hop, uint32_t programme, double out[3]);
int s2r_loudness_design(double sample_rate, float coeffs[10]);

/* BUILD-DEFINED spectrum meters (the reference has none): a windowed power-of-two FFT of every bus and of the master,
 * behind the loudness meters, in s2r_fill_master only, on the device the stems and the master are already on.  Off by default, and a
 * handle on which the meter was never set launches exactly what it launched before; master_lr, the stems and the loudness rows are the
 * same bits with the meter on or off.
 * PROGRAMMES: S2R_SPECTRUM_PROGRAMMES = 9, the loudness meters': programme b < 8 is bus b as the stems hold it (post-effect,
 * pre-return), programme 8 the master as the caller receives it, behind the limiter when one is set.  A bus at or past the call's
 * n_buses is fed +0.0 for every frame of the call.
 * PARAMETERS: n_fft = N, a power of two in S2R_SPECTRUM_MIN_FFT .. S2R_SPECTRUM_MAX_FFT (256 .. 8192); hop in max(16, N / 8) ..
 * S2R_SPECTRUM_MAX_HOP (a hop longer than N skips frames); window[N], finite floats; max_rows in 1 .. S2R_SPECTRUM_MAX_ROWS, the rows
 * the handle keeps: a sliding window whose oldest row drops when a new one would exceed it.
 * STREAM AND ROWS: each programme is a stream of stereo frames; the frames before the first fill, a reset or a set are +0.0.  `pos`
 * counts the frames of the hop under way.  When a frame makes pos + 1 == hop, pos returns to 0 and a ROW is taken over the N most
 * recent frames ending at that frame, oldest first: z[i] = (window[i] * L[i], window[i] * R[i]), one complex transform for both
 * channels.  A row is [9][N / 2 + 1] floats, S2R_SPECTRUM_ROW(N) of them.
 * STATE carried from call to call: the last N frames of all nine programmes, [9][N][2] floats (programme, frame oldest first, L then
 * R), S2R_SPECTRUM_STATE(N) = 18 * N of them, and pos < hop.  All +0.0 / 0 right after a set or a reset.
 * DEVICE RULE, binary32, every operation rounded on its own, no fma, denormals kept.
 *   TWIDDLES T[j], j < N / 2 (s2r_spectrum_twiddles), computed by the host, read by the device:
 *     j <= N / 8:          T[j] = (cos(2 pi j / N), -sin(2 pi j / N)) in binary64, each rounded to nearest binary32; T[0].im is +0.0
 *     N / 8 < j <= N / 4:  T[j] = (-T[N / 4 - j].im, -T[N / 4 - j].re)
 *     N / 4 < j < N / 2:   T[j] = (T[j - N / 4].im, -T[j - N / 4].re)
 *   so T[0] = (1, 0) and T[N / 4] = (0, -1) exactly, and the table is symmetric on bits.
 *   TRANSFORM, radix-2 decimation in time: v[i] = z[bitrev(i)] (bitrev over log2 N bits); for s = 1 .. log2 N, m = 2^s, h = m / 2, for
 *   every block base g (a multiple of m) and j < h:
 *     w = T[j * (N / m)];   a = v[g + j];   b = v[g + j + h]
 *     t = (w.re * b.re - w.im * b.im,  w.re * b.im + w.im * b.re)
 *     v'[g + j] = a + t;   v'[g + j + h] = a - t
 *   The rule fixes the arithmetic graph, not the storage: any layout, any number of layers held in registers, is the rule when every
 *   value comes from the same operations.  The products with T[0] and T[N / 4] change only the signs of zeros, which cannot reach a
 *   row for finite input; an implementation may skip them.  FOR NON-FINITE INPUT THE CONTRACT IS ONLY THAT A ROW VALUE IS NON-FINITE
 *   WHERE THE RULE'S IS.
 *   POWER, k = 0 .. N / 2, a = v[k], b = v[(N - k) mod N]:
 *     p[k] = ((a.re * a.re + a.im * a.im) + (b.re * b.re + b.im * b.im)) * 0.5f
 *   which is |X_L[k]|^2 + |X_R[k]|^2 without an untangling pass.  A programme at or past the call's n_buses gets p[k] = +0.0.
 * Rows and state do not depend on how a stream is cut into calls.
 * HOST RULE, binary64, pure functions of the rows.  s2r_spectrum_readings, over the last n_avg rows (1 .. n_rows) of one programme:
 *   q[k] = c_k * (sum over those rows, oldest first, from 0.0, of (double)p_r[k]) / n_avg / (S1 * S1),   dB[k] = 10 log10(q[k])
 *   with S1 the sum of (double)window[i] in index order from 0.0, c_k = 2 for 0 < k < N / 2 and 0.5 at k = 0 and k = N / 2.  Silence
 *   reads -inf.  A bin-centred sine of amplitude 1 on both channels reads 0 dB, on one channel -3.01 dB, DC of 1 on both 0 dB.
 *   s2r_spectrum_band_readings: fractional-octave bands, bands_per_octave one of 1, 3, 6, 12.  Centres 1000 * 2^(i / bpo) Hz for
 *   integer i, ascending; edges the centre times 2^(-1 / (2 bpo)) and 2^(+1 / (2 bpo)); a band is kept when its lower edge is at or
 *   above sample_rate / N and its upper edge at or below sample_rate / 2.  Bin k covers [(k - 1/2), (k + 1/2)] * sample_rate / N; a
 *   band's power is the sum, in ascending k from 0.0, of q[k] times the fraction of bin k inside the band; dB = 10 log10 of it.
 * A refused or failed call leaves state, rows and readings as they were; every fill but s2r_fill_master ignores the meter.
 * Single-device handles (a device list refuses every entry).  The first master fill that finds the meter set allocates the two
 * copies of the state, the window and twiddles on the device, and pinned rows for max_frames / hop + 1 rows.
 *   s2r_set_master_spectrum: S2R_ERR_PATCH_RANGE for n_fft, hop or max_rows out of range or a window value that is not finite
 *   (checked before the handle is looked at; nothing is changed); S2R_ERR_INVALID for a NULL window.  Resets state and rows.
 *   s2r_clear_master_spectrum: off.  s2r_get_master_spectrum: any pointer may be NULL; an n_fft of 0 means off; n_rows the stored
 *   rows; `window` receives the N values when window_capacity >= N (S2R_ERR_INVALID when it is non-NULL and smaller).
 *   s2r_reset_master_spectrum: state and rows cleared, parameters kept; S2R_ERR_INVALID with the meter off.
 *   s2r_get_spectrum: out_db[N / 2 + 1] of `programme` (< 9, else S2R_ERR_PATCH_RANGE) over the last n_avg stored rows
 *   (S2R_ERR_PATCH_RANGE for n_avg == 0 or more than the stored rows); capacity in doubles, at least N / 2 + 1.
 *   s2r_get_spectrum_bands: the same per band; out_db and centres hold `capacity` doubles each (centres may be NULL), *n_bands the
 *   bands kept; S2R_ERR_INVALID for a capacity below them.
 *   s2r_get_spectrum_rows / s2r_set_spectrum_rows (checkpoints): the stored rows, oldest first, [n_rows][9][N / 2 + 1]; the getter
 *   takes a capacity in floats, the setter exactly count == n_rows * S2R_SPECTRUM_ROW(N), n_rows <= max_rows (S2R_ERR_PATCH_RANGE
 *   past it).  s2r_get_spectrum_state / s2r_set_spectrum_state: the 18 * N floats and pos; the getter takes a capacity of at least
 *   18 * N, the setter exactly 18 * N and a pos below hop (S2R_ERR_PATCH_RANGE).  S2R_ERR_INVALID for a wrong size, a NULL buffer or
 *   with the meter off.
 *   s2r_spectrum_reference: the device rule on the host (no device, no handle).  stems [n_buses][frames][2] (NULL with n_buses 0),
 *   master_lr [frames][2]; state[18 * N] and *pos updated in place; the call's rows written to rows[0 .. *n_rows * S2R_SPECTRUM_ROW(N)),
 *   which holds rows_capacity floats (checked before anything is changed).  S2R_ERR_PATCH_RANGE as the setter's, for n_buses > 8 or
 *   *pos >= hop; S2R_ERR_INVALID for a NULL or a capacity too small.
 *   s2r_spectrum_readings / s2r_spectrum_band_readings: the host rule over rows [n_rows][9][N / 2 + 1].  S2R_ERR_PATCH_RANGE for an
 *   n_fft out of range, programme >= 9, n_avg == 0 or > n_rows, a bands_per_octave not of the four, a sample_rate that is not
 *   finite and positive; S2R_ERR_INVALID for NULL or a capacity too small.
 *   s2r_spectrum_window: the periodic form of `kind`, binary64 rounded to binary32, x = 2 pi i / N: S2R_WINDOW_RECT 1; S2R_WINDOW_HANN
 *   0.5 - 0.5 cos x; S2R_WINDOW_HAMMING 0.54 - 0.46 cos x; S2R_WINDOW_BLACKMAN_HARRIS 0.35875 - 0.48829 cos x + 0.14128 cos 2x -
 *   0.01168 cos 3x.  S2R_ERR_PATCH_RANGE for an unknown kind or n_fft out of range, S2R_ERR_INVALID for NULL.
 *   s2r_spectrum_twiddles: twiddles[N / 2][2] (re, im), the table above.  The same refusals. */
#define S2R_SPECTRUM_PROGRAMMES 9u
#define S2R_SPECTRUM_MIN_FFT 256u
#define S2R_SPECTRUM_MAX_FFT 8192u
#define S2R_SPECTRUM_MIN_HOP 16u
#define S2R_SPECTRUM_MAX_HOP (1u << 20)
#define S2R_SPECTRUM_MAX_ROWS 256u
#define S2R_SPECTRUM_ROW(n_fft) ((size_t)S2R_SPECTRUM_PROGRAMMES * ((size_t)(n_fft) / 2u + 1u))
#define S2R_SPECTRUM_STATE(n_fft) ((size_t)S2R_SPECTRUM_PROGRAMMES * 2u * (size_t)(n_fft))
#define S2R_WINDOW_RECT 0u
#define S2R_WINDOW_HANN 1u
#define S2R_WINDOW_HAMMING 2u
#define S2R_WINDOW_BLACKMAN_HARRIS 3u
int s2r_set_master_spectrum(s2r_synth *s, uint32_t n_fft, uint32_t hop, const float *window, uint32_t max_rows);
int s2r_clear_master_spectrum(s2r_synth *s);
int s2r_get_master_spectrum(const s2r_synth *s, uint32_t *n_fft, uint32_t *hop, uint32_t *max_rows, size_t *n_rows, float *window,
                            size_t window_capacity);
int s2r_reset_master_spectrum(s2r_synth *s);
int s2r_get_spectrum(const s2r_synth *s, uint32_t programme, uint32_t n_avg, double *out_db, size_t capacity);
int s2r_get_spectrum_bands(const s2r_synth *s, uint32_t programme, uint32_t n_avg, double sample_rate, uint32_t bands_per_octave,
                           double *out_db, double *centres, size_t capacity, size_t *n_bands);
int s2r_get_spectrum_rows(const s2r_synth *s, float *rows, size_t capacity, size_t *n_rows);
int s2r_set_spectrum_rows(s2r_synth *s, const float *rows, size_t n_rows, size_t count);
int s2r_get_spectrum_state(s2r_synth *s, float *state, size_t capacity, uint32_t *pos);
int s2r_set_spectrum_state(s2r_synth *s, const float *state, size_t count, uint32_t pos);
int s2r_spectrum_reference(uint32_t n_fft, uint32_t hop, const float *window, const float *stems, uint32_t n_buses,
                           const float *master_lr, uint32_t frames, float *state, uint32_t *pos, float *rows, size_t rows_capacity,
                           size_t *n_rows);
int s2r_spectrum_readings(const float *rows, size_t n_rows, uint32_t n_fft, const float *window, uint32_t programme, uint32_t n_avg,
                          double *out_db, size_t capacity);
int s2r_spectrum_band_readings(const float *rows, size_t n_rows, uint32_t n_fft, const float *window, uint32_t programme,
                               uint32_t n_avg, double sample_rate, uint32_t bands_per_octave, double *out_db, double *centres,
                               size_t capacity, size_t *n_bands);
int s2r_spectrum_window(uint32_t kind, uint32_t n_fft, float *window);
int s2r_spectrum_twiddles(uint32_t n_fft, float *twiddles);

/* BUILD-DEFINED PCM output stage (the reference's player lets its audio host truncate, audio_player.rs:73-105): the
 * word-length reduction of every bus and of the master to B-bit integers, with dither and error-feedback noise shaping, behind the
 * spectrum meters, the last stage of s2r_fill_master and of no other fill.  Off by default, and a handle on which the stage was never
 * set launches exactly what it launched before and allocates nothing; master_lr, the stems, the loudness rows and the spectrum rows are
 * the same bits with the stage on or off.
 * PROGRAMMES: S2R_PCM_PROGRAMMES = 9, the meters': programme b < 8 is bus b as the stems hold it, programme 8 the master as the caller
 * receives it.  Channel q = 2 p + c, S2R_PCM_CHANNELS = 18 of them.  A bus at or past the call's n_buses is fed +0.0.
 * PARAMETERS: bits = B in S2R_PCM_MIN_BITS .. S2R_PCM_MAX_BITS (8 .. 24); dither S2R_DITHER_NONE, S2R_DITHER_RECT (1 LSB peak to peak)
 * or S2R_DITHER_TRI (2 LSB); taps h[0 .. K), K = n_taps in 0 .. S2R_PCM_MAX_TAPS (9), each finite with |h| <= 16: the noise transfer
 * is 1 - sum h[k-1] z^-k; seed: any value.  One set of parameters serves all 18 channels.
 * STATE carried from call to call: S2R_PCM_STATE = 18 * 9 floats, row q = e_q[n-1], e_q[n-2], ...: the channel's last nine shaped
 * errors, newest first, every one in [-2, 2]; and t, the frames converted since the set or reset, mod 2^32.  All +0.0 / 0 right after
 * a set or a reset.  The rule reads the first K entries of a row; a call of one frame or more leaves the entries past K as +0.0.
 * DEVICE RULE, binary32, every operation rounded on its own, no fma, denormals kept.  Per channel q and frame n of the call, in frame
 * order, G = 2^(B-1), x the channel's sample:
 *   1. xc = +0.0 if x is a NaN, else min(max(x, -2.0f), 2.0f);   s = xc * G   (exact)
 *   2. f = the sum over k = K, K-1, ..., 1 of h[k-1] * e[n-k], from +0.0, in that DESCENDING order: the newest error enters last
 *      (the transposed form — acc[n+k] += h[k-1] * e[n] for every k once e[n] is known — is the same operations)
 *   3. w = s - f
 *   4. the dither d, from integers alone.  mix(u) on uint32_t: u ^= u >> 16; u *= 0x7feb352d; u ^= u >> 15; u *= 0x846ca68b;
 *      u ^= u >> 16.  k = mix(mix(t_n ^ seed) + q), t_n = t + n mod 2^32; r1 = k >> 16, r2 = k & 0xffff.
 *        S2R_DITHER_TRI:   d = (float)((int)r1 - (int)r2) * 2^-16
 *        S2R_DITHER_RECT:  d = (float)(2 * (int)r1 - 65535) * 2^-17
 *        S2R_DITHER_NONE:  d = +0.0
 *      (all exact in binary32)
 *   5. v = w + d;   r = rint(v), ties to even;   y = min(max(r, -G), G - 1);   the sample is (int32_t)y;   y != r counts as a clip
 *      of channel q
 *   6. e[n] = min(max(y - w, -2.0f), 2.0f)
 * Without a clip |y - w| < 1.5 and the clamp of step 6 is idle; with clips it keeps |f| <= 2 sum |h| and lets the loop recover
 * within K frames.  Every sample, the state and the clip counts are independent of how a stream is cut into calls.
 * A refused or failed call leaves state, t, samples and counts as they were.  Single-device handles (a device list refuses every
 * entry).  The first master fill that finds the stage set allocates the two copies of the state and pinned samples for
 * [9][max_frames][2] int32_t.
 *   s2r_set_master_pcm: S2R_ERR_PATCH_RANGE for bits, dither or n_taps out of range or a tap that is not finite or past 16 in
 *   magnitude (checked before the handle is looked at; nothing is changed); S2R_ERR_INVALID for NULL taps with n_taps > 0.  Resets
 *   state, t and counts, and drops the last samples.  s2r_clear_master_pcm: off.
 *   s2r_get_master_pcm: any pointer may be NULL; bits of 0 means off; taps receives S2R_PCM_MAX_TAPS floats, +0.0 past n_taps.
 *   s2r_reset_master_pcm: state, t and counts cleared and the last samples dropped, parameters kept; S2R_ERR_INVALID with the stage off.
 *   s2r_get_pcm: the [frames][2] samples of `programme` (< 9, else S2R_ERR_PATCH_RANGE) of the last successful master fill that
 *   ran the stage, into pcm_lr, which holds `capacity` int32_t (at least 2 * frames, else S2R_ERR_INVALID); *frames that fill's
 *   frames.  S2R_ERR_INVALID before any such fill, with the stage off or for NULL pcm_lr.
 *   s2r_get_pcm_clips: per channel, the clips of that fill (`last`) and since the set or reset (`held`, saturating); either may be NULL.
 *   s2r_get_pcm_state / s2r_set_pcm_state (checkpoints): the 162 floats and t; the getter takes a capacity of at least
 *   S2R_PCM_STATE, the setter exactly S2R_PCM_STATE, every value within [-2, 2] (S2R_ERR_PATCH_RANGE otherwise, for a NaN too);
 *   it keeps the first K entries of a row and stores +0.0 past them.  The setter moves the state and t alone: the last samples and
 *   both clip counts stay as they are, and a fresh handle that is given a checkpoint holds no samples and counts of 0.
 *   S2R_ERR_INVALID for a wrong size, a NULL buffer or with the stage off.
 *   s2r_pcm_reference: the device rule on the host (no device, no handle).  stems [n_buses][frames][2] (NULL with n_buses 0),
 *   master_lr [frames][2]; state[S2R_PCM_STATE] and *t updated in place; pcm [9][frames][2]; clips[18] receives the call's counts
 *   (may be NULL).  S2R_ERR_PATCH_RANGE as the two setters', and for n_buses > 8; S2R_ERR_INVALID for a NULL.
 *   s2r_pcm_dither: step 4 alone, *d for one t_n and q (< 18) and kind.
 *   s2r_pcm_pack: `count` samples of `bits` bits into containers of bytes_per_sample 2, 3 or 4 bytes: little-endian, two's
 *   complement, left-justified in the container (sample << (8 * bytes_per_sample - bits)) as WAV wants; out holds
 *   count * bytes_per_sample bytes.  S2R_ERR_PATCH_RANGE for bits out of range, another container, one narrower than bits, or a
 *   sample outside [-2^(bits-1), 2^(bits-1) - 1] (nothing is written past the samples in front of it).
 *   s2r_pcm_shaper: the taps of `kind` into taps[S2R_PCM_MAX_TAPS] (+0.0 past *n_taps): S2R_SHAPER_FLAT {}; S2R_SHAPER_FIRST {1};
 *   S2R_SHAPER_SECOND {2, -1}; S2R_SHAPER_3TAP {1.623, -0.982, 0.109}; S2R_SHAPER_5TAP {2.033, -2.165, 1.959, -1.590, 0.6149};
 *   S2R_SHAPER_9TAP {2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847} — the last three the commonly quoted
 *   psychoacoustic error-feedback sets for 44.1 kHz, each decimal rounded to nearest binary32. */
#define S2R_PCM_PROGRAMMES 9u
#define S2R_PCM_CHANNELS 18u
#define S2R_PCM_MAX_TAPS 9u
#define S2R_PCM_STATE (S2R_PCM_CHANNELS * S2R_PCM_MAX_TAPS)
#define S2R_PCM_MIN_BITS 8u
#define S2R_PCM_MAX_BITS 24u
#define S2R_PCM_MAX_TAP 16.0f
#define S2R_DITHER_NONE 0u
#define S2R_DITHER_RECT 1u
#define S2R_DITHER_TRI 2u
#define S2R_SHAPER_FLAT 0u
#define S2R_SHAPER_FIRST 1u
#define S2R_SHAPER_SECOND 2u
#define S2R_SHAPER_3TAP 3u
#define S2R_SHAPER_5TAP 4u
#define S2R_SHAPER_9TAP 5u
int s2r_set_master_pcm(s2r_synth *s, uint32_t bits, uint32_t dither, const float *taps, uint32_t n_taps, uint32_t seed);
int s2r_clear_master_pcm(s2r_synth *s);
int s2r_get_master_pcm(const s2r_synth *s, uint32_t *bits, uint32_t *dither, float *taps, uint32_t *n_taps, uint32_t *seed);
int s2r_reset_master_pcm(s2r_synth *s);
int s2r_get_pcm(const s2r_synth *s, uint32_t programme, int32_t *pcm_lr, size_t capacity, size_t *frames);
int s2r_get_pcm_clips(const s2r_synth *s, uint32_t *last, uint32_t *held);
int s2r_get_pcm_state(s2r_synth *s, float *state, size_t capacity, uint32_t *t);
int s2r_set_pcm_state(s2r_synth *s, const float *state, size_t count, uint32_t t);
int s2r_pcm_reference(uint32_t bits, uint32_t dither, const float *taps, uint32_t n_taps, uint32_t seed, const float *stems,
                      uint32_t n_buses, const float *master_lr, uint32_t frames, float *state, uint32_t *t, int32_t *pcm,
                      uint32_t *clips);
int s2r_pcm_dither(uint32_t seed, uint32_t t, uint32_t q, uint32_t kind, float *d);
int s2r_pcm_pack(const int32_t *pcm, size_t count, uint32_t bits, uint32_t bytes_per_sample, uint8_t *out);
int s2r_pcm_shaper(uint32_t kind, float *taps, uint32_t *n_taps);

/* BUILD-DEFINED master sample-rate converter (the reference renders at one rate): a polyphase FIR resampler by the
 * rational ratio L / M of every bus and of the master, behind the spectrum meters and in front of the PCM stage, in s2r_fill_master
 * and in no other fill.  Off by default, and a handle on which the stage was never set launches exactly what it launched before and
 * allocates nothing; master_lr, the stems, the loudness rows and the spectrum rows are the same bits with the stage on or off.
 * PROGRAMMES: S2R_RESAMPLER_PROGRAMMES = 9, the meters' and the PCM stage's: programme b < 8 is bus b as the stems hold it, programme 8
 * the master as the caller receives it.  Channel q = 2 p + c, 18 of them.  A bus at or past the call's n_buses is fed +0.0; its
 * history still rings out.
 * PARAMETERS: L and M each in 1 .. S2R_RESAMPLER_MAX_FACTOR (320), gcd(L, M) == 1, L <= 4 M and M <= 4 L: the output rate is L / M
 * of the input's.  T, the taps per phase: a multiple of 4 in 4 .. S2R_RESAMPLER_MAX_TAPS (128), with L * T <= S2R_RESAMPLER_MAX_TABLE
 * (24 576).  The table h[L][T] is the caller's (s2r_resampler_design makes one): every entry finite and at most 4 in magnitude.  One
 * table serves all 18 channels.
 * STATE carried from call to call: S2R_RESAMPLER_STATE(T) = 18 * (T - 1) floats, row q = the channel's last T - 1 input frames,
 * NEWEST first; and ph, the position of the next output in units of 1 / L input frame, counted from the first frame of the next
 * call: 0 <= ph < M after any call.  All +0.0 / 0 right after a set or a reset.
 * DEVICE RULE, binary32, every operation rounded on its own, no fma, denormals kept, NaN and infinities as the operations have them.
 * Per call of F frames, x[n] the channel's frame n of the call and x[-j] its history's entry j - 1:
 *   1. count = 0 if F * L <= ph, else ceil((F * L - ph) / M): the call's output frames
 *   2. for output i < count: u = ph + i * M;  n = u / L;  p = u % L   (64-bit integers)
 *   3. four accumulators a_0 .. a_3 from +0.0; for k = 0, 1, ..., T - 1 in ascending order: a_(k % 4) = a_(k % 4) + h[p][k] * x[n - k]
 *   4. y[i] = (a_0 + a_1) + (a_2 + a_3)
 *   5. ph' = ph + count * M - F * L; the new history is the last T - 1 frames of the history followed by the call
 * The four chains and the final tree are part of the rule: they are four independent dependency chains for the kernel.  Every output
 * frame, the state and ph are independent of how a stream is cut into calls.  A call makes at most
 * S2R_RESAMPLER_MAX_OUT(frames, L, M) = ceil(frames * L / M) + 1 output frames.
 * A resampled signal can exceed the limiter's ceiling between the original samples: with the sample-peak detector the limiter bounds
 * the samples it is given, not the band-limited curve through them, and the excess can be several dB; with the true-peak detector
 * (s2r_set_master_limiter_ex) it bounds a 4x interpolation of them, and the excess is what that section records, under a percent
 * at a lookahead of 16 frames or more.  The PCM stage behind clamps a sample past full scale and counts it as a clip.
 * WITH THE PCM STAGE ON TOO, its kernel runs on the resampler's output: all eight buses and the master, `count` frames a call, t
 * counting output frames; its integers, state, t and clips are exactly s2r_pcm_reference over s2r_resampler_reference's nine
 * programmes with n_buses = 8.  A call with count == 0 launches no PCM kernel: its state, t and held clips stay, and s2r_get_pcm
 * answers 0 frames.  The PCM stage's pinned samples are sized for S2R_RESAMPLER_MAX_OUT(max_frames, L, M) frames then, and grown by a
 * later fill that finds them short (which drops the samples of the last fill).  With the resampler off the PCM stage is as it was.
 * A refused or failed call leaves table, state, ph and the last outputs as they were.  Single-device handles (a device list refuses
 * every entry).  The first master fill that finds the stage set allocates the device's copy of the table, the two copies of the state
 * and pinned outputs for [9][S2R_RESAMPLER_MAX_OUT(max_frames, L, M)][2] floats; a later fill that finds them short grows them.
 *   s2r_set_master_resampler: S2R_ERR_PATCH_RANGE for L, M or T out of range or a table entry that is not finite or past 4 in
 *   magnitude (checked before the handle is looked at; nothing is changed); S2R_ERR_INVALID for a NULL table.  Resets state and ph
 *   and drops the last outputs.  s2r_clear_master_resampler: off.
 *   s2r_get_master_resampler: any pointer may be NULL; L of 0 means off; table receives L * T floats (at most
 *   S2R_RESAMPLER_MAX_TABLE: ask for L and T first).
 *   s2r_reset_master_resampler: state and ph cleared and the last outputs dropped, parameters kept; S2R_ERR_INVALID with the stage off.
 *   s2r_get_resampled: the [frames][2] outputs of `programme` (< 9, else S2R_ERR_PATCH_RANGE) of the last successful master fill that
 *   ran the stage, into out_lr, which holds `capacity` floats (at least 2 * frames, else S2R_ERR_INVALID); *frames that fill's count,
 *   which may be 0.  S2R_ERR_INVALID before any such fill, with the stage off or for NULL out_lr.
 *   s2r_get_resampler_state / s2r_set_resampler_state (checkpoints): the floats and ph; the getter takes a capacity of at least
 *   S2R_RESAMPLER_STATE(T), the setter exactly that many floats — any values, non-finite ones too — and ph < M (S2R_ERR_PATCH_RANGE
 *   otherwise).  S2R_ERR_INVALID for a wrong size, a NULL buffer or with the stage off.  The setter moves the state and ph alone: the
 *   last outputs stay as they are, and a fresh handle that is given a checkpoint holds none.
 *   s2r_resampler_reference: the device rule on the host (no device, no handle).  stems [n_buses][frames][2] (NULL with n_buses 0),
 *   master_lr [frames][2]; state[S2R_RESAMPLER_STATE(T)] and *ph updated in place; out [9][capacity][2] receives *count frames of
 *   every programme.  S2R_ERR_PATCH_RANGE as the setter's, for n_buses > 8 and for *ph >= M; S2R_ERR_INVALID for a NULL or a
 *   capacity below the call's count (nothing is written or changed then).
 *   s2r_resampler_count: step 1 alone into *count; S2R_ERR_PATCH_RANGE for L or M out of range or ph >= M.
 *   s2r_resampler_design: a Kaiser-windowed sinc, computed in binary64.  N = L T, c = (N - 1) / 2, fc = rolloff * 0.5 / max(L, M);
 *   g[i] = 2 fc L sinc(2 fc (i - c)) * kaiser(i; N, beta), sinc(x) = sin(pi x) / (pi x), kaiser(i) = I0(beta sqrt(1 - ((i - c) / c)^2))
 *   / I0(beta); h[p][k] = g[k L + p]; every row is divided by its own sum, so that no phase has a DC error, and then rounded to
 *   binary32.  The filter delays by (L T - 1) / (2 L) input frames.  beta in [0, 20], rolloff in (0, 1], else S2R_ERR_PATCH_RANGE. */
#define S2R_RESAMPLER_PROGRAMMES 9u
#define S2R_RESAMPLER_CHANNELS 18u
#define S2R_RESAMPLER_MAX_FACTOR 320u
#define S2R_RESAMPLER_MIN_TAPS 4u
#define S2R_RESAMPLER_MAX_TAPS 128u
#define S2R_RESAMPLER_MAX_TABLE 24576u
#define S2R_RESAMPLER_MAX_TAP 4.0f
#define S2R_RESAMPLER_STATE(T) (S2R_RESAMPLER_CHANNELS * ((T) - 1u))
#define S2R_RESAMPLER_MAX_OUT(frames, L, M) (((uint64_t)(frames) * (L) + (M) - 1u) / (M) + 1u)
int s2r_set_master_resampler(s2r_synth *s, uint32_t L, uint32_t M, uint32_t T, const float *table);
int s2r_clear_master_resampler(s2r_synth *s);
int s2r_get_master_resampler(const s2r_synth *s, uint32_t *L, uint32_t *M, uint32_t *T, float *table);
int s2r_reset_master_resampler(s2r_synth *s);
int s2r_get_resampled(const s2r_synth *s, uint32_t programme, float *out_lr, size_t capacity, size_t *frames);
int s2r_get_resampler_state(s2r_synth *s, float *state, size_t capacity, uint32_t *ph);
int s2r_set_resampler_state(s2r_synth *s, const float *state, size_t count, uint32_t ph);
int s2r_resampler_reference(uint32_t L, uint32_t M, uint32_t T, const float *table, const float *stems, uint32_t n_buses,
                            const float *master_lr, uint32_t frames, float *state, uint32_t *ph, float *out, size_t capacity,
                            size_t *count);
int s2r_resampler_count(uint32_t L, uint32_t M, uint32_t ph, uint32_t frames, size_t *count);
int s2r_resampler_design(uint32_t L, uint32_t M, uint32_t T, double beta, double rolloff, float *table);

/* BUILD-DEFINED 4x oversampling (the reference has none; BASELINE config [4]): renders 4 * frames at
 * 4 * sample_rate_hz through the same path and decimates the mix by a 63-tap windowed sinc whose history
 * carries over from call to call (DESIGN.md 4.9 gives taps and arithmetic).  4 * frames must not exceed
 * max_frames.  Voices' offsets, envelopes and filters all run at the oversampled rate. */
#define S2R_OVERSAMPLE 4u
int s2r_fill_oversampled(s2r_synth *s, float *mono_out, size_t frames, uint32_t sample_rate_hz);

/* Multi-GPU building block: renders this shard and leaves its PARTIAL mix (no root add) in
 * `dev_partial_out` (device memory, `frames` floats) on `hip_stream` (a hipStream_t, may
 * be NULL) without synchronising.  Partials of all shards are then combined in rank order
 * by s2r_sum_partials_device. */
int s2r_fill_device(s2r_synth *s, float *dev_partial_out, size_t frames, uint32_t sample_rate_hz, void *hip_stream);
/* Single-shard form of the above: the FINAL mix (root-added, exactly what s2r_fill returns)
 * left in device memory on `hip_stream`, no synchronisation. */
int s2r_fill_device_root(s2r_synth *s, float *dev_out, size_t frames, uint32_t sample_rate_hz, void *hip_stream);
/* out[i] = ((+0.0 + rows[0][i]) + rows[1][i]) + ...   rows is [n_rows][frames] on device. */
int s2r_sum_partials_device(const float *dev_rows, uint32_t n_rows, size_t frames, float *dev_out, void *hip_stream);

/* Mix disabled: every shard voice's frames, host array [shard_voices][frames] (rows of idle
 * voices are +0.0).  Advances state exactly like s2r_fill.  process::process_layer_buf_simd
 * per voice (process.rs:14-49). */
int s2r_render_voices(s2r_synth *s, float *per_voice_out, size_t frames, uint32_t sample_rate_hz);

/* The reference's lower-level public entry for callers that keep their own st::Layer:
 *   process::process_layer_buf_simd(&sc::Layer, &mut st::Layer, Hz, SampleRateKhz, offset: u32, release_offset: Option<u32>, &mut [f32])
 * (process.rs:14-49, pub through try3/mod.rs) — whole 16-frame chunks through process_layer_x16, the remainder through the
 * scalar path, the state advanced in place, the offset passed by value — for n_layers independent layers side by side.
 * static_config = the handle's patch (s2r_set_patch / s2r_load_patch; `program` picks a bank entry); bufs is [n_layers][frames].
 * The handle is the workspace: its first n_layers voices are replaced by the layers (at offset + frames afterwards), the
 * rest go idle — give the calls a handle of their own, sized to the batch (one device, n_layers <= total_voices).
 * S2R_ERR_OFFSET_OVERFLOW where the reference panics (process.rs:36). */
typedef struct {
    float pitch_hz;                /* Hz */
    uint32_t offset;               /* frames since the layer's note_on; by value: the caller adds `frames` (synth.rs:197) */
    uint32_t release_offset;       /* valid when has_release */
    uint8_t has_release;           /* Option<u32>::is_some() */
    uint8_t program;               /* patch bank index (0 without a bank) */
    uint8_t _pad[2];
    /* st::Layer (state.rs:10-21), updated in place */
    float phase_accum;             /* OscillatorState */
    float lpf_last;                /* LowPassFilterState.last */
    uint32_t noise_seed;           /* NoiseState.seed */
    float filt_x1, filt_x2, filt_y1, filt_y2;   /* dsp_filters.rs kinds / SVF */
    float osc_z;                   /* DPW oscillators (NaN: none yet) */
} s2r_layer_call;
int s2r_process_layers(s2r_synth *s, s2r_layer_call *layers, uint32_t n_layers, float *bufs, size_t frames, uint32_t sample_rate_hz);

/* Checkpoint / resume and test access; `voices` has shard_voices entries. */
int s2r_export_state(s2r_synth *s, s2r_voice_state *voices);
int s2r_import_state(s2r_synth *s, const s2r_voice_state *voices);
/* NoiseState.seed of one pool voice ("todo don't default this", state.rs:19). */
int s2r_set_noise_seed(s2r_synth *s, uint32_t voice_index, uint32_t seed);

/* Synth::next_voice's `log::debug!("using new voice index {} for note {}", …)` (synth.rs:118) as a callback: called once
 * per note_on (s2r_note_on, s2r_note_on_ex, every note_on of s2r_note_events, in event order) with the voice the allocation
 * policy chose.  NULL switches it off (the default).  Not on the shards of a device list (their parent's pool decides). */
typedef void (*s2r_voice_log_fn)(void *user, uint32_t voice_index, uint8_t note);
int s2r_set_voice_log(s2r_synth *s, s2r_voice_log_fn fn, void *user);

/* Introspection */
uint32_t s2r_abi_version(void);
/* Which sources this binary was built from: "<sha256 over synth2_amd/csrc, 16 hex>-<include/s2r.h + compiler flags, 8 hex>",
 * compiled in by synth2_amd/build.py.  A loader that has the sources at hand (synth2_amd.load_library, bench.py) compares it
 * with their hash and refuses — or rebuilds — a binary that does not match, whatever the files' times say; bench.py prints it
 * beside the profile's source hash.  (No counterpart in the reference: cargo rebuilds s2_lib from source.) */
const char *s2r_build_id(void);
uint32_t s2r_shard_voices(const s2r_synth *s);
uint32_t s2r_block_voices(const s2r_synth *s);
uint32_t s2r_device_count(const s2r_synth *s);                  /* 1, or the N of a device list */
/* note_offs that found no active (started, unreleased) voice holding the note and therefore did nothing.  The
 * reference ignores them silently: its `log::warn!("note {} released twice")` (synth.rs:77) sits behind
 * find_active_voice, which only returns unreleased voices (synth.rs:36-38,82-90), so it can never fire — this
 * counter is the diagnostic that warning was meant to be. */
uint64_t s2r_double_release_count(const s2r_synth *s);
/* Low-latency fills for the reference's own call pattern — a small pool rendered 16 frames at a time from the audio
 * callback (synth.rs:154-203 called per 16 frames, s2_bin/src/main.rs:138-147, audio_player.rs:56-60).  Enabled, a handle
 * whose shard is ONE workgroup (at most 256 voices, block_voices permitting) with a single one-pole patch keeps a resident
 * render kernel on the device between s2r_fill / s2r_fill_stereo calls: a fill is then a command written to mapped host
 * memory and a completion word (for fills of up to 64 frames: the tags of the frames themselves) polled, not a kernel
 * launch.  The kernel leaves by itself after 1 ms
 * without a fill (the next fill starts it again) and is stopped by every other entry point that touches the device or
 * the patch; fills it cannot take (timed events, more than 9 note events since the last fill, seed overrides) go the
 * ordinary way.  Same bits either way.  While it runs it occupies one compute unit and the handle's stream.
 * s2r_low_latency_active: 1 while the resident kernel is believed to be on the device. */
int s2r_set_low_latency(s2r_synth *s, int enabled);
int s2r_low_latency_active(const s2r_synth *s);
/* The same idea for the THROUGHPUT path: keep the shard's whole render grid on the device between fills.
 * Enabled, a handle (or every shard of a device-list handle) whose grid is at most one workgroup of at most 256 voices per
 * compute unit — any patch, any patch bank — renders the fills of s2r_fill / s2r_fill_stereo / s2r_fill_begin through a
 * POOL-RESIDENT kernel: a fill is a 64-byte command plus the fill's note events grouped by workgroup, written to memory the
 * kernel polls — no launch; every workgroup builds its own voices' event chains, renders, and the last ones to finish add
 * the rows up and end the fill (one workgroup per fill, for a device list, also adds the shards' rows).  With two fills in
 * flight a workgroup that is done early starts the next fill while the slowest still finish this one.  The kernel leaves by
 * itself after 2 ms without a fill (the next fill starts it again) and is stopped by every entry point that touches the
 * device, the patch or a knob, and by s2r_quiesce; fills it cannot take (per-voice rows, caller-owned streams, timing
 * on, the 4x-oversampled fill) go the ordinary way.  Same bits either way.  While it runs it holds the handle's stream
 * and one workgroup slot per 256 voices: enable it for ONE handle per device, on a device the caller does not share.
 * A single-workgroup handle gets s2r_set_low_latency's kernel.  (The reference's Synth is a value on the audio thread's
 * stack, synth.rs:9-12: it is always "resident".)
 * s2r_resident_active: 1 while a resident kernel of either kind is believed to be on the device.
 * s2r_quiesce: stops any resident kernel of the handle and waits for it — what a caller does before it synchronises the
 * whole device (hipDeviceSynchronize would otherwise wait out the kernel's patience). */
/* One process per GPU WITHOUT a collective library in the step (SURVEY 8e's preferred shape): the ranks' partial rows are
 * written into one block of the root's device memory — mapped by the other ranks through an IPC handle; a peer-to-peer store
 * over xGMI where the ranks' devices differ — and added in rank order from +0.0 (synth.rs:176,195) by the root's last
 * workgroup, all inside the render kernels.  Rank 0 calls s2r_exchange_create on its shard's handle and hands the 64 handle
 * bytes to the other ranks by whatever channel the caller has (once, at start-up); they call s2r_exchange_attach.  From
 * then on every rank drives its handle with the SAME events and the same s2r_fill / s2r_fill_begin / s2r_fill_end calls;
 * the root's buffers receive the mix, the other ranks' buffers silence.  Bit for bit what one device returns with
 * mix_groups = n_ranks (contiguous shards).  Shards of more than one workgroup; any patch or patch bank. */
#define S2R_EXCHANGE_HANDLE_BYTES 64
int s2r_exchange_create(s2r_synth *s, uint32_t n_ranks, void *handle_out, size_t handle_bytes);
int s2r_exchange_attach(s2r_synth *s, uint32_t rank, uint32_t n_ranks, const void *handle, size_t handle_bytes);
int s2r_set_resident(s2r_synth *s, int enabled);
int s2r_resident_active(const s2r_synth *s);
int s2r_quiesce(s2r_synth *s);
/* device time of the most recent fill's render kernel in milliseconds (HIP events recorded
 * on the library's stream around the launch); < 0 if timing is off.  Enable with
 * s2r_set_timing(s, 1): adds two event records per fill. */
int s2r_set_timing(s2r_synth *s, int enabled);
/* Measurement knob (default on): while the mod envelope of every voice of a wavefront is in a
 * flat stage the LPF coefficient is reused instead of recomputed — same bits either way.
 * Turning it off makes every frame pay the full pow/exp chain (bench.py's
 * `value_all_voices_modulating` leg). */
int s2r_set_flat_shortcut(s2r_synth *s, int enabled);
/* Measurement knob (default 1): where a patch's filter coefficients come from while a mod envelope moves.
 * 0: computed in-lane per frame; 1: read from the patch's coefficient tables, and a fill with few
 * untimed events carries them in the render kernel's arguments; 2: tables, but note events always through their
 * own launch; 3 / 4: synonyms of 1 / 2 (earlier rounds' test matrices).  Same bits in every mode. */
int s2r_set_coeff_stream(s2r_synth *s, int enabled);
/* Measurement knob (default on): a wavefront whose 64 voices were started together with one patch reads its chunks'
 * filter coefficients, amplitudes and noise from a window in LDS that it fills once per run, instead of computing them
 * on every lane (launch-per-fill form, fills of up to 1024 frames, pools of at most one 256-voice
 * workgroup per compute unit).  Same bits either way. */
int s2r_set_uniform_window(s2r_synth *s, int enabled);
/* How many 16-frame chunks (per wavefront) the handle's fills have rendered through that window since it was created:
 * tells a test, or a profile, whether the path was taken.  Waits for the fills in flight. */
int s2r_uniform_window_chunks(s2r_synth *s, uint64_t *chunks);
float s2r_last_render_ms(s2r_synth *s);
const char *s2r_last_error(const s2r_synth *s);             /* never NULL */
const char *s2r_status_string(int status);

/* ---- host-only helpers: usable without a device (front-ends that route events to shards,
 * CPU-only tests of the host logic) ---- */

/* The wire format of the reference's (disabled) websocket audio server, one text frame per buffer:
 * serde_json::to_string(&Vec<f32>) (threads.rs:303-305; BUFFER_SIZE = 4096 frames, 32 kHz mono,
 * threads.rs:6,263; consumer www/streamer.js:82-90).  Writes a NUL-terminated JSON array into `out`
 * and returns its length; when `out` is NULL or `cap` is below the worst case (3 + S2R_STREAM_CHARS_PER_SAMPLE * n:
 * the longest element, e.g. "-0.0000012345678", is 16 chars + ','; one spare) it writes nothing and returns the capacity to provide.  Host-only. */
#define S2R_STREAM_CHARS_PER_SAMPLE 18u
#define S2R_STREAM_FRAMES 4096u
#define S2R_STREAM_RATE_HZ 32000u
size_t s2r_stream_frame_json(const float *samples, size_t n, char *out, size_t cap);

/* The .synth2 parser on its own; err_buf (may be NULL) receives a message on failure. */
int s2r_parse_patch_text(const char *text, size_t len, s2r_patch *out, char *err_buf, size_t err_cap);

/* The pan a note_on gives its voice, and the constant-power gains of a pan.  binary32, every operation
 * rounded on its own:  k = (float)((int)note - 64) * 0.015625f;  p = pan + key_spread * k, clamped to [-1, 1];
 * gL = sqrtf((1 - p) * 0.5f), gR = sqrtf((1 + p) * 0.5f): the centre gives sqrt(0.5) on both sides, p = -1 gives (1, 0). */
float s2r_voice_pan(float pan, float key_spread, uint8_t note);
void s2r_pan_gains(float p, float *gl, float *gr);

/* The gain a note_on gives its voice.  binary32, every operation rounded on its own, no fma:
 *   u = velocity < 1.0f ? velocity : 1.0f  (NaN -> 1);  u = u > 0.0f ? u : 0.0f;  a = 1.0f - velocity_sens * (1.0f - u);
 *   w = level * a.   w == 1.0f exactly for level 1, sensitivity 0, any velocity. */
float s2r_voice_gain(float level, float velocity_sens, float velocity);

/* The two gains of a voice with pan `pan` and gain `w` under a program fader pair.  binary32, every operation
 * rounded on its own, no fma:  q = pan + pan_shift, clamped to [-1, 1] (q < -1 ? -1 : q > 1 ? 1 : q);
 * (aL, aR) = s2r_pan_gains(q);  gL = (aL * w) * fader, gR = (aR * w) * fader.  With fader 1 and shift 0: aL * w, aR * w exactly.
 * Either pointer may be NULL. */
void s2r_fader_gains(float pan, float w, float fader, float pan_shift, float *gl, float *gr);

/* The gain of a voice's aux send: g * send, one rounded binary32 multiply. */
float s2r_send_gain(float g, float send);

/* The voice-allocation / release policy of Synth (synth.rs:61-120) for a pool of any size,
 * O(1) per event, without rendering.  Offsets advance by s2r_voice_pool_advance. */
typedef struct s2r_voice_pool s2r_voice_pool;
s2r_voice_pool *s2r_voice_pool_create(uint32_t total_voices);
void s2r_voice_pool_destroy(s2r_voice_pool *p);
uint32_t s2r_voice_pool_note_on(s2r_voice_pool *p, uint8_t note, float velocity);  /* returns the chosen index */
int64_t s2r_voice_pool_note_off(s2r_voice_pool *p, uint8_t note);                  /* released index or -1 */
void s2r_voice_pool_advance(s2r_voice_pool *p, uint64_t frames);
uint32_t s2r_voice_pool_next_voice(const s2r_voice_pool *p);                       /* synth.rs:101-120 */
/* The batch form s2r_note_events runs: the whole array at once — what a loop of s2r_voice_pool_advance (to each event's
 * frame) / _note_on / _note_off computes, with the same results, voice_out[k] = the voice event k takes or releases (-1: a
 * note_off that found none, a program change).  `frames_moved`: how far the clock already is inside the fill the events belong
 * to; returns the last event's frame.  s2r_voice_pool_set_threads: batches of at least `batch_threshold` events are resolved
 * by the calling thread (the queue: synth.rs:101-120 depends on earlier note_ons alone) plus `worker_threads` threads that
 * share the notes among them (synth.rs:82-90 depends on one note's events alone); 0 = the calling thread alone. */
void s2r_voice_pool_set_threads(s2r_voice_pool *p, uint32_t worker_threads, size_t batch_threshold);
uint32_t s2r_voice_pool_resolve(s2r_voice_pool *p, const s2r_note_event *events, size_t n, uint32_t frames_moved, int64_t *voice_out);
int s2r_voice_pool_query(const s2r_voice_pool *p, uint32_t voice_index, s2r_voice_state *out);

#ifdef __cplusplus
}
#endif
#endif /* S2R_H */
