// s2r_device.h — kernel argument blocks and launch entry points shared by the host side
// (s2r_host.cpp) and the gfx950 kernels (s2r_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "s2r.h"

// voice flag bits (synth.rs:27-28: the two Option discriminants)
#define S2R_VF_STARTED 1u    // current_frame_offset.is_some()
#define S2R_VF_RELEASED 2u   // release_frame_offset.is_some()

// One ADSR resolved for a sample rate.  A, D, R are `Ms::as_samples` (units.rs:44-53);
// the three slopes are the `y_rise / x_run` of simdtest.rs:247-251, hoisted out of the
// per-frame work (a correctly rounded division gives the same bits wherever it runs).
struct S2rEnv {
    float A;          // attack (samples) == decay_offset
    float D;          // decay (samples)
    float S;          // sustain level
    float R;          // release (samples)
    float sus_off;    // A + D                         simdtest.rs:282
    float slope_att;  // 1.0 / A                       simdtest.rs:295-299
    float slope_dec;  // (S - 1.0) / D                 simdtest.rs:303-307
    float slope_rel;  // (-S) / R                      simdtest.rs:313-317
};

// Per-voice state, struct-of-arrays in HBM (one entry per shard voice, padded to a whole
// number of workgroups).  28 B are read and 12 B written per started voice per fill
// (+16 B each way under the second-order filters).
struct S2rVoiceArrays {
    float *pitch;         // note_to_pitch(note)             synth.rs:179,208-212
    uint32_t *offset;     // current_frame_offset            synth.rs:27
    uint32_t *release;    // release_frame_offset            synth.rs:28
    uint32_t *flags;      // S2R_VF_*
    float *phase;         // OscillatorState.phase_accum     oscillators.rs:402-406
    float *lpf_last;      // LowPassFilterState.last         filters.rs:5-7
    uint32_t *seed;       // NoiseState.seed                 state.rs:17-21
    // dsp_filters.rs:12-17,82-89 states; only touched by patches with lpf.kind != onepole
    float *fx1, *fx2, *fy1, *fy2;
    uint32_t *program;    // index into the patch bank the voice was started with (0 without a bank)
    float *osc_z;         // DPW oscillators: the differentiator's memory F(s[n-1]); NaN in a voice that has not rendered a frame
};
#define S2R_VOICE_WORDS 13
#define S2R_OSC_Z_NONE 0x7fc00000u   // the bits of that NaN

// One patch of the bank, resolved for the fill's sample rate (what S2rRenderParams carries for
// the single-patch kernels).
struct S2rBankEntry {
    int32_t osc_kind;
    float osc_gain, noise_level, lpf_freq, amt_osc, amt_lpf;
    int32_t lpf_kind;
    float lpf_shape;      // damping_factor (LP2/HP2) or quality_factor (BP2)
    S2rEnv amp, mod;
    // this patch's coefficient tables (S2rTabRef with `base` = the bank's table buffer + tab_off floats); always four
    // planes: c0, c1, c2 (x, 1 - x, - for the one-pole; alpha, beta, gamma otherwise), pow(2, mod * amt_osc)
    uint32_t tab_valid;   // 0: envelopes too long to tabulate — the voices of this patch compute in-lane
    uint32_t tab_off, tab_plane;
    int32_t tab_ad, tab_rc;
    uint32_t tab_rc_t0;
    int32_t tab_ru, tab_sus, tab_end, tab_dead;
};

struct S2rTimedEvent;

// How the LAST kernel of a fill tells the host that the output (in mapped host memory) is complete: the last workgroup
// to finish (a counter in device memory, reset by that workgroup) stores `value` into a word of mapped host memory the
// host polls — a few hundred nanoseconds after the data, where waiting on a HIP event costs the caller tens of
// microseconds between the GPU finishing and the wait returning.  flag == nullptr: nothing is signalled.
struct S2rDone {
    uint32_t *flag;          // mapped host memory (device view)
    uint32_t value;
    uint32_t *counter;       // device memory, 0 between launches
};

// Coefficient tables of ONE patch at one sample rate.  The x16 ADSR (old/simdtest.rs:270-331) makes
// the mod envelope's value a function of the frame offset t alone while the voice is in its attack or decay stage
// (the release offset is clamped to attack + decay, simdtest.rs:283), of t alone in a release that starts at that
// clamp, and of d = t - release_offset alone in a later release; in sustain and after the end it is a constant.  So
// the chain behind it — sleef pow -> * freq -> filter coefficients (process.rs:146-152,231-250; filters.rs:20-24 or
// dsp_filters.rs) — is tabulated once per (patch, sample rate) by s2r_table_kernel with the very routines the render
// kernels would run per voice and frame, and a voice reads its coefficients at base[idx + (offset & mask)].
// Planes (each `plane` floats apart): one-pole: x = exp(-2 pi f / sr), 1 - x; dsp_filters.rs kinds / SVF: alpha,
// beta, gamma; then, under oscillator FM, pow(2, mod * mod_env_to_osc_freq).
// Valid for offsets below 2^24 (where (offset as f32) is exact); older voices compute in-lane.
struct S2rTabRef {
    const float *base;    // plane 0, entry 0; nullptr: no tables (too long an envelope, or switched off)
    uint32_t plane;       // floats per plane
    int32_t ad;           // attack + decay:      entry ad + t,              0 <= t < attack + decay
    int32_t rc;           // release at the clamp: entry rc + (t - rc_t0),   rc_t0 = ceil(attack + decay)
    uint32_t rc_t0;
    int32_t ru;           // later release:       entry ru + (t - release_frame_offset)
    int32_t sus;          // 16 equal entries: the sustain stage's constant
    int32_t end;          // 16 equal entries: after the release
    int32_t dead;         // 16 equal entries: x = 1, 1 - x = 0 — what makes a lane without a started voice put +0.0
                          // into the mix without a select (one-pole kernel)
    uint32_t fm_plane;    // index of the pow(2, mod * mod_env_to_osc_freq) plane (2 or 3), 0 = none
};
#define S2R_TAB_PAD 16u          // entries a 16-frame chunk may read past a region's last used one
#define S2R_TAB_MAX_ENTRIES (1u << 22)

// ONE launch per fill.  The render kernel does the two small jobs that used to be launches of their own:
//   * chain heads: the host hands over the fill's timed-event records GROUPED BY WORKGROUP (mapped host memory) with the
//     groups' bounds; every workgroup copies its own slice into HBM and publishes its own voices' chain heads before it
//     loads its state — nobody waits for anybody;
//   * the mix ("ticket mix"): a workgroup that has written its partial row counts itself in on `arrive`; the LAST
//     `n_mixers` to arrive wait for the very last one (bounded: they are the fill's slowest workgroups, and every workgroup
//     they wait for is already running) and add the rows up in the documented order, 16-frame blocks dealt
//     out among them; the last mixer to finish ends the fill: the completion word, or — a shard of a device list / of a
//     group of processes — one more count on `rows_done` in the root's memory: the shard that counts in LAST adds the
//     shards' rows in shard order from +0.0 (synth.rs:176,195) and ends the fill.  No wait anywhere in that.
struct S2rMixTail {
    uint32_t n_mixers;            // 0: no in-kernel mix (the rows are left for s2r_mix_kernel)
    uint32_t n_blocks, blocks_per_group, n_groups;
    int32_t root_add, stereo;
    float *out;                   // the fill's output (root_add) or this shard's partial row
    S2rDone done;                 // counter: the mixers' own arrival; flag/value: the completion word (no exchange)
    // exchange of partial rows between shards (device list, one process per GPU): nullptr = none
    uint32_t *rows_done;          // counter in the root's memory (system scope)
    uint32_t rows_target;         // value it has when every shard has counted in for this fill
    int32_t xmode;                // 0: the shard that counts in last adds the rows; 1: this shard is the ROOT of a group of
                                  // processes: it waits for every rank and adds the rows; 2: a rank other than the root
    uint32_t n_rows, row_stride;
    const float *rows;            // [n_rows][row_stride], the root's
    float *final_out;
    S2rDone final_done;
    int32_t final_stereo;
    unsigned long long *granules; // != nullptr: the fill's output goes out as tagged 8-byte words instead (mono; no completion word)
    uint32_t granule_tag;
};

struct S2rRenderParams {
    // patch (static_config.rs:4-44), shared by every voice
    int32_t osc_kind;
    float osc_gain;
    float noise_level;
    float lpf_freq;
    float amt_osc;        // mod_env_to_osc_freq
    float amt_lpf;        // mod_env_to_lpf_freq
    int32_t lpf_kind;     // s2r_filter_kind; != 0 renders through s2r_render_dspf_kernel
    float lpf_damping;    // damping_factor (LP2/HP2) or quality_factor (BP2)
    S2rEnv amp;
    S2rEnv mod;
    float sr;             // sample_rate as f32 (units.rs:21)
    float rcp_sr;         // RN(1/sr)
    int32_t fast_div_sr;  // 1 => x/sr may use the 3-op exact quotient (rate verified exhaustively)
    int32_t no_flat_shortcut;  // 1 => always recompute the filter coefficient per frame, in-lane (measurement knob)
    uint32_t frames;      // this fill
    uint32_t n_voices;    // shard voices
    uint32_t frames_stride; // row stride of block_partials / per_voice (== max_frames or frames)
    uint32_t super_frames;  // frames between two cross-wave combines (set by the launcher)
    S2rVoiceArrays v;
    float *block_partials;   // [n_blocks][frames_stride]
    float *direct_out;       // single-workgroup shard with the root add: the final mix, written by the render
                             // kernel itself ((+0.0) + the block's sum, what s2r_mix_kernel computes for one row)
    int32_t direct_stereo;   // interleaved L,R
    S2rDone done;            // with direct_out: told to the host when the output is written
    float *per_voice;        // [n_voices][frames] or nullptr (mix-disabled debug/parity path)
    const float *sin_table;  // 1024 floats (tables.rs)
    const float *noise_tab;  // 65536 floats: the x16 noise (hashnoise.rs:33-51) of hashed word x, seed and offset folded into x
                             // (s2r_noise_table_kernel); nullptr: computed per frame
    // coefficient tables: everything of a frame that depends on the mod envelope alone, as a
    // function of the envelope's own clock — shared by every voice that plays this patch
    S2rTabRef tab;
    // timed events of this fill (nullptr: none)
    const S2rTimedEvent *tev;
    int32_t *voice_ev_head;     // [padded voices] index of the voice's first timed event, -1 = none
    // diagnostic builds only (-DS2R_STAMPS, tools/stamps.py): [waves][16] s_memtime stamps of the render kernel's phases
    unsigned long long *stamps;
    // ... and (tools/gpu_timeline.py) [launches][2] s_memrealtime of this launch's first entry and last exit, slot `tl_slot`
    unsigned long long *timeline;
    uint32_t tl_slot;
    uint32_t uw_frames;   // the uniform window (uw_count below): frames of a wave's window, set by the launcher: S2R_UW_FRAMES,
                          // or 0 where there is none (here: the word fills a gap; the kernel arguments are at their 4 KiB)
    // patch bank (bank_size > 1: s2r_render_general_kernel<ANY, true>; the fields above then hold patch 0)
    const S2rBankEntry *bank;
    uint32_t bank_size;
    // Fills in flight on two streams (S2rOverlap below; the one-pole kernel): this launch waits for its chain heads, built
    // by a kernel on the other stream, and counts its workgroups in for the mix that waits there.  nullptr: not used.
    const uint32_t *ov_heads_counter;
    uint32_t ov_heads_target;
    uint32_t *ov_render_counter;
    uint32_t *ov_fail;
    // One launch per fill (S2rMixTail above): arrive != nullptr
    const S2rTimedEvent *tev_src;    // the fill's records, grouped by workgroup (mapped host memory, device view)
    S2rTimedEvent *tev_copy;         // ... and where the workgroups put them in HBM (== tev)
    const uint32_t *slices;          // workgroup b's records are [slices[b], slices[b + 1]); nullptr: S2rRenderArgs.ev holds the bounds
    uint32_t *arrive;                // rows counter of this fill's parity (device memory; only grows)
    uint32_t arrive_target;          // its value when every workgroup has written its row
    S2rMixTail mt;
    // The uniform window (the one-pole kernel's launch-per-fill form): a wave whose 64 voices started together
    // takes its chunks' coefficients, amplitudes and noise from a region of LDS it fills once per run.
    uint32_t *uw_count;              // the handle's count of chunks rendered that way; nullptr: the window is switched off
};
#define S2R_UW_FRAMES 1024u          /* a whole-fill super-chunk's worth: one fill of the window serves any run */
#define S2R_UW_PLANES 4u             /* x, 1 - x, amplitude, noise */
#define S2R_UW_MIN_RUN 3u            /* chunks a run must have for the window's fill to pay */

// Coalesced note events, one record per touched voice per fill (host folds the event
// stream of synth.rs:61-80 between two fills into the voice's final state).
struct S2rVoiceEvent {
    uint32_t voice;       // shard-local index
    uint32_t flags;       // bit0: restart (note_on), bit1: release (note_off after the last on),
                          // bits 16..: the program (patch bank index) a restart carries
    float pitch;          // valid when restart
    uint32_t seed;        // NoiseState.seed for the restarted voice (reference: 0)
};
#define S2R_EV_RESTART 1u
#define S2R_EV_RELEASE 2u
#define S2R_EV_PROGRAM_SHIFT 16

// A note event that takes effect INSIDE a fill, at a 16-frame boundary — what s2_bin does by
// calling sample() 16 frames at a time with MIDI applied in between (main.rs:138-143), here
// inside one launch.  Records live in mapped host memory; a voice's events of one fill form a
// chain (next), its first one is published through voice_ev_head[voice].
struct S2rTimedEvent {
    uint32_t voice;       // shard-local index
    uint32_t frame;       // frame offset inside the fill, multiple of 16
    uint32_t flags;       // S2R_EV_RESTART / S2R_EV_RELEASE, S2R_TEV_FIRST
    float pitch;          // valid when restart
    uint32_t seed;
    int32_t next;         // index of the voice's next event in this fill, -1 = none
    uint32_t program;     // patch bank index of a restart
    uint32_t _pad;
};
#define S2R_TEV_FIRST 0x100u

// The fill's folded note events ride in the render kernel's own arguments when there are few of them (no trip to
// host memory, no launch of their own): every wave picks the records that hit its 64 voices and applies them before it
// loads its state.
#define S2R_ARG_MAX_EVENTS 288u
struct S2rRenderArgs {
    S2rRenderParams p;
    uint32_t n_events;
    uint32_t _pad;
    uint32_t ev[3 * S2R_ARG_MAX_EVENTS];   // voice, S2rVoiceEvent.flags, pitch bits
};
static_assert(sizeof(S2rRenderArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// The resident render kernel (s2r_resident_kernel; s2r_set_low_latency): ONE workgroup that stays on the device between
// fills, polls a command in mapped host memory, renders the fill it describes (the one-pole kernel's fill, state in HBM
// between fills as ever) straight into mapped host memory and reports through the fill's completion word — a 16-frame
// fill then costs two trips over the host link and a few microseconds of kernel, not a launch.
//   command: 32 words in two 64-byte lines, read by one wave with one load per lane.  The host writes the payload, then
//   word 31, then word 0 (x86 stores become visible in program order): a reader that finds word 0 == word 31 == a new
//   sequence number has the whole command.
#define S2R_RES_CMD_WORDS 32u
#define S2R_RES_MAX_EVENTS 9u          // 4 header words + 9 * 3 + the closing sequence word
#define S2R_RES_FLAG_EXIT 1u
#define S2R_RES_GRANULE_FRAMES 64u     // fills up to this length come back as granules (FillCtl, s2r_kern_common.h)
struct S2rResident {
    const uint32_t *cmd;         // [32], device address of the mapped host command:
                                 //   [0] seq  [1] frames | flags << 16  [2] n_events  [3] the completion word's value
                                 //   [4 .. 30] events (voice, flags, pitch bits)  [31] seq
    uint32_t *exited;            // mapped host word: the kernel stores `launch_id` there as its last act
    uint32_t launch_id;
    uint32_t first_seq;          // the first command's sequence number (everything before it is stale)
    uint32_t idle_ticks;         // leaves after this many 100 MHz ticks without a command ...
    uint32_t max_polls;          // ... or this many polls, whichever comes first: the grid always drains
    uint32_t *done_flag, *done_counter;   // the fills' completion word (S2rDone; the command carries the value)
    unsigned long long *granules;         // [S2R_RES_GRANULE_FRAMES] mapped host memory: short fills' output (tag = the command's completion value)
};

// The POOL-RESIDENT render kernel (s2r_pool_kernel; s2r_set_resident): the whole grid of a shard — at most one workgroup
// per compute unit — stays on the device between fills.  The host posts a fill as a COMMAND (one 64-byte line in a ring of
// S2R_POOL_CMD_SLOTS, in fine-grained device memory behind the BAR or in mapped host memory), the fill's records grouped by
// workgroup and the groups' bounds; every workgroup renders the fill with the code a launch per fill runs (one launch per
// fill's form: S2rMixTail), then looks for the next command — a workgroup that is done early starts the next fill while
// the slowest ones still finish this one, so a fill lasts as long as the AVERAGE workgroup, not the slowest, once two are in
// flight.  No launch, no kernel boundary, no launch latency per fill.
//   command words: [0] seq  [1] frames | flags << 16  [2] records in this fill  [3] the completion word's value
//                  [4] output: 0, 1 the ring slots, 2 the synchronous buffer; | 256: stereo  [5] event slot (tev_src index)
//                  [6] parity  [7] arrive_target  [8] n_mixers  [9] rows_target  [10] rows slot  [11] heads target (two streams)
//                  [12] 1: the output as granules (tag = [3])  [15] seq
//   Whether command `s` runs is decided ONCE for the whole grid, by whoever gets there first: word `decided` in device
//   memory holds 2 * seq + bail of the last command decided; a workgroup that sees command s = last + 1 complete moves it
//   2 * last -> 2 * s (run) and one whose patience has run out moves it -> 2 * s + 1 (everybody leaves: the host finds
//   `exited` == launch_id, waits for the stream and starts the kernel again in front of the commands that were not run).
//   Every wait is bounded in ticks and in polls: the grid always drains.
#define S2R_POOL_CMD_SLOTS 4u
#define S2R_POOL_CMD_WORDS 16u
#define S2R_POOL_FLAG_EXIT 1u
#define S2R_POOL_FLAG_TWO_STREAMS 2u   // the fill's chain heads and mix are a launch on the other stream (S2rOverlapWords); [11] the heads' target
struct S2rPool {
    const uint32_t *cmd;              // [S2R_POOL_CMD_SLOTS][16]
    const uint32_t *slices;           // [S2R_POOL_CMD_SLOTS][n_blocks + 1], mapped host memory
    uint32_t slices_stride;
    const S2rTimedEvent *tev_src[4];  // the event slots' records (mapped host memory, device view)
    S2rTimedEvent *tev_copy[2];       // by parity
    int32_t *heads[2];
    float *partials[2];
    uint32_t *arrive;                 // [2] by parity
    const uint32_t *ov_heads;         // S2rOverlapWords.heads_done[2], .render_done[2] (two-stream fills)
    uint32_t *ov_render;
    float *out[3];                    // ring slot 0, ring slot 1, the synchronous buffer (mapped host memory) — or this shard's rows
    uint32_t *done_flag, *done_counter;   // [3] each, as `out`
    uint32_t *decided;                // device memory
    uint32_t *exited;                 // mapped host memory
    uint32_t *fail;
    uint32_t launch_id, first_seq, idle_ticks, max_polls;
    S2rMixTail mt;                    // what does not change from fill to fill (n_blocks, groups, exchange geometry)
    float *rows[2], *rows_mine[2];    // exchange: the root's rows by rows slot, and this shard's row among them; the ROOT's outputs:
    float *final_out[3];
    uint32_t *final_flag, *final_counter;
    unsigned long long *granules;     // [S2R_RES_GRANULE_FRAMES] mapped host memory: synchronous fills of up to that many frames
};

// what s2r_table_kernel needs: the patch resolved for a sample rate and where the planes go
struct S2rTabBuild {
    S2rEnv mod;
    float lpf_freq, amt_lpf, amt_osc, sr, rcp_sr;
    int32_t fast_div_sr;
    int32_t lpf_kind;
    float lpf_damping;
    float *base;
    uint32_t plane, n_ad, n_rel, n_entries;   // region lengths incl. padding; entries per plane
    uint32_t rc_t0;
    uint32_t fm_plane;
};

// Two fills in flight on TWO streams (s2r_fill_begin / s2r_fill_end).  Between the render kernels of
// consecutive fills the stream used to run the previous fill's mix and this fill's chain heads (3 us and two kernel
// boundaries per step).  Both now run on a second stream, beside the render kernels, and what orders them is in device
// memory: a counter of workgroups per buffer parity that have finished the chain heads (the render kernel of that fill
// waits for it before it looks at its voices' chains) and one of render workgroups that have written their partial row
// (the mix waits for it).  Counters only grow; the host hands every waiter the value to wait for.  Every wait is
// bounded (50 ms of the device clock): a waiter that gives up raises `fail` (mapped host memory) and goes on, and the
// host reports the fill as failed — nothing spins for ever.  Heads, event copies and partial rows are double-buffered by
// the fill's parity (at most two fills are in flight).
struct S2rOverlapWords { uint32_t render_done[2], heads_done[2]; };

struct S2rMixParams {
    const float *block_partials;  // [n_blocks][frames_stride]
    uint32_t n_blocks;
    uint32_t blocks_per_group;
    uint32_t n_groups;
    uint32_t frames;
    uint32_t frames_stride;
    int32_t root_add;             // 1: out = (+0.0) + total  (synth.rs:176), 0: partial only
    int32_t stereo;               // 1: write interleaved L,R (audio_player.rs:224-228)
    float *out;
    S2rDone done;                 // told to the host when `out` (mapped host memory) is complete
    const uint32_t *ov_render_counter;   // S2rOverlap: wait until *counter reaches ov_render_target before reading the rows
    uint32_t ov_render_target;
    uint32_t *ov_heads_counter;   // ... and (s2r_mix_and_heads_kernel) every chain-heads workgroup counts itself in here
    uint32_t *ov_fail;
    unsigned long long *timeline; // diagnostic builds only: as S2rRenderParams.timeline
    uint32_t tl_slot;
    unsigned long long *granules; // short fills of the pool-resident kernel: the output as tagged 8-byte words (FillCtl.granules)
    uint32_t granule_tag;
};

// The panned two-channel mixdown (s2r_fill_panned): the voices' rows of a MODE 1 render, each multiplied by
// its voice's two gains, through the mix tree of DESIGN.md 4.3 once per channel.
struct S2rPanMix {
    const float *rows;            // [n_voices][stride]: what the render kernel left in S2rRenderParams.per_voice
    const float *gain_l, *gain_r; // [n_blocks * block_voices] each, entries past n_voices hold 0
    uint32_t n_voices, block_voices, n_blocks;
    uint32_t frames, stride;      // stride >= frames
    float *partials;              // [n_blocks][2][pstride]: the workgroups' L and R partial rows
    uint32_t pstride;             // >= frames
    uint32_t blocks_per_group, n_groups;
    float *out;                   // interleaved L, R: 2 * frames floats
};

// The bus mixdown (s2r_fill_buses): the same rows, each voice on one of n_buses stereo buses, its two gains
// already scaled by the voice's gain; every bus and channel through the mix tree of DESIGN.md 4.3, all from one read of the rows.
// ONE argument block for every form of it; the optional pointers at its end say which form a fill is:
//   d_l != nullptr: program faders on their way (4.14) — the gain of voice v at frame i of the CALL is g_c[v][i] = G0_c[v] +
//   (float)i * d_c[v] (the product rounded, then the sum); gain_l / gain_r hold G0.
//   send != nullptr: aux sends (4.15) — voice v also feeds bus min(send_bus[v], n_buses - 1) with h_c = g_c * send[v] (under a
//   ramp: H0 = G0 * send, e = d * send), one rounded multiply each, in the kernel; on a bus that is both its main and its send
//   bus its gain is g + h.
struct S2rBusMix {
    const float *rows;            // [n_voices][stride]
    const float *gain_l, *gain_r; // [n_blocks * block_voices] each: pan gain times voice gain, entries past n_voices hold 0
    const uint8_t *bus;           // [n_blocks * block_voices]: the bus a voice is booked on (folded onto n_buses - 1 by the kernel)
    uint32_t n_voices, block_voices, n_blocks;
    uint32_t frames, stride;      // stride >= frames
    float *partials;              // [n_blocks][S2R_MAX_BUSES][2][pstride]: the workgroups' partial rows per bus and channel
    uint32_t pstride;             // >= frames
    uint32_t blocks_per_group, n_groups;
    float *out;                   // [n_buses][ostride]: bus-major, L, R interleaved inside a bus
    size_t ostride;               // floats from one bus to the next, >= 2 * frames
    uint32_t n_buses;             // 1 .. S2R_MAX_BUSES
    uint32_t lanes;               // threads along the frames of a tile (set by s2r_launch_bus_mix)
    const float *d_l, *d_r;       // [n_blocks * block_voices] each: the gain's step per frame, entries past n_voices hold 0; nullptr: a static fill
    uint32_t frame_base;          // the call-relative frame of rows' first frame (a segment's or a slice's start)
    const float *send;            // [n_blocks * block_voices]: the voice's send in [0, 1], entries past n_voices hold 0; nullptr: no sends
    const uint8_t *send_bus;      // [n_blocks * block_voices]: the bus it feeds (folded onto n_buses - 1 by the kernel)
};

hipError_t s2r_launch_tables(const S2rTabBuild &b, hipStream_t stream);
hipError_t s2r_launch_noise_table(float *table_65536, hipStream_t stream);
// one-pole single-patch handles of one workgroup only (a.p.direct_out set, a.p.frames = the longest fill): false otherwise
hipError_t s2r_launch_resident(const S2rRenderArgs &a, const S2rResident &rs, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_render(const S2rRenderArgs &a, uint32_t block_voices, hipStream_t stream);
// the pool-resident kernel of a one-pole single-patch shard (a.p.frames = the longest fill)
hipError_t s2r_launch_pool(const S2rRenderArgs &a, const S2rPool &pl, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_mix(const S2rMixParams &p, hipStream_t stream);
hipError_t s2r_launch_events(const S2rVoiceArrays &v, const S2rVoiceEvent *dev_events, uint32_t n, hipStream_t stream);
hipError_t s2r_launch_mix_and_heads(const S2rMixParams &m, int32_t *heads, const S2rTimedEvent *tev, S2rTimedEvent *tev_copy, uint32_t n,
                                    hipStream_t stream);
hipError_t s2r_launch_tev_heads(int32_t *heads, const S2rTimedEvent *tev, S2rTimedEvent *tev_copy, uint32_t n, hipStream_t stream,
                                uint32_t *ov_heads_counter = nullptr);
// build-defined 4x decimator: x = 62 samples of history + 4 * n_out new ones, h = 63 taps (device), and the
// last 62 inputs copied to the front of x afterwards (second launch) for the next call
hipError_t s2r_launch_decimate4(float *x_with_history, const float *taps, uint32_t n_out, float *out, hipStream_t stream);
// out[i] = ((+0.0 + rows[0][i]) + rows[1][i]) + ...; rows are `stride` floats apart; stereo: interleaved L, R with L == R
hipError_t s2r_launch_sum_rows(const float *rows, uint32_t n_rows, uint32_t frames, uint32_t stride, int stereo, float *out, hipStream_t stream,
                               const S2rDone *done);
// s2r_pan_mix_kernel (a workgroup's voices, both channels from one load of every row element) and the kernel that adds the
// workgroups' partial rows in the documented order, rooted at +0.0
hipError_t s2r_launch_pan_mix(const S2rPanMix &m, hipStream_t stream);
// s2r_bus_mix_kernel (the instantiation for the call's bus count, the rows' alignment, RAMP = d_l != nullptr and SEND = send !=
// nullptr) and s2r_bus_combine_kernel; d_l without d_r or send without send_bus: hipErrorInvalidValue
hipError_t s2r_launch_bus_mix(const S2rBusMix &m, hipStream_t stream);

// The per-bus convolution reverb of s2r_fill_buses.  A bus's line holds, per channel, its K - 1 frames of history
// and behind them the call's dry frames; `next` receives the history the next call starts from (the host swaps the two).
struct S2rFxBus {
    const float *taps;            // [2][tstride] planar: ir_L, then ir_R, each padded with +0.0 up to whole segments
    float *line, *next;           // [2][lstride] planar each
    float *partials;              // [2][n_seg][S2rFx.pstride]: P_s of every segment
    uint32_t n_taps, n_seg;       // K (0: no reverb on this bus) and ceil(K / S2R_IR_SEGMENT)
    uint32_t tstride, lstride;    // tstride >= n_seg * S2R_IR_SEGMENT; lstride >= K - 1 + frames
    float dry, wet;
};
struct S2rFx {
    S2rFxBus bus[S2R_MAX_BUSES];
    const float *stage;           // [n_buses][2 * frames]: what the bus combine wrote, bus-major, L, R interleaved inside a bus
    float *out;                   // the same layout: the caller-visible output
    uint32_t n_buses, frames;
    uint32_t pstride;             // >= frames, a multiple of 8
};
// stage -> lines (or, for a bus without a reverb, -> out unchanged), the segments' partial sums, and the kernel that adds them, mixes
// dry and wet into `out` and advances the history
hipError_t s2r_launch_bus_fx(const S2rFx &fx, hipStream_t stream);

// The per-bus feedback delay in front of the reverbs.  A bus's line holds its D frames of history of the line signal
// W, oldest first, L, R interleaved; `next` receives the history the next call starts from (the host swaps the two).
struct S2rDelayBus {
    const float *line;            // [D][2]
    float *next;                  // [D][2], not `line`
    uint32_t delay;               // D (0: no delay on this bus: it is copied from `in` to `out`)
    float feedback, cross, dry, wet;
};
struct S2rDelay {
    S2rDelayBus bus[S2R_MAX_BUSES];
    const float *in;              // [n_buses][2 * frames]: what the bus combine wrote, bus-major, L, R interleaved inside a bus
    float *out;                   // the same layout, not `in`: what the next stage, or the caller, reads
    uint32_t n_buses, frames;
};
// one kernel: the delays' outputs and next histories, the other buses unchanged; hipErrorInvalidValue for a null pointer, in == out,
// a D past S2R_MAX_DELAY_FRAMES, line == next, n_buses past S2R_MAX_BUSES or no delay at all among the call's buses
hipError_t s2r_launch_bus_delay(const S2rDelay &a, hipStream_t stream);

// The per-bus chorus in front of the delays.  A bus's line holds its H frames of history of the INPUT, oldest first,
// L, R interleaved; `next` receives the history the next call starts from (the host swaps the two and moves the phase on).
struct S2rChorusBus {
    const float *line;            // [H][2]
    float *next;                  // [H][2], not `line`
    uint32_t voices;              // V (0: no chorus on this bus: it is copied from `in` to `out`)
    uint32_t history;             // H = floor(fl(base + depth)) + 1, 2 .. S2R_CHORUS_MAX_DELAY + 1
    uint32_t phase, phase_inc, spread;
    float base, depth, dry, wet;
    uint32_t off[S2R_CHORUS_MAX_VOICES];     // floor(v * 2^32 / V): the left channel's offset of voice v
};
struct S2rChorus {
    S2rChorusBus bus[S2R_MAX_BUSES];
    const float *in;              // [n_buses][2 * frames]: what the bus combine wrote, bus-major, L, R interleaved inside a bus
    float *out;                   // the same layout, not `in`: what the next stage, or the caller, reads
    uint32_t n_buses, frames;
};
// one kernel: the choruses' outputs and next histories, the other buses unchanged; hipErrorInvalidValue for a null pointer, in == out,
// line == next, a V past S2R_CHORUS_MAX_VOICES, an H below 2 or past S2R_CHORUS_MAX_DELAY + 1, n_buses past S2R_MAX_BUSES or no chorus at
// all among the call's buses
hipError_t s2r_launch_bus_chorus(const S2rChorus &a, hipStream_t stream);

// The per-bus parametric EQ at the head of the chain: a cascade of up to S2R_EQ_MAX_BANDS biquads in transposed
// direct form II.  A bus's line holds its state, [band][s1_L, s1_R, s2_L, s2_R]; `next` receives the state the next call starts
// from (the host swaps the two).
#define S2R_EQ_TILE 64u           // frames the kernel stages at a time: its loads run one tile ahead, its stores one tile behind
struct S2rEqBus {
    const float *line;            // [n_bands][4]
    float *next;                  // [n_bands][4], not `line`
    uint32_t n_bands;             // 0: no EQ on this bus: it is copied from `in` to `out`
    float c[S2R_EQ_MAX_BANDS][5]; // (b0, b1, b2, a1, a2) per band
};
struct S2rEq {
    S2rEqBus bus[S2R_MAX_BUSES];
    const float *in;              // [n_buses][2 * frames]: what the bus combine wrote, bus-major, L, R interleaved inside a bus
    float *out;                   // the same layout, not `in`: what the next stage, or the caller, reads
    uint32_t n_buses, frames;
};
// one kernel: the EQs' outputs and next states, the other buses unchanged; hipErrorInvalidValue for a null pointer, in == out,
// line == next, more than S2R_EQ_MAX_BANDS bands, n_buses past S2R_MAX_BUSES or no EQ at all among the call's buses
hipError_t s2r_launch_bus_eq(const S2rEq &a, hipStream_t stream);

// The per-bus dynamics behind the EQ: a sidechain compressor.  A bus's line holds its one gain y; `next` receives
// the gain the next call starts from (the host swaps the two).
#define S2R_DYN_TILE 256u         // frames of one stage of the kernel's pipeline: targets a tile ahead of the walk, outputs a tile behind
struct S2rDynBus {
    const float *line;            // [1]: y
    float *next;                  // [1], not `line`
    const float *curve;           // [S2R_DYN_CURVE_POINTS] in device memory; null: no dynamics on this bus, or idle: it is copied from `in` to `out`
    uint32_t key;                 // the key bus, among the call's buses
    float a_att, a_rel;
};
struct S2rDyn {
    S2rDynBus bus[S2R_MAX_BUSES];
    const float *in;              // [n_buses][2 * frames]: what the EQ, or else the bus combine, wrote; bus-major, L, R interleaved inside a bus
    float *out;                   // the same layout, not `in`: what the next stage, or the caller, reads
    float *meter;                 // [S2R_MAX_BUSES], pinned and device-mapped: the call's minimum of y per bus that ran
    uint32_t n_buses, frames;
};
// one kernel: the outputs, next gains and meters of the buses with dynamics, the other buses unchanged; hipErrorInvalidValue for a null
// pointer, in == out, line == next, a key or n_buses past its range or no dynamics at all among the call's buses
hipError_t s2r_launch_bus_dyn(const S2rDyn &a, hipStream_t stream);

// The per-bus room behind the convolution reverb: eight damped combs and four allpasses per channel.  A bus's line
// holds its state in the checkpoint's layout (s2r.h); `next` receives the state the next call starts from (the host swaps the two).
// Line l of the 24: comb i of channel c is l = c * 8 + i, allpass j is l = 16 + c * 4 + j; len[l] frames at off[l] of the state, a
// comb's f behind its line.  The frames a line gains inside the call go to row l of `work`, [24][wstride], and are read from there.
#define S2R_ROOM_TILE 32u         // frames of one pass of the kernel: half the least delay, so that a tile's reads are a tile old when they are issued
#define S2R_ROOM_LINES 24u
struct S2rRoomBus {
    const float *line;            // the state; null: no room on this bus: it is copied from `in` to `out`
    float *next;                  // the same size, not `line`
    float *work;                  // [S2R_ROOM_LINES][wstride]
    uint32_t len[S2R_ROOM_LINES], off[S2R_ROOM_LINES];
    uint32_t floats;              // of the state
    float feedback, damp, d1, g, gain, dry, wet, cross;
};
struct S2rRoom {
    S2rRoomBus bus[S2R_MAX_BUSES];
    const float *in;              // [n_buses][2 * frames]: what the stage in front wrote; bus-major, L, R interleaved inside a bus
    float *out;                   // the same layout, not `in`
    uint32_t n_buses, frames, wstride;
};
// one kernel: the outputs and next states of the buses with a room, the other buses unchanged; hipErrorInvalidValue for a null
// pointer, in == out, line == next, a line outside its range or its state, frames > wstride, n_buses past
// S2R_MAX_BUSES or no room at all among the call's buses
hipError_t s2r_launch_bus_room(const S2rRoom &a, hipStream_t stream);

// The per-bus drive behind the dynamics: 4x up through g, a table, back down through h.  A bus's line holds its last
// S2R_DRIVE_HISTORY input frames, [32][2]; `next` receives the state the next call starts from (the host swaps the two).  Feed-forward:
// a tile of S2R_DRIVE_TILE output frames needs the 32 input frames in front of it and nothing another tile wrote.
#define S2R_DRIVE_HALF_TAPS 33u   // (S2R_DRIVE_TAPS + 1) / 2
#define S2R_DRIVE_TILE 240u       // output frames of one workgroup: with the S2R_DRIVE_LATENCY frames in front of them, a frame per lane
struct S2rDriveBus {
    const float *curve;           // [S2R_DRIVE_CURVE_POINTS] in device memory; null: no drive on this bus: it is copied from `in` to `out`
    const float *line;            // [S2R_DRIVE_HISTORY][2]
    float *next;                  // the same size, not `line`
    float pre, dry, wet;
};
struct S2rDrive {
    S2rDriveBus bus[S2R_MAX_BUSES];
    float h[S2R_DRIVE_HALF_TAPS], g[S2R_DRIVE_HALF_TAPS];    // taps 0 .. 32 of each filter, which is symmetric on bits; in the kernel's arguments: wave-uniform, read with scalar loads
    const float *in;              // [n_buses][2 * frames]: what the stage in front wrote; bus-major, L, R interleaved inside a bus
    float *out;                   // the same layout, not `in`
    uint32_t n_buses, frames;
};
// one kernel, (tiles, n_buses) workgroups: the outputs and next states of the buses with a drive, the other buses unchanged;
// hipErrorInvalidValue for a null pointer, in == out, line == next, n_buses past S2R_MAX_BUSES or no drive at all among the call's buses
hipError_t s2r_launch_bus_drive(const S2rDrive &a, hipStream_t stream);

// The per-bus flanger behind the drive: one tap at a modulated fractional delay of at least S2R_FLANGER_MIN_DELAY = 32
// frames into the stage's own line signal w, fed back.  A bus's line holds the last `history` frames of w, [H][2], oldest first; `next`
// receives the line the next call starts from (the host swaps the two).  No frame reads a frame of w younger than 32 frames: the frames
// of a tile of S2R_FLANGER_TILE are independent of one another.
#define S2R_FLANGER_TILE 32u
struct S2rFlangerBus {
    const float *line;            // [history][2]; null: no flanger on this bus: it is copied from `in` to `out`
    float *next;                  // the same size, not `line`
    uint32_t history;             // H: 33 .. 4096
    uint32_t phase, phase_inc, spread;
    float base, depth, feedback, cross, dry, wet;
};
struct S2rFlanger {
    S2rFlangerBus bus[S2R_MAX_BUSES];
    float *in;                    // [n_buses][2 * frames]: what the stage in front wrote; bus-major, L, R interleaved inside a bus (the
                                  // product's kernel only reads it; the serial form keeps the call's w in it)
    float *out;                   // the same layout, not `in`
    uint32_t n_buses, frames;
};
// one kernel, one wavefront per bus with a flanger and further workgroups that copy the buses without: the outputs and next lines of the
// buses with a flanger, the other buses unchanged; hipErrorInvalidValue for a null pointer, in == out, line == next, a history outside
// [33, 4096], n_buses past S2R_MAX_BUSES or no flanger at all among the call's buses
hipError_t s2r_launch_bus_flanger(const S2rFlanger &a, hipStream_t stream);

// The master section of s2r_fill_master: the stems of a call, post-effect, each times its return's ramp, added in
// bus order from +0.0, times the master fader's ramp; and the call's meters.  gain at frame i of the CALL: r0 + (float)i * dr (the
// product rounded, then the sum); a pair that did not move has dr = +0.0.
#define S2R_MASTER_CH ((S2R_MAX_BUSES + 1u) * 2u)   // meter channels of a row at most: bus-major, L then R, the master behind the call's buses
#define S2R_MASTER_ROW (2u * S2R_MASTER_CH)         // a row of block partials: the peaks, then the energies
struct S2rMaster {
    const float *stage;           // [n_buses][2 * frames] in device memory: what the last stem writer of the call left, L, R interleaved
    float *out;                   // interleaved L, R: 2 * frames floats (mapped host memory)
    float *stems;                 // nullptr, or where the caller-visible stems go (mapped host memory), the layout of `stage`
    float *partials;              // [ceil(frames / S2R_METER_BLOCK)][S2R_MASTER_ROW] (mapped host memory): one row per meter block
    uint32_t n_buses, frames;     // 1 .. S2R_MAX_BUSES
    float r0[S2R_MAX_BUSES], dr[S2R_MAX_BUSES];     // the returns' applied positions and their steps per frame
    float m0, dm;                 // the master fader's
};
// s2r_master_kernel<NB> for the call's bus count (1, 2, 4 or 8 compiled in; a count between them runs the next form with guarded buses)
hipError_t s2r_launch_master(const S2rMaster &m, hipStream_t stream);

// The master limiter of s2r_fill_master: one launch behind the master kernel.  It reads the master from device memory
// and the current copy of the state, writes the limited master to the pinned output, the call's meter partials and the OTHER copy
// of the state; the host flips the copies after a synchronise that succeeded.
#define S2R_LIMITER_BLOCK 256u                      // frames of one workgroup, one per thread
struct S2rLimiter {
    const float *x;               // [frames][2] in device memory: what the master kernel of the call wrote
    float *out;                   // interleaved L, R: 2 * frames floats (mapped host memory)
    const float *xh, *gh;         // the state the call starts from: [lookahead][2] and [2 * lookahead + hold]
    float *xh_next, *gh_next;     // ... and the state it leaves (never the buffers above)
    float *partials;              // [ceil(frames / S2R_LIMITER_BLOCK)][2] (mapped host memory): min s', max |y| of each workgroup
    uint32_t frames, lookahead, hold;
    float ceiling;
};
hipError_t s2r_launch_limiter(const S2rLimiter &a, hipStream_t stream);

// ... with the true-peak detector: a kernel and a block of its own, so that the sample-peak kernel and its arguments
// stay what they were.  One launch, in the same place; `l.xh`, `l.xh_next` are [lookahead + S2R_LIMITER_TP_HISTORY][2] here.
struct S2rLimiterTp {
    S2rLimiter l;
    float g[33];                  // taps 0 .. 32 of the interpolator g = 4 h, which is symmetric on bits (as S2rLoudness::g)
};
hipError_t s2r_launch_limiter_tp(const S2rLimiterTp &a, hipStream_t stream);

// The master's multiband compressor: one launch behind the master kernel and in front of the limiter, in a master fill
// that finds the stage set.  The master kernel writes the stage's own device buffer in such a call; this kernel reads it and writes
// where the master kernel would have written.  The sections come as the rule's graph (multiband_graph, s2r_rules.h) with their
// coefficients beside them; the state is the checkpoint's (s2r.h), `next` receives what the next call starts from.
#define S2R_MULTIBAND_TILE 128u   // frames of one stage of the kernel's pipeline
struct S2rMultiband {
    const float *in;              // [frames][2] in device memory: what the master kernel wrote
    float *out;                   // [frames][2], not `in`: the limiter's input, the meters' input or the pinned output
    const float *state;           // [S2R_MULTIBAND_STATE(n_bands)]
    float *next;                  // the same size, not `state`
    const float *curves;          // [n_bands][S2R_DYN_CURVE_POINTS] in device memory
    float *meter;                 // [S2R_MULTIBAND_MAX_BANDS], pinned and device-mapped: the call's minimum of y per band
    float c[15][5];               // (b0, b1, b2, a1, a2) of every section, in the state's order
    int32_t src[15];              // the section in front of it; -1: the stage's input
    uint32_t depth[15];           // the sections in front of it
    int32_t leaf[S2R_MULTIBAND_MAX_BANDS];       // the section that leaves band j; -1: the stage's input (one band)
    float a_att[S2R_MULTIBAND_MAX_BANDS], a_rel[S2R_MULTIBAND_MAX_BANDS];
    uint32_t n_bands, n_sections, frames;
};
// hipErrorInvalidValue for a null pointer, in == out, state == next, a band count outside 1 .. 4 or a graph that is not the rule's
hipError_t s2r_launch_multiband(const S2rMultiband &a, hipStream_t stream);

// The loudness and true-peak meters of s2r_fill_master: one launch behind the limiter (or the master kernel), the last
// of a master fill that finds the meter set.  It reads the stems from the master's device stage and the master from device memory —
// whoever writes the master last writes it there in such a call, never into the pinned output —, copies the master to the pinned
// output itself, and writes the call's hop rows, its true-peak partials and the OTHER copy of the state; the host flips the copies
// after a synchronise that succeeded.  `pos` is the host's: the frames of the hop under way when the call starts.
#define S2R_LOUDNESS_TILE 256u                      // frames the walk's workgroup stages at a time, one tile ahead of the walk
#define S2R_LOUDNESS_BLOCK 256u                     // frames of one true-peak workgroup, one per thread
#define S2R_LOUDNESS_HALF_TAPS 33u                  // (S2R_DRIVE_TAPS + 1) / 2
struct S2rLoudness {
    const float *stems;           // [n_buses][2 * frames] in device memory: the master kernel's input
    const float *master;          // [frames][2] in device memory: what the limiter, or without one the master kernel, wrote
    float *out;                   // interleaved L, R: 2 * frames floats (mapped host memory)
    const float *state;           // [S2R_LOUDNESS_STATE]: the state the call starts from
    float *next;                  // ... and the state it leaves (never the buffer above)
    float *rows;                  // [(pos + frames) / hop][S2R_LOUDNESS_CHANNELS] (mapped host memory): the hops the call completes
    float *peaks;                 // [ceil(frames / S2R_LOUDNESS_BLOCK)][2] (mapped host memory): each workgroup's true peak, L and R
    float c[10];                  // the two biquads, (b0, b1, b2, a1, a2) each
    float g[S2R_LOUDNESS_HALF_TAPS];                 // taps 0 .. 32 of the interpolator g = 4 h, which is symmetric on bits
    uint32_t n_buses, frames, hop, pos;
};
hipError_t s2r_launch_loudness(const S2rLoudness &a, hipStream_t stream);

// The spectrum meters of s2r_fill_master: one launch behind the loudness kernel (or, without that meter, behind whoever
// wrote the master last), the last of a master fill that finds the meter set.  It reads the stems from the master's device stage and
// the master from device memory, writes the call's power rows and the OTHER copy of the state, and — only when no loudness kernel did
// it — copies the master to the pinned output (`out` null: somebody else has).  The host flips the copies after a synchronise that
// succeeded.  `pos` is the host's: the frames of the hop under way when the call starts.
#define S2R_SPECTRUM_COPY_BLOCKS 16u                // workgroups that write the next state and the copy, behind the transforms'
struct S2rSpectrum {
    const float *stems;           // [n_buses][2 * frames] in device memory: the master kernel's input
    const float *master;          // [frames][2] in device memory
    float *out;                   // interleaved L, R: 2 * frames floats (mapped host memory), or null
    const float *state;           // [9][n_fft][2]: the state the call starts from
    float *next;                  // ... and the state it leaves (never the buffer above)
    const float *window;          // [n_fft] in device memory
    const float *twiddles;        // [n_fft / 2][2] in device memory
    float *rows;                  // [(pos + frames) / hop][9][n_fft / 2 + 1] (mapped host memory): the rows the call completes
    uint32_t n_buses, frames, n_fft, hop, pos;
};
hipError_t s2r_launch_spectrum(const S2rSpectrum &a, hipStream_t stream);

// The PCM stage of s2r_fill_master: one launch behind the spectrum kernel (or, without the meters, behind whoever wrote
// the master last), the last of a master fill that finds the stage set.  It reads the stems from the master's device stage and the
// master from device memory, writes the call's samples of all nine programmes, the channels' clip counts and the OTHER copy of the
// state, and — only when no meter kernel did it — copies the master to the pinned output (`out` null: somebody else has).  The host
// flips the copies after a synchronise that succeeded.  `t` is the host's: the frames converted when the call starts.
#define S2R_PCM_TILE 128u                           // frames the walk's workgroup stages at a time, one tile ahead of the walk
#define S2R_PCM_COPY_BLOCK 1024u                    // frames of one copying workgroup
struct S2rPcm {
    const float *stems;           // [n_buses][2 * frames] in device memory: the master kernel's input
    const float *master;          // [frames][2] in device memory
    float *out;                   // interleaved L, R: 2 * frames floats (mapped host memory), or null
    const float *state;           // [S2R_PCM_STATE]: the state the call starts from
    float *next;                  // ... and the state it leaves (never the buffer above)
    int32_t *pcm;                 // [9][pstride][2] (mapped host memory): the call's samples, programme-major
    uint32_t *clips;              // [S2R_PCM_CHANNELS] (mapped host memory): the call's clips per channel
    float h[S2R_PCM_MAX_TAPS];    // the taps, +0.0 past n_taps
    uint32_t n_buses, frames, pstride, bits, dither, n_taps, seed, t;
};
hipError_t s2r_launch_pcm(const S2rPcm &a, hipStream_t stream);

// The sample-rate converter of s2r_fill_master: one launch behind the spectrum kernel (or, without the meters, behind
// whoever wrote the master last) and in front of the PCM kernel.  It reads the stems from the master's device stage and the master from
// device memory, writes the call's `count` output frames of all nine programmes to the pinned outputs — and, when the PCM stage runs
// behind it, to device memory in the layout that kernel's launch reads — and the OTHER copy of the state, and — only when no meter kernel
// did it — copies the master to the pinned output (`out` null: somebody else has).  The host flips the copies after a synchronise that
// succeeded.  `ph` and `count` are the host's.
#define S2R_RESAMPLER_TILE 64u                      // output frames of one workgroup, a lane each
#define S2R_RESAMPLER_COPY_BLOCK 1024u              // frames of one copying workgroup
struct S2rResampler {
    const float *stems;           // [n_buses][2 * frames] in device memory: the master kernel's input
    const float *master;          // [frames][2] in device memory
    float *out;                   // interleaved L, R: 2 * frames floats (mapped host memory), or null
    const float *state;           // [S2R_RESAMPLER_STATE(T)]: the state the call starts from
    float *next;                  // ... and the state it leaves (never the buffer above)
    const float *table;           // [L][T] in device memory
    float *res;                   // [9][out_cap][2] (mapped host memory): the call's outputs, programme-major
    float *res_dev;               // [9][count][2] in device memory: the same for the PCM kernel, or null
    uint32_t n_buses, frames, L, M, T, ph, count, out_cap;
};
hipError_t s2r_launch_resampler(const S2rResampler &a, hipStream_t stream);
