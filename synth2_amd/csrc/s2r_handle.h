// s2r_handle.h — the handle behind the C ABI of libs2r (include/s2r.h), as the host translation units share it: s2r_host.cpp (the
// handle's life, events, every launch form), s2r_host_mix.cpp (the panned, bus and master fills and the voice mixer's entries) and
// s2r_host_post.cpp (the entries in front of the post-mix chain).  Compiled with hipcc.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "s2r.h"
#include "s2r_device.h"
#include "s2r_mixer.h"
#include "s2r_patch.h"
#include "s2r_post.h"
#include "s2r_voices.h"

// What the three host files share beside the handle.  Hidden: a call from one of them to another stays a direct call inside the
// library, as it was while they were one file, and the library exports nothing new.
namespace s2r_host __attribute__((visibility("hidden"))) {

constexpr int kEventSlots = 4;

struct EventSlot {
    S2rVoiceEvent *host = nullptr;   // pinned
    S2rVoiceEvent *dev = nullptr;
    S2rTimedEvent *thost = nullptr;  // pinned, mapped: timed events of one fill
    S2rTimedEvent *tdev = nullptr;
    // Who still reads the slot's pinned records: nobody (0); the kernels in front of `done`, a HIP event recorded behind
    // them (1); or a fill whose completion word — index `idx`, value `seq` — the host can look at (2).  An event record
    // between two kernels of a stream costs the GPU ~3 us of idle time at that boundary (measured, tools/gpu_timeline.py:
    // boundaries of 4.5-5.0 us with the records, 1.7-2.4 without), so the fills that are tracked by a completion word
    // record none.
    hipEvent_t done = nullptr;
    int state = 0;
    volatile uint32_t *word = nullptr;   // state 2: the completion word (host view) ...
    uint32_t seq = 0;                    // ... and the value it shows once the fill is done
};

}  // namespace s2r_host

struct s2r_synth {
    s2r_config cfg{};
    int device = 0;
    uint32_t shard_begin = 0, shard_voices = 0, padded_voices = 0, block_voices = 256, n_blocks = 0, mix_groups = 1;
    uint32_t interleave = 0, shard_index = 0, shard_count = 1;   // round-robin sharding (s2r_config.shard_interleave)
    FastDiv div_interleave, div_count, div_per_kid;              // ... and its divisions (interleave, shard count, voices per contiguous shard)
    std::vector<s2r_patch> bank;                 // bank[0] is "the" patch of the reference's Synth
    uint32_t program = 0;                        // current program: the patch the next note_on gives its voice
    S2rBankEntry *bank_dev = nullptr;            // S2R_MAX_BANK entries, resolved for bank_rate
    bool bank_dirty = true; uint32_t bank_rate = 0;
    std::shared_ptr<S2rVoicePool> pool;          // one per Synth: the shards of a device-list handle share their parent's
    // Device list (s2r_config.n_devices > 1): this handle is the PARENT — it owns the pool, runs the allocation policy
    // once per event and routes the event to the shard (`kids[k]`, an ordinary single-device handle on devices[k])
    // that holds the voice; per fill every shard writes its partial mix into row k of `rows_dev` on the parent's
    // device (peer-to-peer where the devices differ) and the parent adds the rows in shard order rooted at +0.0.
    s2r_synth *parent = nullptr;
    std::vector<s2r_synth *> kids;
    float *rows_dev[2] = {nullptr, nullptr};     // [n kids][max_frames], one per fill in flight
    std::vector<float *> kid_stage;              // per kid: a row on ITS device when it cannot write the parent's rows directly
    std::vector<hipEvent_t> kid_done[2];         // per slot, per kid: its partial row is in rows_dev[slot]
    uint32_t rows_slot = 0;
    std::vector<uint32_t> seed_override;         // per pool voice; 0 = reference behaviour
    // event folding (one record per touched shard voice between two fills)
    std::vector<S2rVoiceEvent> pending;
    std::vector<int32_t> pending_slot;           // shard-local voice -> index in pending, -1
    s2r_host::EventSlot slots[s2r_host::kEventSlots];
    int next_slot = 0;
    // timed events (take effect inside the next fill at a 16-frame boundary)
    std::vector<S2rTimedEvent> tpending;
    std::vector<int32_t> tlast;                  // shard-local voice -> its last timed event this fill, -1
    std::vector<int32_t> tfirst;                 // scratch of flush_events: shard-local voice -> its first timed event, -1
    uint32_t fill_time = 0;                      // frames of the next fill the pool clock has already moved
    uint32_t tev_capacity = 0;
    int32_t *voice_ev_head = nullptr;
    S2rTimedEvent *tev_copy = nullptr;           // the fill's timed events in HBM (copied from the mapped slot by the heads kernel)
    // device
    hipStream_t stream = nullptr;
    S2rVoiceArrays v{};
    void *voice_mem = nullptr;
    float *block_partials = nullptr;
    float *out_dev = nullptr;
    float *out_host = nullptr;                   // pinned and device-mapped, 2*max_frames
    float *out_host_dev = nullptr;               // the device's view of out_host
    // Completion words (S2rDone): mapped host memory the last kernel of a fill writes its sequence number to — [0], [1]
    // the two ring slots of s2r_fill_begin / s2r_fill_end, [2] the synchronous fills — and the arrival counter in HBM
    uint32_t *done_host = nullptr, *done_dev = nullptr, *done_counter = nullptr;
    uint32_t done_seq = 0;                       // last value handed out
    uint32_t ring_seq[2] = {0, 0};               // what done_host[slot] must show before s2r_fill_end copies slot's buffer (0: wait on the event)
    // s2r_fill_begin / s2r_fill_end: two more mapped output buffers, the fills in flight (oldest first)
    float *ring_host[2] = {nullptr, nullptr}, *ring_dev[2] = {nullptr, nullptr};
    hipEvent_t ring_done[2] = {nullptr, nullptr};
    size_t ring_frames[2] = {0, 0};
    uint32_t ring_head = 0, ring_count = 0;
    // s2r_fill_begin leaves its fill's mix to the NEXT s2r_fill_begin, which launches it together with its own chain
    // heads (s2r_mix_and_heads_kernel: one launch boundary less per buffer), or to s2r_fill_end, whichever comes first
    struct DeferredMix { bool active = false; bool overlap = false; S2rMixParams m{}; int ring_slot = -1; } dmix;
    // Two streams for the fills of s2r_fill_begin (S2rOverlapWords, s2r_device.h): the mixes and the chain heads run on
    // stream_b beside the render kernels on `stream`; [1] of each pair is the second buffer (by the fill's parity)
    hipStream_t stream_b = nullptr;
    bool ov_enabled = false;                     // stream_b and the second buffers exist (S2R_OVERLAP=0 leaves them out)
    bool ov_registered = false;                  // ... and this handle holds its device's two-stream slot (g_two_stream_handles)
    bool ov_busy = false;                        // kernels of an overlapped fill may still be running on stream_b
    float *partials2[2] = {nullptr, nullptr};
    int32_t *heads2[2] = {nullptr, nullptr};
    S2rTimedEvent *tevcopy2[2] = {nullptr, nullptr};
    S2rOverlapWords *ov_words = nullptr;         // device memory
    uint32_t ov_render_target[2] = {0, 0}, ov_heads_target[2] = {0, 0};
    uint32_t ov_fill = 0;                        // overlapped fills begun so far: the next one's parity is its low bit
    // One launch per fill (S2rMixTail, s2r_device.h): the render kernel builds its own chain heads from the fill's records grouped
    // by workgroup and the last workgroups to finish add the rows up.  S2R_FUSED=0: the three-launch form (heads, render, mix)
    int fused_mode = 1;                          // 0 never; 1 everything but the two-stream fills of s2r_fill_begin; 2 those too
    uint32_t *fz_arrive = nullptr;               // device memory [2]: rows written, by parity (launches per fill use [0])
    uint32_t fz_target[2] = {0, 0};
    FastDiv div_block;                           // local voice -> workgroup
    std::vector<S2rTimedEvent> tsorted;          // the fill's records grouped by workgroup ...
    std::vector<uint32_t> tperm, tbounds;        // ... arrival index -> grouped index; workgroup b's records are [tbounds[b], tbounds[b + 1])
    // exchange of partial rows between the shards of a device list: a counter per rows slot in the parent's device memory
    uint32_t *rows_done = nullptr;
    uint32_t rows_target[2] = {0, 0};
    // exchange between PROCESSES (one process per GPU; s2r_exchange_create / _attach): the ranks' rows and the counters live in
    // one block of the root's device memory that the other ranks map through an IPC handle
    bool xg_on = false;
    uint32_t xg_rank = 0, xg_n = 0, xg_target[2] = {0, 0};
    float *xg_rows = nullptr;                    // [2][xg_n][max_frames]
    uint32_t *xg_done = nullptr;                 // [2] counters behind the rows, then [2] words `consumed` (the root's: fused_tail)
    void *xg_block = nullptr; bool xg_owner = false;
    bool force_stage = false, force_peer = false;   // S2R_FORCE_STAGE / S2R_FORCE_PEER: the multi-device branches on one device (tests)
    // The pool-resident render kernel (S2rPool, s2r_device.h; s2r_set_resident): running on `stream` between fills while
    // pool_running; stopped by every entry point that touches the device or what the kernel's arguments were built from
    bool resident = false, pool_running = false;
    uint32_t pool_seq = 0, pool_launch_id = 0, pool_rate = 0, pool_fills = 0;
    uint32_t *pool_cmd = nullptr, *pool_cmd_dev = nullptr; bool pool_cmd_vram = false;
    uint32_t *pool_slices = nullptr, *pool_slices_dev = nullptr;   // mapped host memory [S2R_POOL_CMD_SLOTS][n_blocks + 1]
    uint32_t *pool_host = nullptr, *pool_host_dev = nullptr;       // mapped host memory: [0] the kernel's "exited" word
    uint32_t *pool_decided = nullptr;                              // device memory
    bool pool_gran_pending = false;                                // the fill just posted comes back as granules (fill_host reads them)
    s2r_host::EventSlot *pool_gran_slot = nullptr;                   // ... and this event slot's records are free again once it has
    volatile uint32_t *pool_staged = nullptr; uint32_t pool_staged_seq = 0;   // a command whose payload is written and whose sequence words
                                                                   // the caller (a device list's parent) writes with its other shards'
    uint32_t pool_idle_ticks = 200000u;                            // 2 ms without a command
    int n_cu = 0;
    float *os_buf = nullptr, *os_taps = nullptr; // 4x oversampling: [62 history + max_frames] mix at 4x rate, 63 taps
    float *sin_dev = nullptr;
    float *noise_dev = nullptr;                  // the noise table (S2rRenderParams.noise_tab), 65 536 floats
    float *per_voice_dev = nullptr; size_t per_voice_cap = 0;
    // coefficient tables of the patch (S2rTabRef): rebuilt on the device when the patch or the sample
    // rate changes
    float *tab_dev = nullptr; size_t tab_cap = 0;        // floats
    S2rTabRef tab{};
    bool tab_dirty = true; uint32_t tab_rate = 0;
    float *bank_tab_dev = nullptr; size_t bank_tab_cap = 0;      // the patch bank's coefficient tables (floats)
    unsigned long long *stamps_dev = nullptr;            // diagnostic builds (-DS2R_STAMPS): per-wave phase stamps of the last fill
    unsigned long long *timeline_dev = nullptr; uint32_t timeline_n = 0, timeline_cap = 0;   // ... and the launches' timeline
    bool use_tab = true, use_arg_events = true;
    // s2r_set_low_latency: the resident kernel (S2rResident, s2r_device.h) — running on `stream` between fills while
    // res_running; every entry point that touches the device or what the kernel's arguments were built from stops it first
    bool low_latency = false, res_running = false, res_stereo = false;
    uint32_t res_rate = 0, res_seq = 0, res_launch_id = 0;
    uint32_t *res_host = nullptr, *res_dev = nullptr;    // mapped host memory: [32] the kernel's "exited" word, and, where the CPU cannot
                                                         // write device memory, [0 .. 31] the command
    unsigned long long *res_gran = nullptr, *res_gran_dev = nullptr;   // mapped: the granules of fills of up to S2R_RES_GRANULE_FRAMES frames
    uint32_t *res_cmd = nullptr;                         // the command as the CPU writes it: res_host, or 32 words of fine-grained
    uint32_t *res_cmd_dev = nullptr;                     // DEVICE memory (large BAR) that the kernel polls without crossing the link
    bool res_cmd_vram = false;
    // The voice mixer (s2r_fill_panned, s2r_fill_buses): what the programs give their voices and what every shard
    // voice got at its note_on (s2r_mixer_keep.h), and what the mixdown holds on the device (s2r_mixer.h)
    S2rMixerKeep mixer;
    S2rVoiceMixer mixer_dev;
    // What runs behind the bus mixdown (s2r_post.h): the eight bus stages, the master section and the master limiter
    S2rPostChain post;
    float pitch_table[256];
    hipEvent_t t0 = nullptr, t1 = nullptr;
    bool timing = false, timed = false, no_flat_shortcut = false;
    uint64_t double_release = 0;
    bool uniform_window = true;                  // s2r_set_uniform_window
    uint32_t *uw_count_dev = nullptr;            // chunks rendered through the uniform window (S2rRenderParams.uw_count), one word
    s2r_voice_log_fn voice_log = nullptr;    // synth.rs:118's log::debug!, as a callback
    void *voice_log_user = nullptr;
    // A kernel that gave up a bounded wait for another kernel's (or workgroup's) work left the fill unrendered — it touches
    // neither the voices' state nor the chain heads then — while the host's pool clock and event bookkeeping had moved on:
    // the handle says so from then on instead of rendering something else than what its caller believes (import a checkpoint
    // into a new handle to go on).
    bool broken = false;
    std::string err = "";
};

namespace s2r_host __attribute__((visibility("hidden"))) {

// ---- defined in s2r_host.cpp, for the other two host files ----
// the handle's error text; returns `code` (every entry that refuses a call)
int set_err(s2r_synth *s, int code, const char *fmt, ...);
// stops the resident kernels (S2R_QUIESCE): every entry that touches the device or what a resident kernel's arguments were built from
int quiesce(s2r_synth *s);
// the checks every fill begins with (fill_rows_mixed)
int check_fill(s2r_synth *s, size_t frames, uint32_t sample_rate);
// one more event into the folded record of a shard voice (fill_rows_mixed, which splits a fill at its event frames) ...
void fold_event(s2r_synth *s, uint32_t local, uint32_t flags, float pitch, uint32_t seed, uint32_t program);
// ... and the frame-0 records that wait for the next fill folded back (fill_rows_mixed)
void fold_frame0_records(s2r_synth *top);
// events and render of `frames` frames on the handle's stream, every voice into its own row of `rows`: enqueue_fill without a mix
// (pan_segment, once per slice)
int render_rows(s2r_synth *s, uint32_t frames, uint32_t sample_rate, float *rows);

#define S2R_TRY(call) do { const int rc_t_ = (call); if (rc_t_ != S2R_OK) return rc_t_; } while (0)     // any step that returns a status
// every entry point that touches the device, or anything a running resident kernel's arguments were built from, first
#define S2R_QUIESCE(s) S2R_TRY(s2r_host::quiesce(s))

#define S2R_HIP(s, call)                                                                              \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) return s2r_host::set_err((s), S2R_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

#define S2R_REFUSE_BROKEN(s) do { if ((s)->broken) return s2r_host::set_err((s), S2R_ERR_HIP, "an earlier fill failed on the device (a bounded wait between kernels ran out): the device's voices no longer match the host's bookkeeping; destroy the handle"); } while (0)

template <class T> inline void put(T *to, T v) { if (to) *to = v; }             // an optional output of a getter
// what the post-mix chain and the voice mixer are told of the handle
inline S2rPostCtx post_ctx(const s2r_synth *s) { return S2rPostCtx{s->stream, s->cfg.max_frames, s->timing, s->mixer_dev.stems_dev(), s->out_host_dev}; }
inline S2rMixCtx mix_ctx(const s2r_synth *s) {
    return S2rMixCtx{s->stream, s->shard_voices, s->padded_voices, s->block_voices, s->n_blocks, s->mix_groups, s->cfg.max_frames, s->timing, s->out_host_dev};
}

}  // namespace s2r_host
