// s2r_render_onepole.inc — the hot kernel: one-pole LPF patches (filters.rs, the reference's live path).
// Included by s2r_render_onepole_<osc>.hip with S2R_TU_OSC defined: one translation unit per oscillator kind.
//
//   * one voice per lane; a workgroup = block_voices voices; grid = ceil(n_voices / block_voices);
//   * the fill's note events, when they ride in the kernel arguments, are applied first (apply_arg_events);
//   * the x16 path walks the fill in 16-frame chunks.  Where no lane's envelope changes stage, whole RUNS of chunks go
//     through the branch-free chunk_fast (coefficient source chosen once per run: the flat stage's constant, the
//     patch's coefficient tables, or in-lane arithmetic); around a stage change the chunk is walked in groups of 4
//     frames (closed_form_x4 on 4-wide vectors, then the recurrence per frame);
//   * frames % 16 trailing frames take the scalar path of the reference's tail (process.rs:39-48).
#include "s2r_kern_common.h"

namespace {

// One fill of the workgroup's voices.  `ctl`: what changes from fill to fill — the kernel arguments' own values (one
// launch per fill), or the command the host has just posted to the resident kernel (below).
// UWK: the launch-per-fill form of 256-thread workgroups, the one form that may have a uniform window (S2rRenderParams.uw_frames)
template <int OSC, bool FM, int MODE, int MAXT, bool UWK = false>
__device__ __forceinline__ void render_fill(const S2rRenderArgs &a, const FillCtl &ctl) {
    const S2rRenderParams &p = a.p;
    constexpr bool PV = MODE == 1;       // also store every voice's frames (mix-disabled debug/parity output)
    constexpr bool TEV = MODE == 2;      // note events that take effect inside the fill
    const uint32_t kSuper = p.super_frames;                      // 64 or 256, wave-uniform
    __shared__ uint64_t sT[S2R_EXP2F_N];
    __shared__ __attribute__((aligned(8))) float sSin[OSC == S2R_OSC_SINE ? 2048 : 2];
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    __shared__ uint32_t s_word;                                  // (one launch per fill: the workgroup's arrival ticket)

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6, n_waves = blockDim.x >> 6;
    // mixdown staging (DESIGN.md 4.3): per wave a [16 frames][64 voices + 1] tile that is written
    // voice-per-lane and read frame-per-lane, and per block the 16-voice group sums
    // sW[2][n_groups][kSuper frames] for the cross-wave combine
    constexpr uint32_t VW = 64;                                  // voices per wave
    constexpr uint32_t GW = VW / 16;                             // 16-voice groups per wave
    const uint32_t n_groups = n_waves * GW;
    float *const sW = s_dyn;                                     // [2][n_groups][kSuper]
    // (one tile: the wave's LDS operations complete in issue order, so chunk i's stores may follow the loads that add
    // up chunk i - 1 into the same rows)
    constexpr uint32_t kTile = kChunk * kTileRow;
    const uint32_t sw_floats = s2r_sw_buffers(p.frames, kSuper) * n_groups * kSuper;
    float *const tile = s_dyn + sw_floats + wave * kTile;
    // 64 floats per wave, and behind them the wave's uniform window where the launch has one (launch_mode sized it:
    // S2R_UW_PLANES planes of p.uw_frames floats; the window hangs on the scratch so that no second address is kept)
    float *const wave_scratch = s_dyn + sw_floats + n_waves * kTile + wave * (64u + (UWK ? S2R_UW_PLANES * p.uw_frames : 0u));
    uint32_t uw_chunks = 0;                                      // chunks this wave rendered through the window
    // the tile's LDS byte address (the low half of a generic pointer into LDS), for the address-free stores of chunk_fast
    const uint32_t tile_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)tile);
    const uint32_t vi = blockIdx.x * blockDim.x + tid;
#if defined(S2R_STAMPS)
    // diagnostic build: s_memtime at the phase boundaries of every wave (slot 0 entry, 1 prologue done, 2 + 2k wave work of
    // super-chunk k done, 3 + 2k its barrier and combine done, 15 exit); never in the product build
    uint32_t stamp_k = 0;
    auto stamp = [&](uint32_t slot) { if (p.stamps && lane == 0 && slot < 16u) p.stamps[(size_t)(vi >> 6) * 16u + slot] = __builtin_amdgcn_s_memtime(); };
    stamp(0);
#else
    auto stamp = [&](uint32_t) {};
    uint32_t stamp_k = 0; (void)stamp_k;
#endif
    uint32_t dbg_events = 0, dbg_dense = 0, dbg_general = 0, dbg_runs = 0, dbg_runchunks = 0;   // (diagnostic build: slots 10..14)
    unsigned long long dbg_t_dense = 0, dbg_t_run = 0;           // cycles inside the dense-event loop / the branch-free runs
    unsigned long long dbg_t_top = 0, dbg_t_sel = 0; (void)dbg_t_top; (void)dbg_t_sel;   // ... at the chunk loop's top / choosing a run
    unsigned long long dbg_t_pick1 = 0, dbg_t_casc = 0; (void)dbg_t_pick1; (void)dbg_t_casc;   // ... of that: the first look, the stage change
    (void)dbg_events; (void)dbg_dense; (void)dbg_general; (void)dbg_runs; (void)dbg_runchunks; (void)dbg_t_dense; (void)dbg_t_run;
#if defined(S2R_STAMPS)
#define S2R_DBG_NOW() __builtin_amdgcn_s_memtime()
#else
#define S2R_DBG_NOW() 0ull
#endif

    tl_mark(p.timeline, p.tl_slot, 0);
    if (tid < S2R_EXP2F_N) sT[tid] = c_exp2f_table[tid];
    if (OSC == S2R_OSC_SINE)
        for (uint32_t i = tid; i < 1024u; i += blockDim.x) { sSin[2u * i] = p.sin_table[(i + 1023u) & 1023u]; sSin[2u * i + 1u] = p.sin_table[i]; }

    apply_arg_events(p, ctl.n_events, ctl.ev, vi, lane);

    // ---- load per-voice state (coalesced SoA reads) ----
    // Every word of the voice is asked for at once, whether or not the flags will say the voice is started: the loads
    // are one trip to memory instead of two (the flags first, then — under their mask — the rest).
    const bool in_range = vi < p.n_voices;
    // Two streams (S2rOverlapWords): this fill's chain heads and event copy come from a kernel on the other stream —
    // normally long done; one lane makes sure, and everything read of them below is read `sc1` (ov_load)
    // One launch per fill (S2rMixTail): the workgroup copies ITS slice of the fill's records and publishes its own voices'
    // chain heads here — write-through, read `sc1` like the other stream's
    const bool ovh = TEV && (ctl.fused || ctl.ov_heads_counter != nullptr);
    if (TEV && ctl.fused) { fused_heads(ctl); stamp(7); }
    else if (ovh) {
        if (tid == 0) { const bool ok = ov_wait(ctl.ov_heads_counter, ctl.ov_heads_target); if (!ok) ov_raise(ctl.fail, 1u); s_word = ok ? 1u : 0u; }
        __syncthreads();
        if (s_word == 0u) {
            // The chain heads never came (bounded wait): the fill is NOT rendered — the voices' state and their chains stay as
            // they are, the workgroup's row is silence, the mix is told the row is there — and the host, which has raised word
            // `fail`, reports the fill and refuses the handle from then on (s2r_host.cpp: broken).
            float *row = ctl.partials + (size_t)blockIdx.x * p.frames_stride;
            for (uint32_t f = 4u * tid; f < p.frames_stride && f < ((ctl.frames + 3u) & ~3u); f += 4u * blockDim.x) ov_store4(row + f, (f4){0.0f, 0.0f, 0.0f, 0.0f});
            if (ctl.ov_render_counter != nullptr) ov_signal(ctl.ov_render_counter);
            return;
        }
    }
    auto tev_at = [&](int32_t i) -> S2rTimedEvent { return tev_load(ctl.tev, ovh, i); };
    uint32_t flags = 0u, w_offset = 0u, w_release = 0u, w_seed = 0u;
    float w_pitch = 440.0f, w_phase = 0.0f, w_last = 0.0f;
    int32_t ev_idx = -1;
    if (in_range) {
        flags = p.v.flags[vi];
        w_pitch = p.v.pitch[vi]; w_offset = p.v.offset[vi]; w_release = p.v.release[vi];
        w_phase = p.v.phase[vi]; w_last = p.v.lpf_last[vi]; w_seed = p.v.seed[vi];
        if (TEV) ev_idx = ovh ? ov_load(ctl.heads + vi) : ctl.heads[vi];
    }
    bool live = (flags & S2R_VF_STARTED) != 0u;                // synth.rs:178
    // timed events: this voice's chain for the fill (taken over and cleared for the next fill)
    // (the voice's NEXT event sits in registers, fetched when the one before it is applied: with one wave per SIMD a
    // dependent trip to memory at the moment the event is due is a stall nothing else fills)
    uint32_t ev_frame = 0xffffffffu;
    S2rTimedEvent ev_next{};
    bool ev_dirty = false, ev_restart = false;
    if (TEV && ev_idx >= 0) {
        ev_next = tev_at(ev_idx);
        ev_frame = ev_next.frame;
        if (ovh) ov_store(ctl.heads + vi, (int32_t)-1); else ctl.heads[vi] = -1;
    }
    VoiceRegs r;
    r.pitch = live ? w_pitch : 440.0f;
    r.offset = live ? w_offset : 0u;
    r.release_u = live ? w_release : 0u;
    r.released = live && (flags & S2R_VF_RELEASED) != 0u;
    r.phase = live ? w_phase : 0.0f;
    r.last = live ? w_last : 0.0f;
    uint32_t seed = live ? w_seed : 0u;
    uint32_t program_now = 0u;
    // A chain that starts at frame 0 starts with the fill's folded untimed events (the host merges them into the chains
    // when the fill has timed events too, s2r_host.cpp flush_events): applied here, to the words just loaded, before
    // anything is derived from them — *voice = Voice { .. } (synth.rs:63-69) or release_frame_offset =
    // current_frame_offset (:74-75) — so that a cohort of note-ons costs its waves a few selects, not a restart of 64
    // voices inside the frame loop.
    if (TEV && ev_frame == 0u) {
        const S2rTimedEvent e = ev_next;
        if (e.flags & S2R_EV_RESTART) {
            r.pitch = e.pitch; r.offset = 0u; r.release_u = 0u;
            r.released = (e.flags & S2R_EV_RELEASE) != 0u;
            r.phase = 0.0f; r.last = 0.0f;
            // (the two words only a restart needs are read again from the record instead of riding in registers with every
            // lane's next event: the timed-event kernel is the one at the register file's limit)
            { const S2rTimedEvent er = tev_at(ev_idx); seed = er.seed; program_now = er.program; }
            live = true; ev_restart = true;
        } else if ((e.flags & S2R_EV_RELEASE) && live && !r.released) {
            r.released = true;
            r.release_u = r.offset;
        }
        ev_dirty = true;
        ev_idx = e.next;
        ev_frame = 0xffffffffu;
        if (ev_idx >= 0) { ev_next = tev_at(ev_idx); ev_frame = ev_next.frame; }
    }
    // A RELEASE that is the voice's next event is booked at once, whatever its frame.  The x16 ADSR is a pure function of
    // the frame offset and the release offset (simdtest.rs:270-331), and a release offset that lies ahead changes nothing
    // before the offset reaches it: the cascade's `t < max(release, attack + decay)` keeps the voice where it is until
    // then, and from then on it is in its release — exactly what applying the event at its boundary does
    // (synth.rs:74-75: release_frame_offset = current_frame_offset AT that boundary = the fill's first offset + the
    // event's frame).  So a note-off costs its wave nothing until the envelope actually turns: no run ends at it, no wave
    // walks chunk by chunk because of it.  (A voice in sustain gets a finite stage end — a threshold on a chunk boundary,
    // which the run logic handles like any other.)  Only restarts, and releases of voices older than 2^24 frames, stay in
    // the chain as events.
    bool took_release = false;
    auto take_releases = [&]() {
        while (ev_idx >= 0 && !(ev_next.flags & S2R_EV_RESTART)) {
            // (only where f32 tells every earlier offset from the release offset: up to 2^24.  Beyond, (float)(rel - 1) may
            // equal (float)rel and the voice would turn a frame early; such an event stays in the chain.  The offset base
            // of a voice restarted inside this fill is minus the restart's frame: small once the event's frame is added.)
            const uint32_t rel = r.offset + ev_next.frame;
            const bool base_ok = r.offset <= (1u << 24) || r.offset >= 0u - ctl.frames;
            if (!(base_ok && rel <= (1u << 24))) break;
            if ((ev_next.flags & S2R_EV_RELEASE) && live && !r.released) {
                r.released = true;
                r.release_u = rel;
                took_release = true;
            }
            ev_dirty = true;
            ev_idx = ev_next.next;
            ev_frame = 0xffffffffu;
            if (ev_idx >= 0) { ev_next = tev_at(ev_idx); ev_frame = ev_next.frame; }
        }
    };
    if (TEV) take_releases();
    r.seed_rot = (seed << 5) | (seed >> 27);

    const float rel_f = r.released ? (float)r.release_u : 4294967296.0f;     // u32::MAX as f32
    r.ro_a = __builtin_fmaxf(rel_f, p.amp.sus_off); r.end_a = r.ro_a + p.amp.R;
    r.ro_m = __builtin_fmaxf(rel_f, p.mod.sus_off); r.end_m = r.ro_m + p.mod.R;

    // mod_env_to_osc_freq == 0: pow(2, mod*0) == 1 exactly, so freq == 1.0 * pitch and the
    // period (and everything derived from it by correctly rounded divisions) is constant.
    OscK k_const = make_osck<OSC>(p.sr / (1.0f * r.pitch));
    uint32_t seed_now = seed;

    // envelope stage registers: the cascade for the fill's first frame, run here once so that the first
    // chunk can already take the branch-free path (a timed event or a stage boundary resets thr_min to
    // -inf, which sends the next frame through the cascade again)
    EnvRun ea = env_stage_at(p.amp, r.ro_a, r.end_a, (float)r.offset);
    EnvRun em = env_stage_at(p.mod, r.ro_m, r.end_m, (float)r.offset);
    float thr_min = __builtin_fminf(ea.s3, em.s3);
    FlatCache fc;
    fc.xc = 0.0f; fc.k = k_const;

    __syncthreads();
    const bool have_tab = p.tab.base != nullptr && !p.no_flat_shortcut;
    // (wave-uniform choice; computing them takes two pow and two exp per lane, needing the exp2 table in LDS)
    FlatConsts fcc = (have_tab && (!FM || p.tab.fm_plane != 0u)) ? flat_consts_from_tables<OSC, FM>(p, r.pitch) : make_flat_consts<OSC, FM>(p, r.pitch, sT);
    fc = refresh_flat<OSC, FM>(fcc, em, fc);

    const bool wave_live = __ballot(live || ev_idx >= 0) != 0ull;
    bool wave_events = TEV && __ballot(ev_idx >= 0) != 0ull;     // some lane still has a timed event in this fill
    const uint32_t x16_frames = ctl.frames & ~(uint32_t)(kChunk - 1);      // frames in full 16-chunks
    // preconditions of the branch-free chunk that hold for the whole fill once they hold at its start
    // (phase' = fmodf(phase + 1/period, 1) stays in [0,1) for a positive period)
    // Under oscillator FM the period constants are per-frame values — except while every lane's mod envelope
    // is flat, when they are the ones cached at stage entry (fc.k): that case is checked per run.
    // (a NORMAL period: RN(period * phase) stays below a normal period, but on a denormal one's grid of 2^-149 it can round up
    // to the period itself, where fmodf(off, period) is +0 and not `off` — such a wave takes the general path)
    const bool fast_ok = __ballot(!(r.phase >= 0.0f && r.phase < 1.0f)) == 0ull &&
        (FM || __ballot(!(k_const.period >= 0x1p-126f && k_const.period < __builtin_inff())) == 0ull);
    const size_t pv_base = (size_t)vi * ctl.frames;
    float *bp = ctl.partials + (size_t)blockIdx.x * p.frames_stride;
    uint32_t buf = 0;

    // after each 16-frame chunk lane j adds, for frame (j & 15), the 16 voices of group (j >> 4) in
    // index order (the reference's own order within the group, synth.rs:177-195) and files the
    // group sum for the cross-wave combine
    auto reduce_chunk = [&](uint32_t f_base, uint32_t n_frames) {
        const uint32_t f = lane & 15u, grp = lane >> 4;
        __builtin_amdgcn_wave_barrier();                         // the tile's stores (other lanes') before these loads
        if (f < n_frames) {
            const float *src = tile + f * kTileRow + grp * 16u;
            float acc = src[0];
#pragma unroll
            for (int k = 1; k < 16; ++k) acc += src[k];
            sW[(buf * n_groups + wave * GW + grp) * kSuper + f_base + f] = acc;
        }
        __builtin_amdgcn_wave_barrier();                         // ... and these loads before the next chunk's stores
    };

    // note events that land on the 16-frame boundary `fpos` (synth.rs:61-80 applied between two
    // 16-frame sample() calls, main.rs:140-142): restart or release this lane's voice
    // Wave-uniform facts about the lanes' stages that the run logic needs; they change only when some lane changes
    // stage (a threshold, a timed event), so they are looked at then, not per run (each is a VALU compare + a scalar
    // round trip the lone wave waits for):
    //   w_flat    every started voice's mod envelope in a zero-slope stage (and, under FM, valid cached constants)
    //   w_aflat   every started voice's amplitude envelope in a zero-slope stage
    //   w_aligned chunk starts are multiples of 16 frames and rotl(seed, 5) has a zero low nibble, on every lane
    //   w_small   no offset passes 2^24 during this fill
    //   w_uni     a cohort: all 64 lanes started, with the same offset, seed, amplitude line and mod stage, whose table
    //             entry advances with the offset (tab_cursor) and is therefore the same too: what chunk_fast<UW> needs
    bool w_flat = false, w_aflat = false, w_aligned = false, w_small = false, w_uni = false;
    auto classify_uniform = [&]() {
        if (!(UWK && !FM) || p.uw_frames == 0u) return;           // (no window: w_uni stays false)
        const TabCur c = tab_cursor(p.tab, em.s4, r.ro_m > p.mod.sus_off, r.release_u, live);
        auto differs = [](uint32_t v) { return v != (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
        const bool odd = !live || c.mask != 0xffffffffu || differs((uint32_t)c.idx) || differs(r.offset) || differs(r.seed_rot) ||
                         differs(s2r_f2u(ea.s0)) || differs(s2r_f2u(ea.s1)) || differs(s2r_f2u(ea.s2)) || differs(s2r_f2u(em.s4));
        w_uni = __ballot(odd) == 0ull;
    };
    auto reclassify_stages = [&]() {                             // what a stage change can move
        w_flat = !p.no_flat_shortcut && __ballot(live && em.s0 != 0.0f) == 0ull &&
                 (!FM || __ballot(!(fc.k.period >= 0x1p-126f && fc.k.period < __builtin_inff())) == 0ull);
        w_aflat = __ballot(live && ea.s0 != 0.0f) == 0ull;
        classify_uniform();
    };
    auto reclassify = [&]() {
        reclassify_stages();
        w_aligned = p.noise_tab != nullptr && __ballot(((r.offset | r.seed_rot) & 15u) != 0u) == 0ull;
        // (the host refuses a fill that would carry an offset past u32::MAX, so the sum wraps only for a voice restarted
        // inside this fill, whose offset base is minus the event's frame: small, as the wrapped sum says)
        w_small = __ballot(r.offset + ctl.frames > (1u << 24)) == 0ull;
    };
    reclassify();
    stamp(1);

    // note events that land on the 16-frame boundary `fpos` (synth.rs:61-80 applied between two
    // 16-frame sample() calls, main.rs:140-142): restart or release this lane's voice
    // The lane's part of an event boundary: applies this lane's events of frame `fpos` (if any) and moves its envelope
    // stage registers on.  No wave-level decision in here (no ballot): the callers look at the wave once, afterwards.
    // Returns whether the lane was restarted (its offset base and seed may have changed).
    auto apply_events_lane = [&](uint32_t fpos) -> bool {
        bool restarted = false, released_now = false;
        took_release = false;
        while (ev_frame == fpos) {
            const S2rTimedEvent e = ev_next;
            if (e.flags & S2R_EV_RESTART) {                  // *voice = Voice { .. }, synth.rs:63-69
                r.pitch = e.pitch;
                r.offset = 0u - fpos;                        // current_frame_offset == 0 at frame fpos
                r.release_u = 0u;
                r.released = (e.flags & S2R_EV_RELEASE) != 0u;
                r.phase = 0.0f; r.last = 0.0f;
                const S2rTimedEvent er = tev_at(ev_idx);
                seed_now = er.seed;
                r.seed_rot = (seed_now << 5) | (seed_now >> 27);
                program_now = er.program;
                live = true; ev_restart = true; restarted = true;
                k_const = make_osck<OSC>(p.sr / (1.0f * r.pitch));
            } else if ((e.flags & S2R_EV_RELEASE) && live && !r.released) {   // synth.rs:74-75
                r.released = true;
                r.release_u = r.offset + fpos;
                released_now = true;
            }
            ev_dirty = true;
            ev_idx = e.next;
            ev_frame = 0xffffffffu;
            if (ev_idx >= 0) { ev_next = tev_at(ev_idx); ev_frame = ev_next.frame; }
            take_releases();                                 // (what follows a restart is usually its release)
        }
        const float rf = r.released ? (float)r.release_u : 4294967296.0f;
        r.ro_a = __builtin_fmaxf(rf, p.amp.sus_off); r.end_a = r.ro_a + p.amp.R;
        r.ro_m = __builtin_fmaxf(rf, p.mod.sus_off); r.end_m = r.ro_m + p.mod.R;
        const float t0 = (float)(r.offset + fpos);
        if (restarted) {
            // a restart (rare as a timed event): the whole cascade for the boundary's frame and, under FM, the voice's
            // flat-stage constants
            if (FM) {
                const FlatConsts n = (have_tab && p.tab.fm_plane != 0u) ? flat_consts_from_tables<OSC, FM>(p, r.pitch) : make_flat_consts<OSC, FM>(p, r.pitch, sT);
                fcc.k_s = n.k_s; fcc.k_0 = n.k_0;
            }
            ea = env_stage_at(p.amp, r.ro_a, r.end_a, t0);
            em = env_stage_at(p.mod, r.ro_m, r.end_m, t0);
        } else if (released_now) {
            // A release (the common timed event).  The cascade (simdtest.rs:288-292) tests attack and decay first, and
            // the release offset is clamped to their end (:283): an envelope still in attack or decay keeps its stage,
            // line and threshold; one in sustain (t0 >= attack + decay, so the clamp does not bind and release_offset
            // == t0) enters the release line at its first frame — or, with a zero release time, the end.  A dozen
            // instructions on the lanes concerned instead of two full cascades of compares and selects.
            if (ea.s4 == 2.0f) { const bool rel = t0 < r.end_a;
                ea.s0 = rel ? p.amp.slope_rel : 0.0f; ea.s1 = rel ? r.ro_a : 0.0f; ea.s2 = rel ? p.amp.S : 0.0f;
                ea.s3 = rel ? r.end_a : __builtin_inff(); ea.s4 = rel ? 3.0f : 4.0f; }
            if (em.s4 == 2.0f) { const bool rel = t0 < r.end_m;
                em.s0 = rel ? p.mod.slope_rel : 0.0f; em.s1 = rel ? r.ro_m : 0.0f; em.s2 = rel ? p.mod.S : 0.0f;
                em.s3 = rel ? r.end_m : __builtin_inff(); em.s4 = rel ? 3.0f : 4.0f; }
        }
        else if (took_release) {
            // a release ahead of a voice in sustain: the stage now ends where the release begins
            if (ea.s4 == 2.0f) ea.s3 = r.ro_a;
            if (em.s4 == 2.0f) em.s3 = r.ro_m;
        }
        thr_min = __builtin_fminf(ea.s3, em.s3);
        fc = refresh_flat<OSC, FM>(fcc, em, fc);
        return restarted;
    };

    // note events that land on the 16-frame boundary `fpos` (synth.rs:61-80 applied between two
    // 16-frame sample() calls, main.rs:140-142): restart or release the voices concerned, then what the wave has to agree on
    auto apply_events_at = [&](uint32_t fpos) {
        if (!wave_events || __ballot(ev_frame == fpos) == 0ull) return;
        dbg_events += (uint32_t)__builtin_popcountll(__ballot(ev_frame == fpos));
        bool restarted = false;
        if (ev_frame == fpos) restarted = apply_events_lane(fpos);
        if (__ballot(restarted) != 0ull) {                       // an offset base or a seed moved
            w_aligned = p.noise_tab != nullptr && __ballot(((r.offset | r.seed_rot) & 15u) != 0u) == 0ull;
            w_small = __ballot(r.offset + ctl.frames > (1u << 24)) == 0ull;
        }
        wave_events = __ballot(ev_idx >= 0) != 0ull;
        w_flat = !p.no_flat_shortcut && __ballot(live && em.s0 != 0.0f) == 0ull &&
                 (!FM || __ballot(!(fc.k.period >= 0x1p-126f && fc.k.period < __builtin_inff())) == 0ull);
        w_aflat = __ballot(live && ea.s0 != 0.0f) == 0ull;
        classify_uniform();
    };

    // The two stage changes that are as frequent as the note-offs themselves, by hand (the cascade is two dozen compares
    // and selects per envelope): a release that has run out (stage 3, t0 at or past its threshold) goes to the end stage;
    // a sustain whose booked release begins (stage 2, threshold ro: take_releases) enters the release line at its first
    // frame — or, with nothing left of the release, the end — exactly as the cascade would: the lane has passed attack
    // and decay (offsets only grow), so simdtest.rs:288-292 is down to `t < ro` (false) and `t < end`.  Everything else
    // takes the cascade.
    auto end_of_release = [&](float t0) {
        if (ea.s4 == 3.0f && !(t0 < ea.s3)) { ea.s0 = 0.0f; ea.s1 = 0.0f; ea.s2 = 0.0f; ea.s3 = __builtin_inff(); ea.s4 = 4.0f; }
        if (em.s4 == 3.0f && !(t0 < em.s3)) { em.s0 = 0.0f; em.s1 = 0.0f; em.s2 = 0.0f; em.s3 = __builtin_inff(); em.s4 = 4.0f; }
        if (ea.s4 == 2.0f && !(t0 < ea.s3)) { const bool rel = t0 < r.end_a;
            ea.s0 = rel ? p.amp.slope_rel : 0.0f; ea.s1 = rel ? r.ro_a : 0.0f; ea.s2 = rel ? p.amp.S : 0.0f;
            ea.s3 = rel ? r.end_a : __builtin_inff(); ea.s4 = rel ? 3.0f : 4.0f; }
        if (em.s4 == 2.0f && !(t0 < em.s3)) { const bool rel = t0 < r.end_m;
            em.s0 = rel ? p.mod.slope_rel : 0.0f; em.s1 = rel ? r.ro_m : 0.0f; em.s2 = rel ? p.mod.S : 0.0f;
            em.s3 = rel ? r.end_m : __builtin_inff(); em.s4 = rel ? 3.0f : 4.0f; }
    };

    // Software pipeline of the transpose-and-add of the branch-free chunks: the 16 loads of chunk i's column sums are
    // issued right behind its stores (the wave's LDS operations complete in issue order), the serial adds and the store
    // of the sum are placed in FRONT of the next fast chunk's stores — whenever that chunk comes: the pending sum
    // (tv, pend_dst) survives run boundaries, events and stage changes and is flushed before anything else touches the
    // tile.  Not behind the stores: the compiler does not count the inline-asm stores of chunk_fast, so an
    // `s_waitcnt lgkmcnt(N)` it places behind some of them waits for those stores too (SQ_WAIT_ANY was a third of the
    // wave's cycles with the adds at the end of the chunk).
    const uint32_t rf = lane & 15u, rgrp = lane >> 4;
    const float *const tsrc = tile + rf * kTileRow + rgrp * 16u;
    const f4 *const tsrc4 = reinterpret_cast<const f4 *>(tsrc);          // (16-byte aligned: kTileRow)
    float *const sw_dummy = wave_scratch + lane;                 // where a sum goes when none is pending
    float *pend_dst = sw_dummy;
    // (the 16 values are read here, at the head of the NEXT chunk's basic block — whose first instructions do not depend on
    // them and cover the reads' latency — rather than behind the chunk that stored them: sixteen registers fewer live
    // across every loop, run boundary and stage change)
    auto tsum = [&]() {
        float tv[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) { const f4 t4 = tsrc4[q]; tv[4 * q] = t4.x; tv[4 * q + 1] = t4.y; tv[4 * q + 2] = t4.z; tv[4 * q + 3] = t4.w; }
        float acc = tv[0];
#pragma unroll
        for (int q = 1; q < 16; ++q) acc += tv[q];
        return acc;
    };
    auto flush_pending = [&]() {                                 // wave-uniform: pend_dst is the same kind on every lane
        *pend_dst = tsum();
        pend_dst = sw_dummy;
        __builtin_amdgcn_wave_barrier();
    };

    // Frames are walked in super-chunks of kSuper (one barrier and one cross-wave combine each), each
    // made of 16-frame chunks (one wave-local transpose-and-add each).
    bool dense_stay = false;                                     // the dense-event loop was cut short by a super-chunk's end
    for (uint32_t sc0 = 0; sc0 < ctl.frames; sc0 += kSuper) {
        const uint32_t n_sc = (ctl.frames - sc0 < kSuper) ? (ctl.frames - sc0) : kSuper;
        const uint32_t n_x16 = (x16_frames > sc0) ? ((x16_frames - sc0 < n_sc) ? (x16_frames - sc0) : n_sc) : 0u;
        if (wave_live) {
            for (uint32_t c16 = 0; c16 < n_x16; c16 += kChunk) {
                const unsigned long long dbg_tt0 = S2R_DBG_NOW();
                // (the dense-event loop, entered when the wave's next event is at most two chunks ahead, handles the events of
                // its first boundary itself: no second look at them here)
                if (TEV) apply_events_at(sc0 + c16);
                // (entered when the wave's next event is at most two chunks ahead)
                // (under FM its chunks take per-frame periods from the tables' FM plane, flat envelope or not: the pitch bound of
                // the run logic below; a voice restarted inside the loop gets a MIDI pitch, which meets it at any sample rate)
                const bool dense = TEV && wave_events && fast_ok && have_tab && w_small && w_aligned && p.noise_level == 0.0f &&
                                   (!FM || __ballot(live && !(p.sr >= r.pitch * 0x1p-115f)) == 0ull) &&
                                   (dense_stay || wave_min_u32((ev_frame - (sc0 + c16)) >> 4) <= 2u);
                dbg_t_top += S2R_DBG_NOW() - dbg_tt0;
                if (dense) {
                    // DENSE EVENTS.  The pool's note-offs cluster on its youngest voices (synth.rs:82-90 releases the LAST
                    // active match), so under a busy event stream some waves see an event on almost every 16-frame
                    // boundary.  For them the run logic — a decision, a variant, a loop set-up per run, code far apart —
                    // costs more than the chunks (measured with tools/stamps.py: ~3000 cycles per event against ~1700 per
                    // chunk).  While such a wave still expects events it walks chunk by chunk through ONE loop: one
                    // compare + ballot says whether any lane has an event or a threshold at this boundary (then: apply,
                    // re-run the cascade for the lanes at a threshold), and the chunk runs in the variant that is valid for
                    // any mix of stages (coefficients from the tables, amplitude per frame).
                    // Per chunk, the common boundaries cost ONE ballot ("some lane has an event that is not a plain release,
                    // or a threshold") and two selects.  The cheapest and, on a pool's youngest voices, the commonest event
                    // is a single release of a voice whose envelopes are still in attack or decay: the cascade tests those
                    // stages first and the release offset is clamped to their end (simdtest.rs:283,288-292), so stages,
                    // lines and thresholds stay as they are and only the voice's release bookkeeping moves (synth.rs:74-75)
                    // — and that is not needed before the wave next runs a cascade or leaves this loop: the lane only notes
                    // the release's offset (pend_rel) and commit_plain() does the rest then.  Every fourth chunk the wave
                    // looks where its next event is.
                    bool inside = false;                         // a threshold strictly inside the chunk: general path
                    bool idle_exit = false;                      // the next event is more than 8 chunks away: the run logic does better
                    constexpr uint32_t kNoRel = 0xffffffffu;
                    uint32_t pend_rel = kNoRel;                  // offset of this lane's plain release, not yet booked
                    auto commit_plain = [&]() {
                        if (pend_rel != kNoRel) {
                            if ((ev_next.flags & S2R_EV_RELEASE) && live && !r.released) {
                                r.released = true;
                                r.release_u = pend_rel;
                                const float rf = (float)pend_rel;
                                r.ro_a = __builtin_fmaxf(rf, p.amp.sus_off); r.end_a = r.ro_a + p.amp.R;
                                r.ro_m = __builtin_fmaxf(rf, p.mod.sus_off); r.end_m = r.ro_m + p.mod.R;
                            }
                            ev_dirty = true; ev_idx = -1;
                            pend_rel = kNoRel;
                        }
                    };
                    // this lane's next event, if it has one, is a plain release (looked at again after every cascade)
                    auto plain_now = [&]() { return !(ev_next.flags & S2R_EV_RESTART) && ev_next.next < 0 && ea.s4 <= 1.0f && em.s4 <= 1.0f; };
                    bool plain = plain_now();
                    TabCur cur = tab_cursor(p.tab, em.s4, r.ro_m > p.mod.sus_off, r.release_u, live);
                    const unsigned long long dbg_td0 = S2R_DBG_NOW();
                    // Two loops: the outer one handles a boundary in full (events of any kind, thresholds, the cascade);
                    // the inner one runs chunk after chunk while the boundaries ahead need nothing but the two selects —
                    // it modifies none of the wave's other state, so nothing else is merged per chunk.
                    while (c16 < n_x16 && wave_events && !idle_exit) {
                        {
                            const uint32_t fpos = sc0 + c16;
                            bool lane_bad = false;
                            const bool hit = ev_frame == fpos;
                            commit_plain();
                            if (hit) {
                                dbg_events += 1u;
                                if (apply_events_lane(fpos)) lane_bad = ((r.offset | r.seed_rot) & 15u) != 0u || r.offset + ctl.frames > (1u << 24);
                            }
                            const uint32_t oc = r.offset + fpos;
                            const float t0 = (float)oc;
                            end_of_release(t0);
                            thr_min = __builtin_fminf(ea.s3, em.s3);
                            if (!(t0 < thr_min)) {               // (lane-masked: the cascade for the lanes at another threshold)
                                ea = env_stage_at(p.amp, r.ro_a, r.end_a, t0);
                                em = env_stage_at(p.mod, r.ro_m, r.end_m, t0);
                                thr_min = __builtin_fminf(ea.s3, em.s3);
                            }
                            fc = refresh_flat<OSC, FM>(fcc, em, fc);
                            cur = tab_cursor(p.tab, em.s4, r.ro_m > p.mod.sus_off, r.release_u, live);
                            plain = plain_now();
                            wave_events = __ballot(ev_idx >= 0) != 0ull;
                            // a threshold strictly inside the chunk, or a restart that moved an offset base or a seed off
                            // the grid: out of this loop
                            const bool bad_align = __ballot(lane_bad) != 0ull;
                            inside = __ballot(!((float)(oc + (kChunk - 1u)) < thr_min)) != 0ull;
                            if (bad_align) { w_aligned = false; w_small = false; }      // (reclassify() below looks again)
                            if (inside || bad_align) break;
                        }
                        for (;;) {
                            const uint32_t fpos = sc0 + c16;
                            const uint32_t oc = r.offset + fpos;
                            ++dbg_dense;
                            *pend_dst = tsum();
                            float *pvd = (PV && in_range) ? p.per_voice + pv_base + fpos : nullptr;
                            const float *tp = p.tab.base + (ptrdiff_t)(cur.idx + (int32_t)(oc & cur.mask));
                            chunk_fast<OSC, 1, 0, FM, 2, false>(p, r, ea, em, fc, FM ? fc.k : k_const, oc, tp, sT, sSin, live, tile_lds, pvd);
                            __builtin_amdgcn_wave_barrier();
                            pend_dst = sW + (buf * n_groups + wave * GW + rgrp) * kSuper + rf + c16;
                            c16 += kChunk;
                            if (c16 >= n_x16) break;
                            // the next boundary
                            const uint32_t fnext = fpos + kChunk, onext = oc + kChunk;
                            const bool hit = ev_frame == fnext;
                            if (__ballot((hit && !plain) || !((float)(onext + (kChunk - 1u)) < thr_min)) != 0ull) break;
                            pend_rel = hit ? onext : pend_rel;   // (a lane has at most one: a plain release is its last event)
                            ev_frame = hit ? 0xffffffffu : ev_frame;
                            if ((c16 & 0x30u) == 0x30u) {        // every fourth chunk: what does the wave still expect?
                                // nothing -> out; a few events far apart (the next one more than 8 chunks away) -> the run
                                // logic does better with the stretch in between; many -> stay: every change between this
                                // loop and the run logic costs about two chunks (tools/stamps.py)
                                const uint64_t pending = __ballot(ev_frame != 0xffffffffu);
                                if (pending == 0ull) { idle_exit = true; break; }
                                if (__builtin_popcountll(pending) <= 4) {
                                    const uint32_t nxt = wave_min_u32(ev_frame);
                                    if (((nxt - fnext) >> 4) > 8u) { idle_exit = true; break; }
                                }
                            }
                        }
                    }
                    commit_plain();
                    wave_events = __ballot(ev_idx >= 0) != 0ull;
                    // (left only because the super-chunk ended: back in here at the next one's first chunk)
                    dense_stay = wave_events && !idle_exit && !inside && c16 >= n_x16;
                    dbg_t_dense += S2R_DBG_NOW() - dbg_td0;
                    reclassify();
                    if (c16 >= n_x16) break;
                    if (!inside) { c16 -= kChunk; continue; }    // events are behind (or alignment is gone): the run logic takes over at c16
                }
                const unsigned long long dbg_ts0 = S2R_DBG_NOW();
                const uint32_t o_chunk = r.offset + sc0 + c16;
                if (fast_ok) {
                    // How many 16-frame chunks can run branch-free from here?  Offsets only grow and the
                    // active stages' thresholds stay put on this path, so if the LAST frame of a run is below
                    // every lane's next threshold, every earlier frame is too: one wave-uniform decision per
                    // run (up to the rest of the super-chunk) instead of several per chunk — with one wave per
                    // SIMD every VALU->scalar decision and taken branch is a bubble nothing else fills.
                    const uint32_t left = (n_x16 - c16) / kChunk;
                    // n chunks from here are clear when their LAST frame is below every lane's next threshold and no lane
                    // has a timed event before their end (events at this very boundary were just applied)
                    auto clear_for = [&](uint32_t n) {
                        bool bad = !((float)(o_chunk + n * kChunk - 1u) < thr_min);
                        if (TEV) bad = bad || ev_frame < sc0 + c16 + n * kChunk;
                        return __ballot(bad) == 0ull;
                    };
                    // The longest clear run, in one reduction: per lane the chunks before its next threshold — the largest n
                    // with o_chunk + 16 n - 1 < thr, i.e. n < (thr - o_chunk + 1) / 16 (exact in f32 below 2^24: thr - t0 is a
                    // multiple of thr's ulp no larger than thr) — and before its next event, then the wave's minimum; the
                    // exact test confirms it (offsets beyond 2^24 round).
                    auto pick_run = [&]() -> uint32_t {
                        const float q = ((thr_min - (float)o_chunk) + 1.0f) * 0.0625f;
                        float nf = __builtin_ceilf(q) - 1.0f;
                        nf = __builtin_fminf(__builtin_fmaxf(nf, 0.0f), (float)left);        // (a NaN threshold cannot occur; inf clamps)
                        uint32_t n = (uint32_t)nf;
                        if (TEV) { const uint32_t ne = (ev_frame - (sc0 + c16)) >> 4; n = ne < n ? ne : n; }
                        n = wave_min_u32(n);
                        if (n == 0u) return 0u;
                        if (clear_for(n)) return n;
                        return (n > 1u && clear_for(1u)) ? 1u : 0u;
                    };
                    // A stage that ends exactly at this chunk's first frame — the common case: envelope times are usually
                    // whole multiples of 16 frames past a note event that itself sits on a chunk boundary (4800 = 16 * 300),
                    // and booked releases are thresholds on such boundaries — is looked for first: the lanes that have
                    // reached their threshold move on (by hand, or through the cascade as at the start of the fill), and
                    // the run is chosen once, afterwards.  (A threshold strictly inside the chunk gives a run of 0: general
                    // path.)
                    {
                        const float t0 = (float)o_chunk;
                        if (__ballot(!(t0 < thr_min)) != 0ull) {
                            end_of_release(t0);
                            thr_min = __builtin_fminf(ea.s3, em.s3);
                            if (!(t0 < thr_min)) {
                                ea = env_stage_at(p.amp, r.ro_a, r.end_a, t0);
                                em = env_stage_at(p.mod, r.ro_m, r.end_m, t0);
                                thr_min = __builtin_fminf(ea.s3, em.s3);
                            }
                            fc = refresh_flat<OSC, FM>(fcc, em, fc);
                            reclassify_stages();
                        }
                    }
                    const unsigned long long dbg_ts1 = S2R_DBG_NOW();
                    dbg_t_casc += dbg_ts1 - dbg_ts0;
                    uint32_t run = pick_run();
                    dbg_t_pick1 += S2R_DBG_NOW() - dbg_ts1;
                    // where the run's coefficients come from (wave-uniform): every started voice's mod envelope in a
                    // zero-slope stage -> the constants cached at stage entry; else the patch's tables (offsets below
                    // 2^24); else in-lane arithmetic (not under FM: such a run takes the general path)
                    bool flat = false, tab_ok = false, offs_small = false;
                    if (run) {
                        run = (uint32_t)__builtin_amdgcn_readfirstlane((int)run);
                        offs_small = w_small || __ballot(o_chunk + run * kChunk > (1u << 24)) == 0ull;
                        flat = w_flat;
                        tab_ok = !flat && have_tab && offs_small;
                        if (FM && !flat && !tab_ok) run = 0;
                        // (the tables' per-frame periods are sr / (2^(mod * amount) * pitch) with the power at most 2^10: not
                        // below 2^-125 while sr >= pitch * 2^-115.  This covers underflow only; a product 2^x * pitch that
                        // overflows makes the period +0 and the reference's sample NaN, which nothing here reproduces)
                        if (FM && !flat && __ballot(live && !(p.sr >= r.pitch * 0x1p-115f)) != 0ull) run = 0;
                    }
                    if (run) {
                        ++dbg_runs; dbg_runchunks += run;
                        const unsigned long long dbg_tr0 = S2R_DBG_NOW();
                        dbg_t_sel += dbg_tr0 - dbg_ts0;
                        float *const sw_row = sW + (buf * n_groups + wave * GW + rgrp) * kSuper + rf;
                        // this lane's entry in the coefficient tables for the run's first frame; it advances with the
                        // offset in the attack, decay and release stages and stays put in sustain / after the end
                        const TabCur cur = tab_cursor(p.tab, em.s4, r.ro_m > p.mod.sus_off, r.release_u, live);
                        auto run_chunks = [&](auto src_tag, auto nz_tag, auto aflat_tag, auto uw_tag) {
                            constexpr int SRC = decltype(src_tag)::value;
                            constexpr int NZ = decltype(nz_tag)::value;
                            constexpr bool AFLAT = decltype(aflat_tag)::value;
                            constexpr bool UW = decltype(uw_tag)::value;
                            if (UW) {
                                // the run's coefficients, amplitudes and noise, once for the wave (the pending sum reads the tile, not the window)
                                const uint32_t o_run = (uint32_t)__builtin_amdgcn_readfirstlane((int)o_chunk);
                                uw_fill(p, ea, r.seed_rot, o_run, run, p.tab.base + (ptrdiff_t)(cur.idx + (int32_t)o_chunk), wave_scratch + 64u, lane);
                                uw_chunks += run;
                            }
                            for (uint32_t i = 0; i < run; ++i) {
                                const uint32_t f0 = c16 + i * kChunk;            // frame inside the super-chunk
                                // the previous fast chunk's sums, stored unconditionally (into a scratch slot when none is
                                // pending) so that the adds sit in the chunk's basic block, in front of its first store
                                *pend_dst = tsum();
                                float *pvd = (PV && in_range) ? p.per_voice + pv_base + sc0 + f0 : nullptr;
                                const uint32_t oc = o_chunk + i * kChunk;
                                const float *tp = p.tab.base + (ptrdiff_t)(cur.idx + (int32_t)(oc & cur.mask));
                                chunk_fast<OSC, SRC, 0, (FM && SRC == 1), NZ, AFLAT, UW>(p, r, ea, em, fc, FM ? fc.k : k_const, oc, tp, sT, sSin, live,
                                                                              tile_lds, pvd, nullptr, nullptr, wave_scratch + 64u + i * kChunk);
                                __builtin_amdgcn_wave_barrier();
                                pend_dst = sw_row + f0;
                            }
                        };
                        // every offset of the run below 2^24 on every lane (349 s at 48 kHz; voices are never freed,
                        // synth.rs:196-199, so older ones exist) and a patch without noise (the default one): the cheaper
                        // offset and noise arithmetic of SMALL; on top of that, chunks that start on multiples of 16
                        // frames and seeds with a zero low nibble after the rotation (the reference's: 0): ALIGNED
                        const bool small = p.noise_level == 0.0f && offs_small;
                        const bool aligned = small && w_aligned && ((sc0 + c16) & 15u) == 0u;
                        // ... and every started voice's amplitude envelope in a zero-slope stage (no threshold falls inside
                        // the run, so the stage holds): the amplitude is one value per chunk (AFLAT)
                        const bool aflat = aligned && w_aflat;
                        using T = std::true_type; using F = std::false_type;
                        using N0 = std::integral_constant<int, 0>; using N1 = std::integral_constant<int, 1>; using N2 = std::integral_constant<int, 2>;
                        // ... and a cohort of 64 voices with a run long enough for the window's fill to pay: about one chunk's
                        // feed-forward work and 16 LDS stores per 64 chunks' worth of frames, against ~50 instructions and eight
                        // global loads saved per chunk — from S2R_UW_MIN_RUN chunks on
                        using UWon = std::integral_constant<bool, UWK && !FM>;
                        const bool uw = UWon::value && w_uni && run >= S2R_UW_MIN_RUN;
                        if (tab_ok) {
                            if (aflat) run_chunks(N1{}, N2{}, T{}, F{});
                            else if (aligned && uw) run_chunks(N1{}, N2{}, F{}, UWon{});
                            else if (aligned) run_chunks(N1{}, N2{}, F{}, F{});
                            else if (small) run_chunks(N1{}, N1{}, F{}, F{});
                            else run_chunks(N1{}, N0{}, F{}, F{});
                        } else if (flat) {
                            if (aflat) run_chunks(N0{}, N2{}, T{}, F{});
                            else if (aligned) run_chunks(N0{}, N2{}, F{}, F{});
                            else if (small) run_chunks(N0{}, N1{}, F{}, F{});
                            else run_chunks(N0{}, N0{}, F{}, F{});
                        } else if (!FM) {
                            if (aligned) run_chunks(N2{}, N2{}, F{}, F{});
                            else if (small) run_chunks(N2{}, N1{}, F{}, F{});
                            else run_chunks(N2{}, N0{}, F{}, F{});
                        }
                        c16 += (run - 1u) * kChunk;
                        dbg_t_run += S2R_DBG_NOW() - dbg_tr0;
                        continue;
                    }
                }
                flush_pending();
                ++dbg_general;
                for (uint32_t g = c16; g < c16 + kChunk; g += kP) {
                    // closed-form work of frames sc0+g .. +3 on this lane, then the recurrence for each of them
                    FrameCF4 cf; OscK4 kf;
                    closed_form_x4<OSC, FM>(p, r, ea, em, thr_min, fc, fcc, r.offset + sc0 + g, sT, cf, kf);
                    f4 out4;
#pragma unroll
                    for (int j = 0; j < kP; ++j) {
                        FrameCF c1; c1.amp = cf.amp[j]; c1.xc = cf.xc[j]; c1.nz = cf.nz[j];
                        OscK k1 = k_const;
                        if (FM) { k1.period = kf.period[j]; k1.inv_period = kf.inv_period[j];
                                  k1.a = kf.a[j]; k1.b = kf.b[j]; k1.c = kf.c[j]; }
                        const float o = recur_x16<OSC>(p, r, c1, k1, sSin);
                        out4[j] = live ? o : 0.0f;
                    }
                    if (PV) { if (in_range) {
                        float *dst = p.per_voice + pv_base + sc0 + g;
                        dst[0] = out4.x; dst[1] = out4.y; dst[2] = out4.z; dst[3] = out4.w; } }
                    float *trow = tile + (g & 15u) * kTileRow + lane;
                    trow[0 * kTileRow] = out4.x; trow[1 * kTileRow] = out4.y;
                    trow[2 * kTileRow] = out4.z; trow[3 * kTileRow] = out4.w;
                }
                reduce_chunk(c16, kChunk);
                reclassify();                                            // (a stage changed inside this chunk)
            }
            flush_pending();
            if (n_x16 < n_sc) {                                          // scalar tail (< 16 frames, last super-chunk)
                if (TEV) apply_events_at(sc0 + n_x16);
                for (uint32_t i = n_x16; i < n_sc; ++i) {
                    float out = frame_sisd<OSC>(p, r, r.offset + sc0 + i, sT, sSin);
                    out = live ? out : 0.0f;
                    if (PV) { if (in_range) p.per_voice[pv_base + sc0 + i] = out; }
                    tile[(i - n_x16) * kTileRow + lane] = out;
                }
                reduce_chunk(n_x16, n_sc - n_x16);
            }
        } else {
            for (uint32_t i = lane; i < GW * kSuper; i += 64u)
                sW[(buf * n_groups + wave * GW + i / kSuper) * kSuper + (i % kSuper)] = 0.0f;
            if (PV) { if (in_range) for (uint32_t i = 0; i < n_sc; ++i) p.per_voice[pv_base + sc0 + i] = 0.0f; }
        }
        stamp(2u + 2u * stamp_k);
        __syncthreads();
        combine_groups(p, ctl.done, sW + (size_t)buf * n_groups * kSuper, n_groups, kSuper, n_sc, sc0, bp + sc0, tid, blockDim.x, ctl.granules, ctl.granule_tag, ctl.fused || ctl.ov_render_counter != nullptr);
        buf ^= 1u;
        stamp(3u + 2u * stamp_k);
        ++stamp_k;
    }

    // ---- write back the recurrence state ----
    if (live) {
        const uint32_t o = r.offset;
        // (a voice restarted at frame f carries offset = -f here, so the sum is frames - f)
        p.v.offset[vi] = (!ev_dirty && o > 0xffffffffu - ctl.frames) ? 0xffffffffu : o + ctl.frames;   // synth.rs:197
        p.v.phase[vi] = r.phase;
        p.v.lpf_last[vi] = r.last;
        if (ev_dirty) {
            p.v.pitch[vi] = r.pitch;
            p.v.release[vi] = r.release_u;
            p.v.flags[vi] = S2R_VF_STARTED | (r.released ? S2R_VF_RELEASED : 0u);
            p.v.seed[vi] = seed_now;
            if (ev_restart) {                                    // st::Layer::default(), and the program it was started with
                p.v.fx1[vi] = 0.0f; p.v.fx2[vi] = 0.0f; p.v.fy1[vi] = 0.0f; p.v.fy2[vi] = 0.0f;
                p.v.osc_z[vi] = s2r_u2f(S2R_OSC_Z_NONE);
                p.v.program[vi] = program_now;
            }
        }
    }
    // (one atomic per wave and fill: the handle's count of window chunks, s2r_uniform_window_chunks)
    if (UWK && uw_chunks != 0u && lane == 0u) __hip_atomic_fetch_add(p.uw_count, uw_chunks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p.direct_out && ctl.granules == nullptr) signal_done(ctl.done, 1u);     // (a shard of one workgroup: its output is the fill's)
    if (ctl.ov_render_counter != nullptr) ov_signal(ctl.ov_render_counter);   // (two streams: the mix on the other one waits for every workgroup's row)
#if defined(S2R_STAMPS)
    if (p.stamps && lane == 0) p.stamps[(size_t)(vi >> 6) * 16u + 8u] = __builtin_amdgcn_s_memrealtime();
    if (ctl.fused) fused_tail(p, ctl, sW, &s_word, p.stamps ? p.stamps + (size_t)(vi >> 6) * 16u : nullptr);
#else
    if (ctl.fused) fused_tail(p, ctl, sW, &s_word);              // (one launch per fill: the last workgroups to get here add the rows up)
#endif
#if defined(S2R_STAMPS)
    if (p.stamps && lane == 0) { unsigned long long *d = p.stamps + (size_t)(vi >> 6) * 16u; d[11] = dbg_events; d[12] = (unsigned long long)dbg_dense | ((dbg_t_pick1 & 0x3fffffull) << 20) | ((dbg_t_casc & 0x3fffffull) << 42); d[13] = (dbg_t_top << 32) | (dbg_t_sel & 0xffffffffull); d[14] = dbg_runs;
        d[10] = ((unsigned long long)dbg_runchunks << 48) | ((dbg_t_dense & 0xffffffull) << 24) | (dbg_t_run & 0xffffffull); }
#endif
    stamp(15);
    tl_mark(p.timeline, p.tl_slot, 1);
}

template <int OSC, bool FM, int MODE, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT == 256 ? 2 : 1)) s2r_render_kernel(const S2rRenderArgs a) {
    const FillCtl ctl = fill_ctl_from_args(a);
    render_fill<OSC, FM, MODE, MAXT, MAXT == 256>(a, ctl);
}

// The resident kernel (S2rResident, s2r_device.h): wave 0 polls the command, the workgroup renders the fill it describes
// with the very code a launch per fill runs (MODE 0: events from the command, no timed events, no per-voice rows), until
// the host says EXIT or no command has come for idle_ticks.  Every wave reaches the exit: the poll loop is bounded in
// ticks and in polls, and its outcome is handed to the other waves through LDS and a barrier.
template <int OSC, bool FM>
__global__ void __launch_bounds__(256, 1) s2r_resident_kernel(const S2rRenderArgs a, const S2rResident rs) {
    __shared__ uint32_t s_cmd[S2R_RES_CMD_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint32_t last = rs.first_seq - 1u;
    for (;;) {
        if (tid < 64u) {
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            uint32_t polls = 0;
            for (;;) {
                uint32_t w = 0u;
                if (lane < S2R_RES_CMD_WORDS) w = __hip_atomic_load(rs.cmd + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                const uint32_t s_first = (uint32_t)__builtin_amdgcn_readlane((int)w, 0), s_last = (uint32_t)__builtin_amdgcn_readlane((int)w, 31);
                if (s_first == s_last && (int32_t)(s_first - last) > 0) {
                    if (lane < S2R_RES_CMD_WORDS) s_cmd[lane] = w;
                    break;
                }
                ++polls;
                if (__builtin_amdgcn_s_memrealtime() - t0 > (unsigned long long)rs.idle_ticks || polls >= rs.max_polls) {
                    if (lane == 0u) { s_cmd[0] = last + 1u; s_cmd[1] = S2R_RES_FLAG_EXIT << 16; s_cmd[2] = 0u; }
                    break;
                }
            }
        }
        __syncthreads();
        const uint32_t seq = s_cmd[0], w1 = s_cmd[1];
        if ((w1 >> 16) & S2R_RES_FLAG_EXIT) break;               // (uniform: every thread reads the same LDS word)
        last = seq;
        FillCtl ctl = fill_ctl_from_args(a);
        ctl.frames = w1 & 0xffffu;
        ctl.n_events = s_cmd[2] <= S2R_RES_MAX_EVENTS ? s_cmd[2] : 0u;
        ctl.ev = s_cmd + 4;
        ctl.done = S2rDone{rs.done_flag, s_cmd[3], rs.done_counter};
        ctl.granules = ctl.frames <= S2R_RES_GRANULE_FRAMES ? rs.granules : nullptr;
        ctl.granule_tag = s_cmd[3];
        if (ctl.frames != 0u && ctl.frames <= a.p.frames) render_fill<OSC, FM, 0, 256>(a, ctl);
        __syncthreads();                                         // (the command words and the staging are reused)
    }
    if (tid == 0u) __hip_atomic_store(rs.exited, rs.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The pool-resident kernel of the one-pole patches (pool_loop, s2r_kern_common.h): render_fill in MODE 2.
template <int OSC, bool FM>
__global__ void __launch_bounds__(256, 1) s2r_pool_kernel(const S2rRenderArgs a, const S2rPool pl) {
    pool_loop(a, pl, [&](const FillCtl &ctl) __attribute__((always_inline)) { render_fill<OSC, FM, 2, 256>(a, ctl); });
}

template <int OSC, bool FM, int MODE>
hipError_t launch_mode(const S2rRenderArgs &a0, uint32_t block_voices, hipStream_t stream) {
    static thread_local S2rRenderArgs a;                         // 4 KiB of kernel arguments, copied by the launch
    a = a0;
    S2rRenderParams &p = a.p;
    const uint32_t grid = (p.n_voices + block_voices - 1) / block_voices;
    const uint32_t n_waves = block_voices / 64, n_groups = n_waves * 4;
    // keeps the staging (group sums + two transpose tiles per wave) under the 160 KiB of LDS
    p.super_frames = s2r_pick_super_frames(n_groups, grid, p.frames);
    size_t lds = sizeof(float) * ((size_t)s2r_sw_buffers(p.frames, p.super_frames) * n_groups * p.super_frames + (size_t)n_waves * (kChunk * kTileRow + 64));
    // The uniform window: S2R_UW_PLANES x S2R_UW_FRAMES floats per wave behind the rest, only where the workgroup has its compute
    // unit to itself and the fill is one super-chunk, and only if it fits the 160 KiB beside the group sums, the tiles and
    // the kernel's static tables (exp2 and sine: at most 8 KiB + 8 * S2R_EXP2F_N + a word).  Otherwise none: the kernel
    // then runs exactly the variants it ran before there was a window.
    p.uw_frames = 0u;
    if (p.uw_count != nullptr && !FM && block_voices <= 256 && p.super_frames == kSuperWhole && s2r_sw_buffers(p.frames, p.super_frames) == 1u) {
        const size_t with_uw = lds + sizeof(float) * (size_t)n_waves * S2R_UW_PLANES * S2R_UW_FRAMES;
        if (with_uw + 8192u + 8u * S2R_EXP2F_N + 64u <= 160u * 1024u) { lds = with_uw; p.uw_frames = S2R_UW_FRAMES; }
    }
    if (lds > 65536) {                                           // (HIP wants to be told about more than 64 KiB of dynamic LDS)
        static thread_local size_t told256 = 0, told1024 = 0;
        if (block_voices <= 256 && told256 < lds) {
            const hipError_t e = hipFuncSetAttribute((const void *)s2r_render_kernel<OSC, FM, MODE, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            told256 = lds;
        } else if (block_voices > 256 && told1024 < lds) {
            const hipError_t e = hipFuncSetAttribute((const void *)s2r_render_kernel<OSC, FM, MODE, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            told1024 = lds;
        }
    }
    // the launch bound is the register budget: 256-thread workgroups (one wave per SIMD) may use
    // the whole file, which the 4-frame vector code wants; bigger workgroups get what is left
    if (block_voices <= 256) hipLaunchKernelGGL((s2r_render_kernel<OSC, FM, MODE, 256>), dim3(grid), dim3(block_voices), lds, stream, a);
    else hipLaunchKernelGGL((s2r_render_kernel<OSC, FM, MODE, 1024>), dim3(grid), dim3(block_voices), lds, stream, a);
    return hipGetLastError();
}

template <int OSC, bool FM>
hipError_t launch_resident(const S2rRenderArgs &a0, const S2rResident &rs, uint32_t block_voices, hipStream_t stream) {
    static thread_local S2rRenderArgs a;
    a = a0;
    S2rRenderParams &p = a.p;
    if (block_voices > 256u || p.n_voices > block_voices || p.direct_out == nullptr || p.per_voice != nullptr || p.tev != nullptr) return hipErrorInvalidValue;
    const uint32_t n_waves = block_voices / 64, n_groups = n_waves * 4;
    p.super_frames = s2r_pick_super_frames(n_groups, 1u, p.frames);
    p.uw_frames = 0u;                                            // (no uniform window in the resident form)
    const size_t lds = sizeof(float) * ((size_t)s2r_sw_buffers(p.frames, p.super_frames) * n_groups * p.super_frames + (size_t)n_waves * (kChunk * kTileRow + 64));
    if (lds > 65536) {
        static thread_local size_t told = 0;
        if (told < lds) {
            const hipError_t e = hipFuncSetAttribute((const void *)s2r_resident_kernel<OSC, FM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            told = lds;
        }
    }
    hipLaunchKernelGGL((s2r_resident_kernel<OSC, FM>), dim3(1), dim3(block_voices), lds, stream, a, rs);
    return hipGetLastError();
}

template <int OSC, bool FM>
hipError_t launch_pool(const S2rRenderArgs &a0, const S2rPool &pl, uint32_t block_voices, hipStream_t stream) {
    static thread_local S2rRenderArgs a;
    a = a0;
    S2rRenderParams &p = a.p;
    if (block_voices > 256u || p.per_voice != nullptr || p.direct_out != nullptr) return hipErrorInvalidValue;
    const uint32_t grid = (p.n_voices + block_voices - 1) / block_voices;
    const uint32_t n_waves = block_voices / 64, n_groups = n_waves * 4;
    p.super_frames = s2r_pick_super_frames(n_groups, grid, p.frames);
    p.uw_frames = 0u;                                            // (no uniform window in the pool-resident form)
    const size_t lds = sizeof(float) * ((size_t)s2r_sw_buffers(p.frames, p.super_frames) * n_groups * p.super_frames + (size_t)n_waves * (kChunk * kTileRow + 64));
    if (lds > 65536) {
        static thread_local size_t told = 0;
        if (told < lds) {
            const hipError_t e = hipFuncSetAttribute((const void *)s2r_pool_kernel<OSC, FM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            told = lds;
        }
    }
    hipLaunchKernelGGL((s2r_pool_kernel<OSC, FM>), dim3(grid), dim3(block_voices), lds, stream, a, pl);
    return hipGetLastError();
}

}  // namespace

#define S2R_CAT2(a, b) a##b
#define S2R_CAT(a, b) S2R_CAT2(a, b)
hipError_t S2R_CAT(s2r_launch_onepole_resident_osc, S2R_TU_OSC)(const S2rRenderArgs &a, const S2rResident &rs, uint32_t block_voices, hipStream_t stream) {
    return a.p.amt_osc != 0.0f ? launch_resident<S2R_TU_OSC, true>(a, rs, block_voices, stream) : launch_resident<S2R_TU_OSC, false>(a, rs, block_voices, stream);
}

hipError_t S2R_CAT(s2r_launch_onepole_pool_osc, S2R_TU_OSC)(const S2rRenderArgs &a, const S2rPool &pl, uint32_t block_voices, hipStream_t stream) {
    return a.p.amt_osc != 0.0f ? launch_pool<S2R_TU_OSC, true>(a, pl, block_voices, stream) : launch_pool<S2R_TU_OSC, false>(a, pl, block_voices, stream);
}

// one exported launcher per translation unit / oscillator kind (s2r_aux.hip dispatches)
hipError_t S2R_CAT(s2r_launch_onepole_osc, S2R_TU_OSC)(const S2rRenderArgs &a, uint32_t block_voices, hipStream_t stream) {
    const S2rRenderParams &p = a.p;
    // pow(2, mod * amount) == 1 exactly iff amount is +-0 (mod is always finite and >= 0)
    const bool fm = p.amt_osc != 0.0f;
    if (p.per_voice != nullptr && p.tev != nullptr) return hipErrorInvalidValue;   // the host refuses this combination
    const int mode = p.per_voice != nullptr ? 1 : (p.tev != nullptr ? 2 : 0);
    switch (mode) {
    case 1: return fm ? launch_mode<S2R_TU_OSC, true, 1>(a, block_voices, stream) : launch_mode<S2R_TU_OSC, false, 1>(a, block_voices, stream);
    case 2: return fm ? launch_mode<S2R_TU_OSC, true, 2>(a, block_voices, stream) : launch_mode<S2R_TU_OSC, false, 2>(a, block_voices, stream);
    default: return fm ? launch_mode<S2R_TU_OSC, true, 0>(a, block_voices, stream) : launch_mode<S2R_TU_OSC, false, 0>(a, block_voices, stream);
    }
}
