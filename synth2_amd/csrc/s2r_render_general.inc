// s2r_render_general.inc — everything the tuned one-pole kernel (s2r_render_onepole.inc) does not cover.
// Included by s2r_render_general_<osc>.hip with S2R_TU_OSC defined (0..3: one patch whose filter is one of
// dsp_filters.rs / the SVF; 4 = S2R_OSC_ANY: a bank of patches, oscillator and filter kind per lane).
#include "s2r_kern_common.h"

namespace {

// ---------------------------------------------------------------------------------------
// general render kernel: everything the tuned one-pole kernel above does not cover.
//   BANK = false: one patch (kernel arguments), filter = one of dsp_filters.rs (lpf.kind != onepole);
//   BANK = true : a bank of patches, every voice renders with bank[its program] — oscillator kind,
//                 filter kind and every level are per-lane values (OSC == S2R_OSC_ANY).
// Same voice-per-lane layout, state arrays, mixdown staging and timed events as s2r_render_kernel
// (L = 1), but the plain frame loop: per frame the envelope cascade, the oscillator and the filter
// step; the oscillator constants and the filter coefficients (pow2, exp or sin/cos/tan, the
// divisions) are recomputed only when some lane's mod-envelope value differs from the previous
// frame's (wave-uniform test).  DESIGN.md 4.6, 4.7.
// ---------------------------------------------------------------------------------------
struct LanePatch {           // field names as in S2rRenderParams: frame_sisd & co. take either
    int32_t osc_kind;
    float osc_gain, noise_level, lpf_freq, amt_osc, amt_lpf;
    int32_t lpf_kind;
    float lpf_damping;
    S2rEnv amp, mod;
    float sr, rcp_sr;
    S2rTabRef tab;           // this patch's coefficient tables (base == nullptr: none); base: the bank's table buffer
    uint32_t tab_off;        // ... where this patch's planes start in it (floats)
};

__device__ __forceinline__ LanePatch lane_patch_from_bank(const S2rBankEntry *bank, uint32_t n, uint32_t program, float sr,
                                                          const float *tab_base) {
    const S2rBankEntry e = bank[program < n ? program : 0u];     // an index past the bank renders with patch 0
    LanePatch lp;
    lp.osc_kind = e.osc_kind; lp.osc_gain = e.osc_gain; lp.noise_level = e.noise_level; lp.lpf_freq = e.lpf_freq;
    lp.amt_osc = e.amt_osc; lp.amt_lpf = e.amt_lpf; lp.lpf_kind = e.lpf_kind; lp.lpf_damping = e.lpf_shape;
    lp.amp = e.amp; lp.mod = e.mod; lp.sr = sr; lp.rcp_sr = 0.0f;
    lp.tab.base = (e.tab_valid && tab_base) ? tab_base : nullptr;
    lp.tab_off = e.tab_off;
    lp.tab.plane = e.tab_plane; lp.tab.ad = e.tab_ad; lp.tab.rc = e.tab_rc; lp.tab.rc_t0 = e.tab_rc_t0; lp.tab.ru = e.tab_ru;
    lp.tab.sus = e.tab_sus; lp.tab.end = e.tab_end; lp.tab.dead = e.tab_dead; lp.tab.fm_plane = 3u;
    return lp;
}

// ---------------------------------------------------------------------------------------
// The patch bank's branch-free chunk: 16 frames of 64 voices that may each render with another patch.
//   What differs between the lanes is data, not control flow, wherever that is cheap:
//   * square / saw / triangle are one expression with per-lane constants (oscillators.rs:60-183):
//         x < half ? fma(A1, x, 1) : fma(A2, arg2, B2)      saw: A1 = A2 = -2/period, arg2 = x, B2 = 1
//                                                            square: A1 = A2 = +0 (fma(+0, x, +-1) = +-1), B2 = -1
//                                                            triangle: A1 = -4/period, A2 = 4/period, arg2 = x - half, B2 = -1
//     (the selects are bit-field inserts under a sign mask, as in chunk_fast); the sine lookup runs for every lane when
//     some lane of the wave needs it (SINE) and is picked by mask.
//   * the filters form four families — the one-pole (filters.rs:20-33); LP1/HP1 (dsp_filters.rs:25-80: x +- x1);
//     LP2/HP2/BP2 (:99-230: x +- 2 x1 + x2 or x - x2); the SVF's three taps — whose 16-frame recurrences run one after
//     the other under their lanes' EXEC mask, AFTER the feed-forward work of the whole chunk: four branches per chunk,
//     not per frame.  Inside a family the kinds differ by sign masks and selects.
//   Coefficients come from each lane's patch tables (`tab`: the lane's entry for the chunk's first frame; planes c0,
//   c1, c2, pow(2, mod * amt_osc)); preconditions as chunk_fast's SMALL: no envelope threshold inside the chunk,
//   0 <= phase < 1, offsets below 2^24.
// ---------------------------------------------------------------------------------------
struct BankLane {
    float c1, c2, b2;              // A1 = c1 / period, A2 = c2 / period, B2
    uint32_t m_arg, m_sine;        // all ones: arg2 = x - half (triangle); the lane's oscillator is the sine table
    uint32_t m_dpw_saw, m_dpw_sq;  // DPW shapes (a wave of DPW voices only): F = s^2 / 2, |s|, else s (|s| - 1)
    uint32_t fam;                  // 0 one-pole, 1 LP1/HP1, 2 LP2/HP2/BP2, 3 SVF
    uint32_t s1;                   // HP1: sign bit (x - x1 == x + (-x1))
    float c2f;                     // LP2 +2, HP2 -2
    uint32_t m_bp2, s2;            // BP2: xs = x - x2
    uint32_t m_svf_lp, m_svf_bp;
    float svf_k;                   // 1 / q
};

__device__ __forceinline__ BankLane make_bank_lane(const LanePatch &lp) {
    BankLane b;
    const int o = lp.osc_kind, f = lp.lpf_kind;
    b.c1 = o == S2R_OSC_SAW ? -2.0f : o == S2R_OSC_TRIANGLE ? -4.0f : 0.0f;
    b.c2 = o == S2R_OSC_SAW ? -2.0f : o == S2R_OSC_TRIANGLE ? 4.0f : 0.0f;
    b.b2 = o == S2R_OSC_SAW ? 1.0f : -1.0f;
    b.m_arg = o == S2R_OSC_TRIANGLE ? 0xffffffffu : 0u;
    b.m_sine = o == S2R_OSC_SINE ? 0xffffffffu : 0u;
    b.m_dpw_saw = o == S2R_OSC_DPW_SAW ? 0xffffffffu : 0u;
    b.m_dpw_sq = o == S2R_OSC_DPW_SQUARE ? 0xffffffffu : 0u;
    b.fam = f == S2R_FILT_ONEPOLE ? 0u : f <= S2R_FILT_HP1 ? 1u : f <= S2R_FILT_BP2 ? 2u : 3u;
    b.s1 = f == S2R_FILT_HP1 ? 0x80000000u : 0u;
    b.c2f = f == S2R_FILT_HP2 ? -2.0f : 2.0f;
    b.m_bp2 = f == S2R_FILT_BP2 ? 0xffffffffu : 0u;
    b.s2 = f == S2R_FILT_BP2 ? 0x80000000u : 0u;
    b.m_svf_lp = f == S2R_FILT_SVF_LP ? 0xffffffffu : 0u;
    b.m_svf_bp = f == S2R_FILT_SVF_BP ? 0xffffffffu : 0u;
    b.svf_k = f >= S2R_FILT_SVF_LP ? 1.0f / lp.lpf_damping : 0.0f;
    return b;
}

// m ? a : b bit by bit: v_bfi_b32, spelled out (from (a & m) | (b & ~m) the compiler makes a compare and a select where
// m is a sign mask, and three instructions where ~m is loop-invariant)
__device__ __forceinline__ float sel_bits(uint32_t m, float a, float b) {
    float d;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(d) : "v"(m), "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ f4 sel_bits4(u4 m, f4 a, f4 b) {
    return (f4){sel_bits(m.x, a.x, b.x), sel_bits(m.y, a.y, b.y), sel_bits(m.z, a.z, b.z), sel_bits(m.w, a.w, b.w)};
}

//   FAMS: bit f set = some started voice of the wave has a filter of family f.
//   DPW: every started voice of the wave has a DPW oscillator (4.10): F's first difference, the differentiator's memory
//   in `osc_z` (a NaN — no DPW frame rendered since the note-on — resolves to the chunk's first F).
template <bool SINE, bool POLY, bool FMV, int FAMS, bool DPW = false>
__device__ __forceinline__ float chunk_bank(const LanePatch &lp, const BankLane &bl, VoiceRegs &r, Filt2 &f2, float osc_z, const EnvRun &ea,
                                           float period0, uint32_t o_chunk, const float *tab, uint32_t plane,
                                           const float *sSin, bool live, uint32_t tile_m0, float *pv_dst,
                                           float *pend_dst, const f4 *tsrc4) {
    constexpr bool F0 = (FAMS & 1) != 0, F1 = (FAMS & 2) != 0, F2 = (FAMS & 4) != 0, F3 = (FAMS & 8) != 0;
    constexpr bool C12 = (FAMS & ~1) != 0;                       // planes c1, c2 are needed
    constexpr bool MIXED = (FAMS & (FAMS - 1)) != 0;             // more than one family: per-lane selects
    // the previous branch-free chunk's column sums: its 16 values are read here, at the head of this chunk's basic block
    // (not kept in registers from behind that chunk's stores: sixteen registers fewer live across the loops)
    float tv[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) { const f4 t4 = tsrc4[q]; tv[4 * q] = t4.x; tv[4 * q + 1] = t4.y; tv[4 * q + 2] = t4.z; tv[4 * q + 3] = t4.w; }
    f4 xq[4], bq[4], gq[4], pq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        xq[q] = load_f4u(tab + 4 * q);
        if (FMV) pq[q] = load_f4u(tab + 3u * plane + 4 * q);
        if (C12) { bq[q] = load_f4u(tab + plane + 4 * q); gq[q] = load_f4u(tab + 2u * plane + 4 * q); }
    }
    const float inv_period0 = 1.0f / period0;                    // oscillators.rs:378 (constants of the run when !FMV)
    const double rcp_period = (SINE && !FMV) ? s2r_rcp_f64(period0) : 0.0;
    const float ea_slope = live ? ea.s0 : 0.0f, ea_base = live ? ea.s1 : 0.0f, ea_y0 = live ? ea.s2 : 0.0f;
    const uint32_t o_lo = o_chunk & 0xffffu;
    uint32_t o01 = pk_add_u16(o_lo | (o_lo << 16), 0x00010000u), o23 = pk_add_u16(o01, 0x00020002u);
    const uint32_t seed_pair = (r.seed_rot & 0xffffu) | (r.seed_rot << 16);
    f4 t = splat((float)o_chunk) + (f4){0.0f, 1.0f, 2.0f, 3.0f};    // exact below 2^24, as are the + 4 steps
    const uint32_t livemask = live ? 0xffffffffu : 0u;
    const uint32_t fam = bl.fam;
    // (a lane without a voice counts as a one-pole lane where the wave has one: x = 1 from the "no voice" entries of the
    // tables it reads and last = 0 make y0 = +0 without a mask, as in chunk_fast)
    const uint32_t m_f0 = (fam == 0u || !live) ? 0xffffffffu : 0u, m_f1 = fam == 1u ? 0xffffffffu : 0u, m_f2 = fam == 2u ? 0xffffffffu : 0u;
    // filter state, one copy per family (every lane steps every family of the wave; the lane's own is kept at the end).
    // A lane without a voice has no history: x = 1 from its tables' "no voice" entries and last = 0 make its one-pole
    // output +0 (chunk_fast); the other families' outputs are masked
    float last = live ? r.last : 0.0f;
    float px1 = f2.x1, px2 = f2.x2;                              // LP1/HP1 and the biquads: the previous two inputs
    float ay1 = f2.y1;                                           // LP1/HP1
    float by1 = f2.y1, by2 = f2.y2;                              // biquads
    float i1 = f2.x1, i2 = f2.x2;                                // SVF integrators
    float phc = r.phase;
    float zdpw = DPW ? osc_z : 0.0f;
    f4 outs[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        // process.rs:347-356: the noise plus the patch's level (ADD, x16 path)
        const f4 nz = hash_noise4_low16(seed_pair, o01, o23) + splat(lp.noise_level);
        const f4 amp = splat(ea_slope) * pk_add4(t, splat(-ea_base)) + splat(ea_y0);
        t = t + splat(4.0f);
        o01 = pk_add_u16(o01, 0x00040004u); o23 = pk_add_u16(o23, 0x00040004u);
        f4 period = splat(period0), inv_period = splat(inv_period0);
        if (FMV) {
            const f4 f_osc = pq[q] * splat(r.pitch);             // pow(2, mod * amount) * freq   process.rs:146-147,231-250
            period = splat(lp.sr) / f_osc;                       // units.rs:32-42
            inv_period = splat(1.0f) / period;                   // oscillators.rs:378
        }
        f4 ph;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ph[j] = phc;
            phc = __builtin_amdgcn_fractf(phc + inv_period[j]);  // oscillators.rs:377-381 (see chunk_fast)
        }
        const f4 x = period * ph;                                // == off % period (chunk_fast)
        f4 osc = splat(0.0f);
        SineQuad sq;
        if (SINE) sq = sine_quad_issue<FMV>(x, period, rcp_period, sSin);    // the four LDS reads, collected behind the next block
        if (POLY) {
            const f4 half = period * splat(0.5f);
            const f4 d = x - half;
            const u4 lt = (u4)((i4)(u4)d >> 31);                 // all ones where x < half
            const f4 arg2 = sel_bits4((u4)bl.m_arg, d, x);
            const f4 first = vfma(splat(bl.c1) * inv_period, x, splat(1.0f));
            const f4 second = vfma(splat(bl.c2) * inv_period, arg2, splat(bl.b2));
            osc = sel_bits4(lt, first, second);
        }
        if (SINE) {
            const f4 sn = sine_quad_finish(sq);
            osc = POLY ? sel_bits4((u4)bl.m_sine, sn, osc) : sn;
        }
        if (DPW) {
            static_assert(!(DPW && (SINE || POLY)), "a DPW wave has DPW voices only");
            // dpw_value on four frames: s = (-2 / period) x + 1, F by shape, y = (-period / 2) (F - z), z = F
            const f4 sw = vfma(splat(-2.0f) * inv_period, x, splat(1.0f));
            const f4 aw = (f4)((u4)sw & 0x7fffffffu);
            const f4 F = sel_bits4((u4)bl.m_dpw_saw, splat(0.5f) * (sw * sw), sel_bits4((u4)bl.m_dpw_sq, aw, sw * (aw - splat(1.0f))));
            if (q == 0) zdpw = zdpw != zdpw ? F.x : zdpw;        // (the voice's first DPW frame differences against its own F)
            const f4 zsh = {zdpw, F.x, F.y, F.z};
            zdpw = F.w;
            osc = (splat(-0.5f) * period) * (F - zsh);
        }
        const f4 sv = pk_add4(osc + splat(lp.osc_gain), nz);     // process.rs:342-345 (ADD), :358
        f4 y;
        const f4 a0 = splat(1.0f) - xq[q];                       // filters.rs:23
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = sv[j];
            float y0 = 0.0f, y1 = 0.0f, y2 = 0.0f, y3 = 0.0f;
            if (F0) { last = __builtin_fmaf(a0[j], s, xq[q][j] * last); y0 = last; }           // filters.rs:23-33
            if (F1) {                                            // dsp_filters.rs:25-45, :60-80: x +- x1
                const float xs = s + s2r_u2f(s2r_f2u(px1) ^ bl.s1);
                ay1 = xq[q][j] * xs + gq[q][j] * ay1;
                y1 = ay1;
            }
            if (F2) {                                            // dsp_filters.rs:99-130, :149-180, :199-230
                const float lead = sel_bits(bl.m_bp2, s, __builtin_fmaf(bl.c2f, px1, s));      // x +- 2 x1 (2 x1 is exact), or x
                const float xs = lead + s2r_u2f(s2r_f2u(px2) ^ bl.s2);
                y2 = 2.0f * ((xq[q][j] * xs + gq[q][j] * by1) - bq[q][j] * by2);
                by2 = by1; by1 = y2;
            }
            if (F3) {                                            // the SVF (dsp_filter_apply)
                const float v3 = s - i2;
                const float v1 = xq[q][j] * i1 + bq[q][j] * v3;
                const float v2 = (i2 + bq[q][j] * i1) + gq[q][j] * v3;
                i1 = 2.0f * v1 - i1;
                i2 = 2.0f * v2 - i2;
                const float hp = (s - bl.svf_k * v1) - v2;
                y3 = sel_bits(bl.m_svf_lp, v2, sel_bits(bl.m_svf_bp, v1, hp));
            }
            if (F1 || F2) { px2 = px1; px1 = s; }
            // the lane's own family
            float yy = F3 ? y3 : F2 ? y2 : F1 ? y1 : y0;
            if (F3 && F2) yy = sel_bits(m_f2, y2, yy);
            if ((F3 || F2) && F1) yy = sel_bits(m_f1, y1, yy);
            if ((F3 || F2 || F1) && F0) yy = sel_bits(m_f0, y0, yy);
            y[j] = yy;
        }
        f4 out = y * amp;                                        // process.rs:373-376
        if (!F0) out = (f4)((u4)out & livemask);                 // (a lane without a voice runs the recursive filters on nothing)
        if (q == 0) {
            // ... and go out in front of this chunk's first store; the serial adds have the first quad's arithmetic to hide in
            float acc = tv[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) acc += tv[i];
            *pend_dst = acc;
            tile_set_base(tile_m0);
        }
        tile_store4(q, out);
        outs[q] = out;
    }
    if (pv_dst) {                                                // per-voice rows: one branch behind the chunk's basic block
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<f4u *>(pv_dst + 4 * q) = outs[q];
    }
    r.phase = phc;
    // the lane's own filter's state back (one family: no select)
    if (!MIXED) {
        if (F0) r.last = last;
        if (F1) { f2.x1 = px1; f2.y1 = ay1; }
        if (F2) { f2.x1 = px1; f2.x2 = px2; f2.y1 = by1; f2.y2 = by2; }
        if (F3) { f2.x1 = i1; f2.x2 = i2; }
    } else {
        const bool is0 = fam == 0u || !live, is1 = fam == 1u, is2 = fam == 2u, is3 = fam == 3u;
        if (F0) r.last = is0 ? last : r.last;
        if (F1) { f2.x1 = is1 ? px1 : f2.x1; f2.y1 = is1 ? ay1 : f2.y1; }
        if (F2) { f2.x1 = is2 ? px1 : f2.x1; f2.x2 = is2 ? px2 : f2.x2; f2.y1 = is2 ? by1 : f2.y1; f2.y2 = is2 ? by2 : f2.y2; }
        if (F3) { f2.x1 = is3 ? i1 : f2.x1; f2.x2 = is3 ? i2 : f2.x2; }
    }
    return (DPW && live) ? zdpw : osc_z;         // the differentiator's memory after the chunk
}

// One fill of the workgroup's voices (the kernel's body as a function: a launch is a fill, or — the pool-resident kernel — a
// posted command is; `ctl`: what changes from fill to fill, s2r_kern_common.h)
template <int OSC, bool BANK, int MAXT>
__device__ __forceinline__ void general_fill(const S2rRenderArgs &a, const FillCtl &ctl) {
    const S2rRenderParams &p = a.p;
    const uint32_t kSuper = p.super_frames;
    const bool PV = p.per_voice != nullptr, TEV = ctl.tev != nullptr;        // wave-uniform
    __shared__ uint64_t sT[S2R_EXP2F_N];
    __shared__ __attribute__((aligned(8))) float sSin[(OSC == S2R_OSC_SINE || OSC == S2R_OSC_ANY) ? 2048 : 2];
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    __shared__ uint32_t s_word;                                  // (one launch per fill: the workgroup's arrival ticket)

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6, n_waves = blockDim.x >> 6;
    constexpr uint32_t GW = 4;
    const uint32_t n_groups = n_waves * GW;
    float *const sW = s_dyn;                                     // [2][n_groups][kSuper]
    float *const tile = s_dyn + s2r_sw_buffers(p.frames, kSuper) * n_groups * kSuper + wave * (kChunk * kTileRow + 64u);
    float *const wave_scratch = tile + kChunk * kTileRow;        // 64 floats: where a column sum goes when none is pending
    const uint32_t tile_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)tile);   // its LDS byte address
    const uint32_t vi = blockIdx.x * blockDim.x + tid;

    if (tid < S2R_EXP2F_N) sT[tid] = c_exp2f_table[tid];
    if (OSC == S2R_OSC_SINE || OSC == S2R_OSC_ANY)
        for (uint32_t i = tid; i < 1024u; i += blockDim.x) { sSin[2u * i] = p.sin_table[(i + 1023u) & 1023u]; sSin[2u * i + 1u] = p.sin_table[i]; }

    apply_arg_events(p, ctl.n_events, ctl.ev, vi, lane);

    // two streams (S2rOverlapWords): the fill's chain heads and event copy come from a kernel on the other stream
    // (one launch per fill: the workgroup copies ITS slice of the fill's records and publishes its own voices' chain heads)
    const bool ovh = TEV && (ctl.fused || ctl.ov_heads_counter != nullptr);
    if (TEV && ctl.fused) fused_heads(ctl);
    else if (ovh) {
        __shared__ uint32_t s_ok;
        if (tid == 0) { const bool ok = ov_wait(ctl.ov_heads_counter, ctl.ov_heads_target); if (!ok) ov_raise(ctl.fail, 1u); s_ok = ok ? 1u : 0u; }
        __syncthreads();
        if (s_ok == 0u) {
            // (the chain heads never came: the fill is not rendered, the voices and their chains stay as they are, the row is
            // silence — s2r_render_onepole.inc)
            float *row = ctl.partials + (size_t)blockIdx.x * p.frames_stride;
            for (uint32_t f = 4u * tid; f < p.frames_stride && f < ((ctl.frames + 3u) & ~3u); f += 4u * blockDim.x) ov_store4(row + f, (f4){0.0f, 0.0f, 0.0f, 0.0f});
            if (ctl.ov_render_counter != nullptr) ov_signal(ctl.ov_render_counter);
            return;
        }
    }
    const bool in_range = vi < p.n_voices;
    const uint32_t flags = in_range ? p.v.flags[vi] : 0u;
    bool live = (flags & S2R_VF_STARTED) != 0u;                  // synth.rs:178
    LanePatch lp;
    uint32_t program = 0u;
    if constexpr (BANK) {
        program = live ? p.v.program[vi] : 0u;
        lp = lane_patch_from_bank(p.bank, p.bank_size, program, p.sr, p.no_flat_shortcut ? nullptr : p.tab.base);
    } else {
        lp.osc_kind = p.osc_kind; lp.osc_gain = p.osc_gain; lp.noise_level = p.noise_level; lp.lpf_freq = p.lpf_freq;
        lp.amt_osc = p.amt_osc; lp.amt_lpf = p.amt_lpf; lp.lpf_kind = p.lpf_kind; lp.lpf_damping = p.lpf_damping;
        lp.amp = p.amp; lp.mod = p.mod; lp.sr = p.sr; lp.rcp_sr = p.rcp_sr;
        lp.tab = p.tab; lp.tab_off = 0u;
    }
    VoiceRegs r;
    r.pitch = live ? p.v.pitch[vi] : 440.0f;
    r.offset = live ? p.v.offset[vi] : 0u;
    r.release_u = live ? p.v.release[vi] : 0u;
    r.released = live && (flags & S2R_VF_RELEASED) != 0u;
    r.phase = live ? p.v.phase[vi] : 0.0f;
    r.last = live ? p.v.lpf_last[vi] : 0.0f;
    Filt2 f2;
    f2.x1 = live ? p.v.fx1[vi] : 0.0f; f2.x2 = live ? p.v.fx2[vi] : 0.0f;
    f2.y1 = live ? p.v.fy1[vi] : 0.0f; f2.y2 = live ? p.v.fy2[vi] : 0.0f;
    const uint32_t seed = live ? p.v.seed[vi] : 0u;
    r.seed_rot = (seed << 5) | (seed >> 27);
    // DPW oscillators (patch banks' kernel only): the differentiator's memory (NaN: the voice has not rendered a DPW
    // frame since its note-on)
    float osc_z = 0.0f;
    if (OSC == S2R_OSC_ANY) osc_z = live ? p.v.osc_z[vi] : 0.0f;
    auto set_release_thresholds = [&]() {
        const float rf = r.released ? (float)r.release_u : 4294967296.0f;    // u32::MAX as f32
        r.ro_a = __builtin_fmaxf(rf, BANK ? lp.amp.sus_off : p.amp.sus_off); r.end_a = r.ro_a + (BANK ? lp.amp.R : p.amp.R);
        r.ro_m = __builtin_fmaxf(rf, BANK ? lp.mod.sus_off : p.mod.sus_off); r.end_m = r.ro_m + (BANK ? lp.mod.R : p.mod.R);
    };
    int32_t ev_idx = -1;
    uint32_t ev_frame = 0xffffffffu;
    bool ev_dirty = false, ev_restart = false;
    uint32_t seed_now = seed;
    // A release that is the voice's next event is booked at once, whatever its frame (s2r_render_onepole.inc: the x16
    // ADSR is a pure function of the offset and the release offset, and a release that lies ahead changes nothing
    // until the offset reaches it) — where f32 tells every earlier offset from the release offset, i.e. up to 2^24.
    auto take_releases = [&]() {
        while (ev_idx >= 0) {
            const S2rTimedEvent e = tev_load(ctl.tev, ovh, ev_idx);
            const uint32_t rel = r.offset + e.frame;
            const bool base_ok = r.offset <= (1u << 24) || r.offset >= 0u - ctl.frames;
            if ((e.flags & S2R_EV_RESTART) || !(base_ok && rel <= (1u << 24))) { ev_frame = e.frame; return; }
            if ((e.flags & S2R_EV_RELEASE) && live && !r.released) { r.released = true; r.release_u = rel; }
            ev_dirty = true;
            ev_idx = e.next;
        }
        ev_frame = 0xffffffffu;
    };
    if (TEV && in_range) {
        ev_idx = ovh ? ov_load(ctl.heads + vi) : ctl.heads[vi];
        if (ev_idx >= 0) { if (ovh) ov_store(ctl.heads + vi, (int32_t)-1); else ctl.heads[vi] = -1; take_releases(); }
    }
    set_release_thresholds();

    // envelope stage registers: the cascade for the fill's first frame, so that the first chunk can already take the
    // branch-free path (as in s2r_render_kernel)
    EnvRun ea = env_stage_at(lp.amp, r.ro_a, r.end_a, (float)r.offset), em = env_stage_at(lp.mod, r.ro_m, r.end_m, (float)r.offset);
    float thr_min = __builtin_fminf(ea.s3, em.s3);
    uint32_t mod_key = 0xffffffffu;          // bits of the mod value `k`, `xc`, `fc` were computed for (a NaN: never equal)
    OscK k = make_osck_any<OSC>(lp.osc_kind, lp.sr / r.pitch);
    float xc = 0.0f;                         // one-pole coefficient exp(-2 pi f / sr), filters.rs:21
    FiltCoef fc; fc.alpha = fc.beta = fc.gamma = 0.0f;
    fc.k = lp.lpf_kind >= S2R_FILT_SVF_LP ? 1.0f / lp.lpf_damping : 0.0f;   // the SVF's k = 1 / q does not depend on the cutoff
    __syncthreads();

    const bool wave_live = __ballot(live || ev_idx >= 0) != 0ull;
    const uint32_t x16_frames = ctl.frames & ~(uint32_t)(kChunk - 1);
    const size_t pv_base = (size_t)vi * ctl.frames;
    float *bp = ctl.partials + (size_t)blockIdx.x * p.frames_stride;
    uint32_t buf = 0;
    // the patch's coefficient tables (single patch, 256-thread workgroups): alpha / beta / gamma per frame, and under
    // oscillator FM pow(2, mod * amount) (DESIGN.md 4.4)
    constexpr bool kFast = !BANK && MAXT == 256;
    const bool fmv = p.amt_osc != 0.0f;                          // kernel argument: uniform
    const bool have_tab = kFast && p.tab.base != nullptr && !p.no_flat_shortcut;
    // the patch bank's chunk (chunk_bank): what the wave's started voices need, looked at again after every restart
    constexpr bool kBank = BANK && MAXT == 256;
    // The two values a flat mod envelope can take — the sustain level and +0 (EnvRun: a zero-slope stage's value is its y0) — give
    // two sets of filter coefficients, and they sit in the tables' sustain and end regions at wave-uniform addresses: read here
    // once instead of pow2 + sin / cos / tan per lane at every stage change of any lane of the wave (as s2r_render_kernel's
    // FlatConsts).  Without oscillator FM only: the period then does not depend on the envelope.
    const bool flat_tab = have_tab && !fmv;
    FiltCoef fc_s = fc, fc_0 = fc;
    if (flat_tab) {
        const float *tb = p.tab.base; const uint32_t pl = p.tab.plane;
        fc_s.alpha = tb[p.tab.sus]; fc_s.beta = tb[pl + p.tab.sus]; fc_s.gamma = tb[2u * pl + p.tab.sus];
        fc_0.alpha = tb[p.tab.end]; fc_0.beta = tb[pl + p.tab.end]; fc_0.gamma = tb[2u * pl + p.tab.end];
    }
    // the two stage changes that are as frequent as note-offs, by hand (s2r_render_onepole.inc: a release that has run out goes to
    // the end stage, a sustain whose booked release begins enters the release line — what the cascade computes for a lane past
    // its attack and decay, simdtest.rs:288-292, in five selects instead of two dozen compares)
    auto end_of_release = [&](float t0) {
        if (ea.s4 == 3.0f && !(t0 < ea.s3)) { ea.s0 = 0.0f; ea.s1 = 0.0f; ea.s2 = 0.0f; ea.s3 = __builtin_inff(); ea.s4 = 4.0f; }
        if (em.s4 == 3.0f && !(t0 < em.s3)) { em.s0 = 0.0f; em.s1 = 0.0f; em.s2 = 0.0f; em.s3 = __builtin_inff(); em.s4 = 4.0f; }
        if (ea.s4 == 2.0f && !(t0 < ea.s3)) { const bool rel = t0 < r.end_a;
            ea.s0 = rel ? lp.amp.slope_rel : 0.0f; ea.s1 = rel ? r.ro_a : 0.0f; ea.s2 = rel ? lp.amp.S : 0.0f;
            ea.s3 = rel ? r.end_a : __builtin_inff(); ea.s4 = rel ? 3.0f : 4.0f; }
        if (em.s4 == 2.0f && !(t0 < em.s3)) { const bool rel = t0 < r.end_m;
            em.s0 = rel ? lp.mod.slope_rel : 0.0f; em.s1 = rel ? r.ro_m : 0.0f; em.s2 = rel ? lp.mod.S : 0.0f;
            em.s3 = rel ? r.end_m : __builtin_inff(); em.s4 = rel ? 3.0f : 4.0f; }
    };
    BankLane bl = make_bank_lane(lp);
    bool wk_dirty = true, wk_ok = false, wk_sine = false, wk_poly = false, wk_fmv = false, wk_dpw = false;
    uint32_t wk_fams = 1u;
    auto classify = [&]() {
        bl = make_bank_lane(lp);
        const uint64_t lm = __ballot(live);
        wk_sine = __ballot(live && lp.osc_kind == S2R_OSC_SINE) != 0ull;
        wk_poly = __ballot(live && lp.osc_kind < S2R_OSC_SINE) != 0ull;
        wk_dpw = OSC == S2R_OSC_ANY && __ballot(live && lp.osc_kind >= S2R_OSC_DPW_SAW && lp.osc_kind <= S2R_OSC_DPW_TRIANGLE) != 0ull;
        // (every started voice with tables and a known oscillator; DPW voices only among themselves)
        wk_ok = lm != 0ull && __ballot(live && !(lp.tab.base != nullptr && lp.osc_kind <= S2R_OSC_DPW_TRIANGLE)) == 0ull &&
                !(wk_dpw && (wk_sine || wk_poly));
        wk_fmv = __ballot(live && lp.amt_osc != 0.0f) != 0ull;
        wk_fams = (__ballot(live && bl.fam == 0u) != 0ull ? 1u : 0u) | (__ballot(live && bl.fam == 1u) != 0ull ? 2u : 0u)
                | (__ballot(live && bl.fam == 2u) != 0ull ? 4u : 0u) | (__ballot(live && bl.fam == 3u) != 0ull ? 8u : 0u);
        wk_dirty = false;
    };

    // Software pipeline of the branch-free chunks' transpose-and-add (as in s2r_render_kernel): the 16 loads of chunk
    // i's column sums are issued right behind its stores, the serial adds and the store of the sum sit in front of the
    // next branch-free chunk's stores; the pending sum (tv, pend_dst) is flushed before anything else touches the tile.
    const uint32_t rf = lane & 15u, rgrp = lane >> 4;
    const float *const tsrc = tile + rf * kTileRow + rgrp * 16u;
    const f4 *const tsrc4 = reinterpret_cast<const f4 *>(tsrc);          // (16-byte aligned: kTileRow)
    float *const sw_dummy = wave_scratch + lane;
    float *pend_dst = sw_dummy;
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
    auto reduce_chunk = [&](uint32_t f_base, uint32_t n_frames) {
        const uint32_t f = lane & 15u, grp = lane >> 4;
        __builtin_amdgcn_wave_barrier();                         // the tile's stores (other lanes') before these loads
        if (f < n_frames) {
            const float *src = tile + f * kTileRow + grp * 16u;
            float acc = src[0];
#pragma unroll
            for (int q = 1; q < 16; ++q) acc += src[q];
            sW[(buf * n_groups + wave * GW + grp) * kSuper + f_base + f] = acc;
        }
        __builtin_amdgcn_wave_barrier();                         // ... and these loads before the next chunk's stores
    };
    auto apply_events_at = [&](uint32_t fpos) {
        if (__ballot(ev_frame == fpos) == 0ull) return;
        while (ev_frame == fpos) {
            const S2rTimedEvent e = tev_load(ctl.tev, ovh, ev_idx);
            if (e.flags & S2R_EV_RESTART) {                      // *voice = Voice { .. }, synth.rs:63-69
                r.pitch = e.pitch;
                r.offset = 0u - fpos;
                r.release_u = 0u;
                r.released = (e.flags & S2R_EV_RELEASE) != 0u;
                r.phase = 0.0f; r.last = 0.0f;
                mod_key = 0xffffffffu;                           // the oscillator constants depend on the pitch
                f2.x1 = f2.x2 = f2.y1 = f2.y2 = 0.0f;
                seed_now = e.seed;
                r.seed_rot = (e.seed << 5) | (e.seed >> 27);
                if constexpr (BANK) { program = e.program; lp = lane_patch_from_bank(p.bank, p.bank_size, program, p.sr, p.no_flat_shortcut ? nullptr : p.tab.base); }
                if (OSC == S2R_OSC_ANY) osc_z = s2r_u2f(S2R_OSC_Z_NONE);
                if constexpr (BANK) fc.k = lp.lpf_kind >= S2R_FILT_SVF_LP ? 1.0f / lp.lpf_damping : 0.0f;
                ev_restart = true; wk_dirty = true;
                k = make_osck_any<OSC>(BANK ? lp.osc_kind : p.osc_kind, (BANK ? lp.sr : p.sr) / r.pitch);    // the new pitch's constants (what FM-free frames use)
                live = true;
            } else if ((e.flags & S2R_EV_RELEASE) && live && !r.released) {   // synth.rs:74-75
                r.released = true;
                r.release_u = r.offset + fpos;
            }
            ev_dirty = true;
            ev_idx = e.next;
            take_releases();                                     // (sets ev_frame: the next event that stays one)
        }
        set_release_thresholds();
        // the envelope cascade for the boundary's frame, so that the chunk can take the branch-free path at once
        const float t0 = (float)(r.offset + fpos);
        ea = env_stage_at(BANK ? lp.amp : p.amp, r.ro_a, r.end_a, t0);
        em = env_stage_at(BANK ? lp.mod : p.mod, r.ro_m, r.end_m, t0);
        thr_min = __builtin_fminf(ea.s3, em.s3);
    };

    // everything below `mod` that depends on it alone (and on the voice's pitch) is kept while no lane's
    // mod-envelope value changes
    auto refresh = [&](float mod) {
        if (__ballot(s2r_f2u(mod) != mod_key) == 0ull) return;
        const float f_osc = s2r_pow2_sleef_core(mod * lp.amt_osc) * r.pitch;     // process.rs:146-147,231-250
        const float f_lpf = s2r_pow2_sleef_core(mod * lp.amt_lpf) * lp.lpf_freq; // process.rs:148-152
        k = make_osck_any<OSC>(lp.osc_kind, lp.sr / f_osc);                      // units.rs:32-42
        if (lp.lpf_kind == S2R_FILT_ONEPOLE) xc = lpf_coeff<false, LanePatch>(lp, f_lpf, sT);
        else fc = dsp_filter_coef(lp.lpf_kind, lp.lpf_damping, lp.sr, f_lpf);
        mod_key = s2r_f2u(mod);
    };

    for (uint32_t sc0 = 0; sc0 < ctl.frames; sc0 += kSuper) {
        const uint32_t n_sc = (ctl.frames - sc0 < kSuper) ? (ctl.frames - sc0) : kSuper;
        const uint32_t n_x16 = (x16_frames > sc0) ? ((x16_frames - sc0 < n_sc) ? (x16_frames - sc0) : n_sc) : 0u;
        if (wave_live) {
            for (uint32_t c16 = 0; c16 < n_x16; c16 += kChunk) {
                if (TEV) apply_events_at(sc0 + c16);
                bool calm = __ballot(!((float)(r.offset + sc0 + c16 + (kChunk - 1u)) < thr_min)) == 0ull;
                if (!calm) {
                    // a stage that ends exactly at this chunk's first frame (the common case: envelope times are mostly
                    // whole multiples of 16 frames): those lanes re-run the cascade for this frame, as at the start of the
                    // fill, and the chunk is calm after all unless a threshold really lies inside it
                    const float t0 = (float)(r.offset + sc0 + c16);
                    if (kFast) { end_of_release(t0); thr_min = __builtin_fminf(ea.s3, em.s3); }
                    if (!(t0 < thr_min)) {
                        ea = env_stage_at(lp.amp, r.ro_a, r.end_a, t0);
                        em = env_stage_at(lp.mod, r.ro_m, r.end_m, t0);
                        thr_min = __builtin_fminf(ea.s3, em.s3);
                    }
                    calm = __ballot(!((float)(r.offset + sc0 + c16 + (kChunk - 1u)) < thr_min)) == 0ull;
                }
                if (kBank && calm) {
                    // (wk_dirty is a per-lane flag set by the lane that restarted)
                    if (__ballot(wk_dirty) != 0ull) classify();
                    const uint32_t left = (n_x16 - c16) / kChunk;
                    const uint32_t o_chunk = r.offset + sc0 + c16;
                    uint32_t run = 0u;
                    if (wk_ok) {
                        auto clear_for = [&](uint32_t n) {
                            return __ballot(!((float)(o_chunk + n * kChunk - 1u) < thr_min)) == 0ull;
                        };
                        run = 1u;
                        uint32_t most = left;
                        if (TEV) {
                            const uint32_t nxt = wave_min_u32(ev_frame);     // 0xffffffff: none
                            const uint32_t until = nxt == 0xffffffffu ? left : (nxt - (sc0 + c16)) / kChunk;
                            most = until < left ? until : left;
                        }
                        if (most > 1u) { if (clear_for(most)) run = most; else if (most > 4u && clear_for(4u)) run = 4u; }
                        // the tables serve offsets below 2^24; a lane whose phase or period is out of the ordinary (a pitch
                        // of 0, inf or NaN; a denormal period, on whose grid RN(period * phase) can reach the period itself — under
                        // FM the per-frame periods are not below 2^-125 while sr >= pitch * 2^-115) sends the wave through the
                        // frame loop
                        const float period0 = lp.sr / r.pitch;
                        const bool lane_bad = live && !(o_chunk + run * kChunk <= (1u << 24) && o_chunk <= (1u << 24)
                                                        && period0 >= 0x1p-126f && period0 < __builtin_inff() && r.phase >= 0.0f && r.phase < 1.0f
                                                        && (lp.amt_osc == 0.0f || lp.sr >= r.pitch * 0x1p-115f));
                        if (__ballot(lane_bad) != 0ull) run = 0u;
                    }
                    if (run) {
                        run = (uint32_t)__builtin_amdgcn_readfirstlane((int)run);
                        // a lane without a started voice reads the "no voice" entries of the first started lane's tables
                        const int first = __builtin_ctzll(__ballot(live));
                        const TabCur cur0 = tab_cursor(lp.tab, em.s4, r.ro_m > lp.mod.sus_off, r.release_u, live);
                        const uint32_t f_off = (uint32_t)__builtin_amdgcn_readlane((int)lp.tab_off, first);
                        const uint32_t f_plane = (uint32_t)__builtin_amdgcn_readlane((int)lp.tab.plane, first);
                        const int32_t f_dead = __builtin_amdgcn_readlane(lp.tab.dead, first);
                        const float *const tbase = p.tab.base + (live ? lp.tab_off : f_off);     // (a kernel argument: global loads)
                        const uint32_t plane = live ? lp.tab.plane : f_plane;
                        const int32_t cidx = live ? cur0.idx : f_dead;
                        const float period0 = live ? lp.sr / r.pitch : 64.0f;
                        auto loop = [&](auto sine_tag, auto poly_tag, auto fmv_tag, auto fams_tag, auto dpw_tag) {
                            for (uint32_t i = 0; i < run; ++i) {
                                const uint32_t f0 = c16 + i * kChunk;
                                float *pvd = (PV && in_range) ? p.per_voice + pv_base + sc0 + f0 : nullptr;
                                const uint32_t oc = o_chunk + i * kChunk;
                                const float *tp = tbase + (ptrdiff_t)(cidx + (int32_t)(oc & cur0.mask));
                                constexpr bool kDpw = decltype(dpw_tag)::value;
                                const float z_new = chunk_bank<decltype(sine_tag)::value, decltype(poly_tag)::value, decltype(fmv_tag)::value,
                                                               decltype(fams_tag)::value, kDpw>(lp, bl, r, f2, kDpw ? osc_z : 0.0f, ea, period0, oc, tp, plane, sSin, live,
                                                                                                tile_lds, pvd, pend_dst, tsrc4);
                                if (kDpw) osc_z = z_new;
                                __builtin_amdgcn_wave_barrier();
                                pend_dst = sW + (buf * n_groups + wave * GW + rgrp) * kSuper + rf + f0;
                            }
                        };
                        const std::true_type T; const std::false_type F;
                        auto pick_osc = [&](auto fmv_tag, auto fams_tag) {
                            if (wk_dpw) loop(F, F, fmv_tag, fams_tag, T);
                            else if (wk_sine && wk_poly) loop(T, T, fmv_tag, fams_tag, F);
                            else if (wk_sine) loop(T, F, fmv_tag, fams_tag, F);
                            else loop(F, T, fmv_tag, fams_tag, F);
                        };
                        auto pick_fmv = [&](auto fams_tag) { if (wk_fmv) pick_osc(T, fams_tag); else pick_osc(F, fams_tag); };
                        switch (wk_fams) {                       // wave-uniform
#define S2R_FAMS_CASE(N) case N: pick_fmv(std::integral_constant<int, N>{}); break;
                        S2R_FAMS_CASE(1) S2R_FAMS_CASE(2) S2R_FAMS_CASE(3) S2R_FAMS_CASE(4) S2R_FAMS_CASE(5) S2R_FAMS_CASE(6)
                        S2R_FAMS_CASE(7) S2R_FAMS_CASE(8) S2R_FAMS_CASE(9) S2R_FAMS_CASE(10) S2R_FAMS_CASE(11) S2R_FAMS_CASE(12)
                        S2R_FAMS_CASE(13) S2R_FAMS_CASE(14)
#undef S2R_FAMS_CASE
                        default: pick_fmv(std::integral_constant<int, 15>{}); break;
                        }
                        mod_key = 0xffffffffu;                   // (the frame loop's cached constants are for another frame now)
                        c16 += (run - 1u) * kChunk;
                        continue;
                    }
                }
                // every lane's mod envelope sits in a zero-slope stage for the whole chunk: its value (0 * (t -
                // base) + y0, the same bits on every frame) is looked at once instead of per frame
                // (lanes without a started voice do not count: their output is a select, their made-up mod value is 0)
                const bool flat = calm && __ballot(live && em.s0 != 0.0f) == 0ull;
                if (flat) {
                    if (flat_tab) {
                        // (the value of a zero-slope stage is its y0: the sustain level or +0 — refresh_flat, s2r_kern_common.h)
                        const bool zero = em.s2 == 0.0f;
                        fc.alpha = zero ? fc_0.alpha : fc_s.alpha; fc.beta = zero ? fc_0.beta : fc_s.beta; fc.gamma = zero ? fc_0.gamma : fc_s.gamma;
                        mod_key = 0xffffffffu;                   // (the frame loop computes its own)
                    } else refresh(live ? env_value(em, (float)(r.offset + sc0 + c16)) : 0.0f);
                }
                // the tables serve offsets below 2^24 (checked for this chunk here, for the whole run below)
                const bool tab_chunk = have_tab && !flat && calm && __ballot(r.offset + sc0 + c16 + kChunk > (1u << 24)) == 0ull;
                if (kFast && calm && (flat || tab_chunk)) {
                    // One patch, and either every lane's mod envelope is flat — oscillator constants and filter
                    // coefficients are constants of the run — or they come from the patch's tables: the branch-free
                    // chunk of the one-pole kernel applies with this patch's filter in its recurrence.  Same run
                    // rule: the LAST frame of the run is below every lane's next threshold.
                    const uint32_t left = (n_x16 - c16) / kChunk;
                    const uint32_t o_chunk = r.offset + sc0 + c16;
                    auto clear_for = [&](uint32_t n) {
                        return __ballot(!((float)(o_chunk + n * kChunk - 1u) < thr_min)) == 0ull;
                    };
                    // The longest clear run in ONE reduction (s2r_render_onepole.inc pick_run): per lane the chunks before its next
                    // threshold — the largest n with o_chunk + 16 n - 1 < thr, exact in f32 below 2^24 — and before its next
                    // timed event, the wave's minimum (DPP), confirmed by the exact test.  (`calm` already covers this chunk.)
                    uint32_t run = 1u;
                    {
                        const float q = ((thr_min - (float)o_chunk) + 1.0f) * 0.0625f;
                        float nf = __builtin_ceilf(q) - 1.0f;
                        nf = __builtin_fminf(__builtin_fmaxf(nf, 1.0f), (float)left);
                        uint32_t n = (uint32_t)nf;
                        if (TEV) { const uint32_t ne = (ev_frame - (sc0 + c16)) >> 4; n = ne < n ? ne : n; }
                        n = wave_min_u32(n);
                        if (n > 1u && clear_for(n)) run = n;
                    }
                    if (tab_chunk && __ballot(o_chunk + run * kChunk > (1u << 24)) != 0ull) run = 1u;
                    // (a NORMAL period — on a denormal one's grid RN(period * phase) can reach the period itself, which chunk_fast does not
                    // fold back to +0; the tables' per-frame periods are not below 2^-125 while sr >= pitch * 2^-115, the power of two being at most 2^10; underflow only)
                    if (__ballot(!(((tab_chunk && fmv) ? (!live || lp.sr >= r.pitch * 0x1p-115f) : (k.period >= 0x1p-126f && k.period < __builtin_inff())) && r.phase >= 0.0f && r.phase < 1.0f)) != 0ull) run = 0u;
                    if (run) {
                        run = (uint32_t)__builtin_amdgcn_readfirstlane((int)run);
                        FlatCache fcx; fcx.xc = xc; fcx.k = k;
                        const FiltCoef fcc = fc;                 // the run's constants, by value
                        const TabCur cur = tab_cursor(p.tab, em.s4, r.ro_m > lp.mod.sus_off, r.release_u, live);
                        // The one-pole kernel's cheaper forms of the chunk (chunk_fast: NZ = 2, AFLAT) apply here unchanged: every
                        // offset of the run below 2^24 and a patch without a noise level; chunk starts on multiples of 16 frames
                        // and rotl(seed, 5) with a zero low nibble on every lane — the chunk's noise is sixteen consecutive
                        // entries of the noise table; and, on top, every started voice's amplitude envelope in a zero-slope
                        // stage — one amplitude per chunk.  (No threshold lies inside the run: the stages hold.)
                        const bool nz_aligned = p.noise_tab != nullptr && p.noise_level == 0.0f &&
                                                __ballot(o_chunk + run * kChunk > (1u << 24) || ((o_chunk | r.seed_rot) & 15u) != 0u) == 0ull;
                        const bool amp_flat = nz_aligned && __ballot(live && ea.s0 != 0.0f) == 0ull;
                        auto run_chunks = [&](auto filt_tag) {
                            constexpr int FILT = decltype(filt_tag)::value;
                            constexpr int O = OSC == S2R_OSC_ANY ? 0 : OSC;
                            auto loop = [&](auto src_tag, auto fmv_tag, auto nz_tag, auto aflat_tag) {   // one tight loop per form of the chunk
                                constexpr int SRC = decltype(src_tag)::value;
                                constexpr bool FMV = decltype(fmv_tag)::value;
                                constexpr int NZ = decltype(nz_tag)::value;
                                constexpr bool AFLAT = decltype(aflat_tag)::value;
                                for (uint32_t i = 0; i < run; ++i) {
                                    const uint32_t f0 = c16 + i * kChunk;
                                    float *pvd = (PV && in_range) ? p.per_voice + pv_base + sc0 + f0 : nullptr;
                                    const uint32_t oc = o_chunk + i * kChunk;
                                    const float *tp = p.tab.base + (ptrdiff_t)(cur.idx + (int32_t)(oc & cur.mask));
                                    *pend_dst = tsum();          // the previous branch-free chunk's sums, in this chunk's basic block
                                    chunk_fast<O, SRC, FILT, FMV, NZ, AFLAT>(p, r, ea, em, fcx, k, oc, tp, sT, sSin, live, tile_lds, pvd, &fcc, &f2);
                                    __builtin_amdgcn_wave_barrier();
                                    pend_dst = sW + (buf * n_groups + wave * GW + rgrp) * kSuper + rf + f0;
                                }
                            };
                            using T = std::true_type; using F = std::false_type;
                            using S0 = std::integral_constant<int, 0>; using S1 = std::integral_constant<int, 1>;
                            using N0 = std::integral_constant<int, 0>; using N2 = std::integral_constant<int, 2>;
                            if (tab_chunk && fmv) loop(S1{}, T{}, N0{}, F{});
                            else if (!tab_chunk) { if (amp_flat) loop(S0{}, F{}, N2{}, T{}); else if (nz_aligned) loop(S0{}, F{}, N2{}, F{}); else loop(S0{}, F{}, N0{}, F{}); }
                            else { if (amp_flat) loop(S1{}, F{}, N2{}, T{}); else if (nz_aligned) loop(S1{}, F{}, N2{}, F{}); else loop(S1{}, F{}, N0{}, F{}); }
                        };
                        switch (lp.lpf_kind) {                   // wave-uniform: the patch is a kernel argument here
                        case S2R_FILT_LP1: run_chunks(std::integral_constant<int, S2R_FILT_LP1>{}); break;
                        case S2R_FILT_HP1: run_chunks(std::integral_constant<int, S2R_FILT_HP1>{}); break;
                        case S2R_FILT_LP2: run_chunks(std::integral_constant<int, S2R_FILT_LP2>{}); break;
                        case S2R_FILT_HP2: run_chunks(std::integral_constant<int, S2R_FILT_HP2>{}); break;
                        case S2R_FILT_BP2: run_chunks(std::integral_constant<int, S2R_FILT_BP2>{}); break;
                        case S2R_FILT_SVF_LP: run_chunks(std::integral_constant<int, S2R_FILT_SVF_LP>{}); break;
                        case S2R_FILT_SVF_BP: run_chunks(std::integral_constant<int, S2R_FILT_SVF_BP>{}); break;
                        case S2R_FILT_SVF_HP: run_chunks(std::integral_constant<int, S2R_FILT_SVF_HP>{}); break;
                        default: break;                          // (the one-pole has its own kernel)
                        }
                        c16 += (run - 1u) * kChunk;
                        continue;
                    }
                }
                flush_pending();
                for (uint32_t j = 0; j < kChunk; ++j) {          // one frame of sample_voice_x16, process.rs:306-379
                    const uint32_t oi = r.offset + sc0 + c16 + j;            // wrapping u32 add (process.rs:213-219)
                    const float t = (float)oi;
                    // the active stages' lines stay valid until t reaches the earlier of their thresholds
                    // (EnvRun, above); `calm`: no lane gets there inside this chunk, so nobody even looks
                    if (!calm && !(t < thr_min)) {
                        ea = env_stage_at(lp.amp, r.ro_a, r.end_a, t);
                        em = env_stage_at(lp.mod, r.ro_m, r.end_m, t);
                        thr_min = __builtin_fminf(ea.s3, em.s3);
                    }
                    const float amp = env_value(ea, t);                                           // process.rs:144
                    const float mod = env_value(em, t);                                           // process.rs:145
                    if (!flat) refresh(mod);
                    const float nz = hash_noise(r.seed_rot, t) + lp.noise_level;                 // process.rs:347-356 (ADD)
                    const float ph = r.phase;                                                    // oscillators.rs:391-400
                    r.phase = s2r_fmod1(ph + k.inv_period);
                    const float off = __builtin_fmaf(k.period, ph, 0.0f);
                    float osc;
                    if (OSC == S2R_OSC_ANY && lp.osc_kind >= S2R_OSC_DPW_SAW) osc = dpw_value(lp.osc_kind, k, off, osc_z);
                    else osc = osc_value_any<OSC>(lp.osc_kind, k, off, sSin);
                    const float smp = (osc + lp.osc_gain) + nz;                                  // process.rs:342-345 (ADD), :358
                    float y;
                    if (lp.lpf_kind == S2R_FILT_ONEPOLE) y = lpf_apply(xc, smp, r.last);         // process.rs:363-371
                    else y = dsp_filter_apply(lp.lpf_kind, fc, smp, f2);
                    const float out = live ? y * amp : 0.0f;                                     // process.rs:373-376
                    if (PV && in_range) p.per_voice[pv_base + sc0 + c16 + j] = out;
                    tile[j * kTileRow + lane] = out;
                }
                reduce_chunk(c16, kChunk);
            }
            flush_pending();
            if (n_x16 < n_sc) {                                  // scalar tail (< 16 frames)
                if (TEV) apply_events_at(sc0 + n_x16);
                for (uint32_t i = n_x16; i < n_sc; ++i) {
                    float out;
                    if (lp.lpf_kind == S2R_FILT_ONEPOLE) out = frame_sisd<OSC, false, LanePatch>(lp, r, r.offset + sc0 + i, sT, sSin, nullptr, &osc_z);
                    else out = frame_sisd<OSC, true, LanePatch>(lp, r, r.offset + sc0 + i, sT, sSin, &f2, &osc_z);
                    out = live ? out : 0.0f;
                    if (PV && in_range) p.per_voice[pv_base + sc0 + i] = out;
                    tile[(i - n_x16) * kTileRow + lane] = out;
                }
                reduce_chunk(n_x16, n_sc - n_x16);
            }
        } else {
            for (uint32_t i = lane; i < GW * kSuper; i += 64u)
                sW[(buf * n_groups + wave * GW + i / kSuper) * kSuper + (i % kSuper)] = 0.0f;
            if (PV && in_range) for (uint32_t i = 0; i < n_sc; ++i) p.per_voice[pv_base + sc0 + i] = 0.0f;
        }
        __syncthreads();
        combine_groups(p, ctl.done, sW + (size_t)buf * n_groups * kSuper, n_groups, kSuper, n_sc, sc0, bp + sc0, tid, blockDim.x, nullptr, 0u, ctl.fused || ctl.ov_render_counter != nullptr);
        buf ^= 1u;
    }

    if (live) {
        const uint32_t o = r.offset;
        p.v.offset[vi] = (!ev_dirty && o > 0xffffffffu - ctl.frames) ? 0xffffffffu : o + ctl.frames;   // synth.rs:197
        p.v.phase[vi] = r.phase;
        p.v.lpf_last[vi] = r.last;
        p.v.fx1[vi] = f2.x1; p.v.fx2[vi] = f2.x2; p.v.fy1[vi] = f2.y1; p.v.fy2[vi] = f2.y2;
        if (OSC == S2R_OSC_ANY) p.v.osc_z[vi] = osc_z;
        else if (ev_restart) p.v.osc_z[vi] = s2r_u2f(S2R_OSC_Z_NONE);     // st::Layer::default(): no DPW memory either
        if (ev_dirty) {
            p.v.pitch[vi] = r.pitch;
            p.v.release[vi] = r.release_u;
            p.v.flags[vi] = S2R_VF_STARTED | (r.released ? S2R_VF_RELEASED : 0u);
            p.v.seed[vi] = seed_now;
            if (BANK) p.v.program[vi] = program;
        }
    }
    if (p.direct_out) signal_done(ctl.done, 1u);                   // (a shard of one workgroup: its output is the fill's)
    if (ctl.ov_render_counter != nullptr) ov_signal(ctl.ov_render_counter);   // (two streams: the mix on the other one waits for every workgroup's row)
    if (ctl.fused) fused_tail(p, ctl, sW, &s_word);              // (one launch per fill: the last workgroups to get here add the rows up)
}

template <int OSC, bool BANK, int MAXT>
__global__ void __launch_bounds__(MAXT) s2r_render_general_kernel(const S2rRenderArgs a) {
    const FillCtl ctl = fill_ctl_from_args(a);
    general_fill<OSC, BANK, MAXT>(a, ctl);
}

// the pool-resident form (S2rPool, s2r_device.h; pool_loop in s2r_kern_common.h): the shard's grid stays on the device and renders
// the fills the host posts — patches with a dsp_filters.rs filter or the SVF, patch banks, the DPW shapes
template <int OSC, bool BANK>
__global__ void __launch_bounds__(256, 1) s2r_pool_general_kernel(const S2rRenderArgs a, const S2rPool pl) {
    pool_loop(a, pl, [&](const FillCtl &ctl) __attribute__((always_inline)) { general_fill<OSC, BANK, 256>(a, ctl); });
}

template <int OSC, bool BANK>
hipError_t launch_general(const S2rRenderArgs &a0, uint32_t block_voices, hipStream_t stream) {
    static thread_local S2rRenderArgs a;                         // 4 KiB of kernel arguments, copied by the launch
    a = a0;
    S2rRenderParams &p = a.p;
    const uint32_t grid = (p.n_voices + block_voices - 1) / block_voices;
    const uint32_t n_waves = block_voices / 64, n_groups = n_waves * 4;
    p.super_frames = n_groups <= 16 ? s2r_pick_super_frames(n_groups, grid, p.frames) : 64u;
    const size_t lds = sizeof(float) * ((size_t)s2r_sw_buffers(p.frames, p.super_frames) * n_groups * p.super_frames + (size_t)n_waves * (kChunk * kTileRow + 64));
    if (lds > 65536) {                                           // (HIP wants to be told about more than 64 KiB of dynamic LDS)
        static thread_local size_t told256 = 0, told1024 = 0;
        if (block_voices <= 256 && told256 < lds) {
            const hipError_t e = hipFuncSetAttribute((const void *)s2r_render_general_kernel<OSC, BANK, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            told256 = lds;
        } else if (block_voices > 256 && told1024 < lds) {
            const hipError_t e = hipFuncSetAttribute((const void *)s2r_render_general_kernel<OSC, BANK, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            told1024 = lds;
        }
    }
    // the launch bound is the register budget (as for s2r_render_kernel): up to 256 threads get the whole file
    if (block_voices <= 256) hipLaunchKernelGGL((s2r_render_general_kernel<OSC, BANK, 256>), dim3(grid), dim3(block_voices), lds, stream, a);
    else hipLaunchKernelGGL((s2r_render_general_kernel<OSC, BANK, 1024>), dim3(grid), dim3(block_voices), lds, stream, a);
    return hipGetLastError();
}

template <int OSC, bool BANK>
hipError_t launch_general_pool(const S2rRenderArgs &a0, const S2rPool &pl, uint32_t block_voices, hipStream_t stream) {
    static thread_local S2rRenderArgs a;
    a = a0;
    S2rRenderParams &p = a.p;
    if (block_voices > 256u || p.per_voice != nullptr || p.direct_out != nullptr) return hipErrorInvalidValue;
    const uint32_t grid = (p.n_voices + block_voices - 1) / block_voices;
    const uint32_t n_waves = block_voices / 64, n_groups = n_waves * 4;
    p.super_frames = s2r_pick_super_frames(n_groups, grid, p.frames);
    const size_t lds = sizeof(float) * ((size_t)s2r_sw_buffers(p.frames, p.super_frames) * n_groups * p.super_frames + (size_t)n_waves * (kChunk * kTileRow + 64));
    if (lds > 65536) {
        static thread_local size_t told = 0;
        if (told < lds) {
            const hipError_t e = hipFuncSetAttribute((const void *)s2r_pool_general_kernel<OSC, BANK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            told = lds;
        }
    }
    hipLaunchKernelGGL((s2r_pool_general_kernel<OSC, BANK>), dim3(grid), dim3(block_voices), lds, stream, a, pl);
    return hipGetLastError();
}

}  // namespace

#define S2R_CAT2(a, b) a##b
#define S2R_CAT(a, b) S2R_CAT2(a, b)
hipError_t S2R_CAT(s2r_launch_general_osc, S2R_TU_OSC)(const S2rRenderArgs &a, uint32_t block_voices, hipStream_t stream) {
    return launch_general<S2R_TU_OSC, (S2R_TU_OSC == S2R_OSC_ANY)>(a, block_voices, stream);
}

hipError_t S2R_CAT(s2r_launch_general_pool_osc, S2R_TU_OSC)(const S2rRenderArgs &a, const S2rPool &pl, uint32_t block_voices, hipStream_t stream) {
    return launch_general_pool<S2R_TU_OSC, (S2R_TU_OSC == S2R_OSC_ANY)>(a, pl, block_voices, stream);
}
