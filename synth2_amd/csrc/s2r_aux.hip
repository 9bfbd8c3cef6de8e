// s2r_aux.hip — the small kernels around the render kernels (coefficient tables, note events, mix, decimator) and
// the launch dispatch.  gfx950 only; -ffp-contract=off.
#include "s2r_kern_common.h"

namespace {

// ---------------------------------------------------------------------------------------
// Coefficient tables of one patch (S2rTabRef): one thread per entry.  The mod envelope's value at the
// entry — the very expression the render kernels evaluate, env_value() on the stage's line — goes through the same
// routines a voice would run per frame: sleef pow (process.rs:231-250), then filters.rs:20-24 or dsp_filters.rs.
//   entries [0, n_ad)                     attack + decay, index = frame offset t
//           [n_ad, n_ad + n_rel)          release that starts at the clamp attack + decay, index = t - rc_t0
//           [n_ad + n_rel, n_ad + 2 n_rel) later release, index = t - release_frame_offset
//           then 16 x sustain, 16 x end, 16 x "no voice" (x = 1, 1 - x = 0)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) s2r_table_kernel(const S2rTabBuild b) {
    __shared__ uint64_t sT[S2R_EXP2F_N];
    if (threadIdx.x < S2R_EXP2F_N) sT[threadIdx.x] = c_exp2f_table[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n_entries) return;
    const S2rEnv &e = b.mod;
    float mod;
    bool dead = false;
    if (i < b.n_ad) {
        const float t = (float)i;
        const EnvRun s = env_stage_at(e, __builtin_inff(), __builtin_inff(), t);      // attack, decay (then sustain: padding)
        mod = env_value(s, t);
    } else if (i < b.n_ad + b.n_rel) {
        const float t = (float)(b.rc_t0 + (i - b.n_ad));
        mod = e.slope_rel * (t - e.sus_off) + e.S;               // simdtest.rs:312-318 with release_offset = attack + decay
    } else if (i < b.n_ad + 2u * b.n_rel) {
        const float d = (float)(i - b.n_ad - b.n_rel);           // t - release_offset, exact below 2^24
        mod = e.slope_rel * d + e.S;
    } else if (i < b.n_ad + 2u * b.n_rel + 16u) {
        mod = 0.0f * 1.0f + e.S;                                 // sustain: 0 * (t - 0) + S
    } else {
        mod = 0.0f;                                              // end: 0 * (t - 0) + 0
        dead = i >= b.n_ad + 2u * b.n_rel + 32u;
    }
    const float f_lpf = s2r_pow2_sleef_core(mod * b.amt_lpf) * b.lpf_freq;            // process.rs:148-152
    float c0, c1, c2 = 0.0f;
    if (b.lpf_kind == S2R_FILT_ONEPOLE) {
        const float num = (-2.0f * 3.14159274101257324f) * f_lpf;                     // filters.rs:20-21
        const float arg = b.fast_div_sr ? s2r_div_const_nocheck(num, b.sr, b.rcp_sr) : (num / b.sr);
        c0 = s2r_expf(arg, sT);
        c1 = 1.0f - c0;                                          // a0, filters.rs:23
        if (dead) { c0 = 1.0f; c1 = 0.0f; }
    } else {
        const FiltCoef fc = dsp_filter_coef(b.lpf_kind, b.lpf_damping, b.sr, f_lpf);
        c0 = fc.alpha; c1 = fc.beta; c2 = fc.gamma;
        if (dead) c0 = 1.0f;                                     // (what a lane without a voice reads as the one-pole's x: chunk_bank)
    }
    b.base[i] = c0;
    b.base[(size_t)b.plane + i] = c1;
    if (b.lpf_kind != S2R_FILT_ONEPOLE) b.base[2u * (size_t)b.plane + i] = c2;
    if (b.fm_plane) b.base[(size_t)b.fm_plane * b.plane + i] = dead ? 1.0f : s2r_pow2_sleef_core(mod * b.amt_osc);   // process.rs:146-147
}

// The noise table: entry x = hashnoise.rs:33-51 for the hashed word x (hash_word_x16's input `start.rotl(5) ^ word`, of
// which only the low 16 bits reach the u16 cast): v = (x * 0x9e3779b9) & 0xffff, ((v / 65535) * 2) - 1 with the
// two-operation quotient of s2r_div_u16_by_65535 in its f = v * 2^-16 form — the operations the render kernels ran per
// frame before the table existed.
__global__ void __launch_bounds__(256) s2r_noise_table_kernel(float *t) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    const float f = (float)((x * 0x79b9u) & 0xffffu) * 0x1p-16f;
    const float q = __builtin_fmaf(f, 0x1.0001p-16f, f);
    t[x] = __builtin_fmaf(q, 2.0f, -1.0f);
}

// ---------------------------------------------------------------------------------------
// mix kernel: adds the workgroup partial rows in the fixed order of DESIGN.md 4.3:
//   runs of 16 consecutive workgroups sequentially -> the run sums of a mix group sequentially
//   -> the mix groups sequentially -> root (+0.0) + total.
// One workgroup handles 16 frames: thread (slot, f) adds whole runs (16 independent loads in
// flight each), the run sums meet in LDS, 16 threads finish.  Runs never straddle a mix group.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void mix_body(const S2rMixParams &m, uint32_t block, float *s_run) {
    const bool ov = m.ov_render_counter != nullptr;              // two streams: the rows' render kernel runs beside this launch
    if (ov) {
        if (threadIdx.x == 0 && !ov_wait(m.ov_render_counter, m.ov_render_target)) ov_raise(m.ov_fail, 2u);
        __syncthreads();
    }
    mix_block(m, block, s_run, ov, m.done.flag != nullptr);
    signal_done(m.done, (m.frames + 15u) / 16u);
}

__global__ void __launch_bounds__(256) s2r_mix_kernel(const S2rMixParams m) {
    extern __shared__ float s_run[];                             // [total runs][16 frames]
    tl_mark(m.timeline, m.tl_slot, 0);
    mix_body(m, blockIdx.x, s_run);
    tl_mark(m.timeline, m.tl_slot, 1);
}

// out[i] = ((+0.0 + rows[0][i]) + rows[1][i]) + ...   (rank-order combine of shard partials)
__global__ void s2r_sum_rows_kernel(const float *rows, uint32_t n_rows, uint32_t frames, uint32_t stride, int stereo, float *out, const S2rDone done) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < frames) {
        float total = 0.0f;                                      // accum = splat(0.0), synth.rs:176
        for (uint32_t r = 0; r < n_rows; ++r) total += rows[(size_t)r * stride + f];
        if (stereo) { out_store(done, out + 2u * f, total); out_store(done, out + 2u * f + 1u, total); }   // audio_player.rs:224-228
        else out_store(done, out + f, total);
    }
    signal_done(done, gridDim.x);
}

// build-defined 4x decimator: out[n] = sum over k of h[k] * x[4n + k], taps in index order,
// product and sum rounded separately
constexpr int kDecimTaps = 63;
__global__ void s2r_decimate4_kernel(const float *x, const float *h, uint32_t n_out, float *out) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_out) return;
    float acc = 0.0f;
    for (int k = 0; k < kDecimTaps; ++k) acc = acc + h[k] * x[4u * n + (uint32_t)k];
    out[n] = acc;
}
__global__ void s2r_decimate4_history_kernel(float *x, uint32_t n_out) {
    const uint32_t i = threadIdx.x;                              // one workgroup of 64: read, then write (ranges may overlap)
    float v = 0.0f;
    if (i < kDecimTaps - 1) v = x[4u * n_out + i];
    __syncthreads();
    if (i < kDecimTaps - 1) x[i] = v;
}

// ---------------------------------------------------------------------------------------
// The panned mixdown (s2r_fill_panned).  x_c[v][i] = row[v][i] * g_c[v] for the two channels c, each through
// the tree of DESIGN.md 4.3 — every addition of oracle/s2_oracle.c:rows_blocks_sum, in its order:
//   s2r_pan_mix_kernel: workgroup (tile, b) takes the block_voices voices of workgroup b of the render grid and a tile of
//   32 * W frames.  A thread adds ONE run of 16 voices for W consecutive frames, sequentially in index order from the first
//   voice's value — sixteen independent loads in flight (16 bytes each where the rows allow it: W = 4), every element read once
//   and multiplied by both of its voice's gains — the run sums meet in LDS and are added in run order; voices past the pool add
//   +0.0 (a row of +0.0 times a gain of 0).  The L and R partial rows go to memory.
//   s2r_pan_combine_kernel: one thread per output float adds the workgroups' rows (combine_partials).
// No atomics, no order that depends on timing.  -ffp-contract=off: a product and the sum that takes it stay two roundings.
// ---------------------------------------------------------------------------------------
constexpr uint32_t kPanLanes = 32;                               // threads along frames; 256 / 32 = 8 runs of voices side by side

// What the panned and the bus mixdown share.  One voice's part of a run's rows, x[16][W]: W consecutive frames from f0 — 16 bytes
// where the rows allow it (W == 4: the launcher has checked alignment and whole quads), else a frame per thread; +0.0 past the
// pool (!in_pool) and past the fill.  `src`: the voice's row at frame f0.
template <int W>
__device__ __forceinline__ void load_row(float (&x)[W], const float *src, bool in_pool, uint32_t f0, uint32_t frames) {
    if (W == 4) {
        const f4 q = (in_pool && f0 < frames) ? *reinterpret_cast<const f4 *>(src) : (f4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < W; ++j) x[j] = q[j];
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) x[j] = (in_pool && f0 + (uint32_t)j < frames) ? src[j] : 0.0f;
    }
}

// One output float of a combine kernel: frame f of row c of every workgroup's partial rows, [n_blocks][rows_per_block][pstride],
// added as DESIGN.md 4.3 says — runs of kMixRun workgroups sequentially, the run sums within a mix group, the groups onto a
// root of +0.0.
__device__ __forceinline__ float combine_partials(const float *partials, uint32_t rows_per_block, uint32_t c, uint32_t pstride, uint32_t f,
                                                  uint32_t n_blocks, uint32_t blocks_per_group, uint32_t n_groups) {
    float total = 0.0f;                                          // accum = splat(0.0), synth.rs:176
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t gb0 = g * blocks_per_group;
        uint32_t gb1 = gb0 + blocks_per_group; if (gb1 > n_blocks) gb1 = n_blocks;
        if (gb0 >= gb1) continue;
        float grp = 0.0f;
        for (uint32_t r0 = gb0; r0 < gb1; r0 += kMixRun) {
            const uint32_t r1 = r0 + kMixRun < gb1 ? r0 + kMixRun : gb1;
            float v[kMixRun];
#pragma unroll
            for (uint32_t j = 0; j < kMixRun; ++j) v[j] = (r0 + j < r1) ? partials[((size_t)(r0 + j) * rows_per_block + c) * pstride + f] : 0.0f;
            float acc = v[0];
#pragma unroll
            for (uint32_t j = 1; j < kMixRun; ++j) if (r0 + j < r1) acc = acc + v[j];
            grp = (r0 == gb0) ? acc : grp + acc;
        }
        total = total + grp;
    }
    return total;
}

template <int W>
__global__ void __launch_bounds__(256) s2r_pan_mix_kernel(const S2rPanMix m) {
    extern __shared__ float s_grp[];                             // [block_voices / 16][2][32 * W]
    constexpr uint32_t TF = kPanLanes * (uint32_t)W;
    const uint32_t lane = threadIdx.x & (kPanLanes - 1u), slot = threadIdx.x / kPanLanes, n_slots = blockDim.x / kPanLanes;
    const uint32_t b = blockIdx.y, fl = lane * (uint32_t)W, f0 = blockIdx.x * TF + fl;
    const uint32_t n_grp = m.block_voices / 16u;
    for (uint32_t g = slot; g < n_grp; g += n_slots) {
        const uint32_t v0 = b * m.block_voices + 16u * g;
        float x[16][W], gl[16], gr[16];
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {
            const uint32_t v = v0 + k;
            gl[k] = m.gain_l[v]; gr[k] = m.gain_r[v];            // (padded with 0 up to the grid's last voice)
            load_row<W>(x[k], m.rows + (size_t)v * m.stride + f0, v < m.n_voices, f0, m.frames);
        }
        float al[W], ar[W];
#pragma unroll
        for (int j = 0; j < W; ++j) { al[j] = x[0][j] * gl[0]; ar[j] = x[0][j] * gr[0]; }
#pragma unroll
        for (uint32_t k = 1; k < 16u; ++k) {
#pragma unroll
            for (int j = 0; j < W; ++j) { al[j] = al[j] + x[k][j] * gl[k]; ar[j] = ar[j] + x[k][j] * gr[k]; }
        }
#pragma unroll
        for (int j = 0; j < W; ++j) { s_grp[(2u * g) * TF + fl + (uint32_t)j] = al[j]; s_grp[(2u * g + 1u) * TF + fl + (uint32_t)j] = ar[j]; }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2u * TF; i += blockDim.x) {
        const uint32_t c = i / TF, t = i - c * TF, f = blockIdx.x * TF + t;
        if (f >= m.frames) continue;
        float acc = s_grp[c * TF + t];
        for (uint32_t g = 1; g < n_grp; ++g) acc = acc + s_grp[(2u * g + c) * TF + t];
        m.partials[((size_t)b * 2u + c) * m.pstride + f] = acc;
    }
}

__global__ void __launch_bounds__(256) s2r_pan_combine_kernel(const S2rPanMix m) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;    // out[i]: frame i / 2, channel i & 1
    const uint32_t f = i >> 1, c = i & 1u;
    if (f >= m.frames) return;
    m.out[i] = combine_partials(m.partials, 2u, c, m.pstride, f, m.n_blocks, m.blocks_per_group, m.n_groups);
}

// ---------------------------------------------------------------------------------------
// The bus mixdown (s2r_fill_buses): up to 8 stereo buses from ONE read of the rows.  Per bus q and channel c
// x[v][i] = row[v][i] * gb_c[v], gb_c[v] = (min(bus[v], n_buses - 1) == q) ? g_c[v] : +0.0 (g_c: the pan gain times the voice's
// gain, multiplied on the host), through the same tree as the panned mixdown above — an off-bus voice is a term of row * +0.0,
// not a skipped one.
//   s2r_bus_mix_kernel<W, NB, RAMP, SEND>: the geometry of s2r_pan_mix_kernel — workgroup (tile, b), a thread adds ONE run of 16 voices for W
//   consecutive frames — with `lanes` threads along the frames: the launcher halves the tile until [block_voices / 16][2 * NB][tile]
//   floats fit 32 KiB of LDS, so that several workgroups share a compute unit.  The run's 16 x W row elements are loaded once and
//   stay in registers; bus after bus (NB is compiled in: no indexed accumulator, nothing in scratch) the sixteen gains are
//   selected once per voice and the run is multiplied and added into W L and W R sums, which go to LDS.  The surplus buses of an
//   instantiation (n_buses < NB) are neither computed nor stored.
//   s2r_bus_combine_kernel: s2r_pan_combine_kernel with a bus index.
// ---------------------------------------------------------------------------------------
constexpr uint32_t kBusLdsBytes = 32u << 10;

// One argument block (S2rBusMix) for every form; the launcher compiles in which of its optional pointers are given.
//   RAMP (d_l, d_r given: program faders moving): the gain of a voice is G0 + (float)i * d at frame i of the CALL —
//   frame_base is the call-relative frame of the rows' first frame.  Per bus the run selects (G0, d) once per voice and channel,
//   exactly as the static form selects its gain (an off-bus voice: +0.0 + i * +0.0 = +0.0), and every element takes a multiply and
//   an add for its gain in front of the static form's multiply and add: nothing but the sixteen voices' two steps and W frame
//   numbers is added to the registers the run keeps live.
//   SEND (send, send_bus given: aux sends): a voice feeds a second bus with its gain times its send, h = g * s (one
//   rounded multiply, here: the run keeps the voices' s and send bus live, 32 more values, not the 48 or 80 of gains multiplied on
//   the host).  Per bus the run selects the main gain and the send's gain with a compare each and adds them once per voice and
//   channel — M + A, and under RAMP likewise for the step — before the W frames are touched; with s = 0 the sum is M bit for bit
//   (gains are finite and not negative).
//   A form that is compiled out reads none of its pointers and keeps none of its values.
template <int W, int NB, bool RAMP, bool SEND>
__global__ void __launch_bounds__(256) s2r_bus_mix_kernel(const S2rBusMix m) {
    extern __shared__ float s_bus[];                             // [block_voices / 16][2 * NB][lanes * W]
    const uint32_t lanes = m.lanes, TF = lanes * (uint32_t)W;
    const uint32_t lane = threadIdx.x & (lanes - 1u), slot = threadIdx.x / lanes, n_slots = blockDim.x / lanes;
    const uint32_t b = blockIdx.y, fl = lane * (uint32_t)W, f0 = blockIdx.x * TF + fl;
    const uint32_t n_grp = m.block_voices / 16u, last = m.n_buses - 1u;
    for (uint32_t g = slot; g < n_grp; g += n_slots) {
        const uint32_t v0 = b * m.block_voices + 16u * g;
        float x[16][W], gl[16], gr[16];
        float dl[RAMP ? 16 : 1], dr[RAMP ? 16 : 1], fi[RAMP ? W : 1];
        float sd[SEND ? 16 : 1];
        uint32_t vb[16], sq[SEND ? 16 : 1];
        if (RAMP) {
#pragma unroll
            for (int j = 0; j < W; ++j) fi[RAMP ? j : 0] = (float)(m.frame_base + f0 + (uint32_t)j);      // i of the call, not of the slice
        }
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {
            const uint32_t v = v0 + k;
            gl[k] = m.gain_l[v]; gr[k] = m.gain_r[v];            // (padded with 0 up to the grid's last voice)
            if (RAMP) { dl[RAMP ? k : 0u] = m.d_l[v]; dr[RAMP ? k : 0u] = m.d_r[v]; }
            const uint32_t q = m.bus[v];
            vb[k] = q < last ? q : last;                         // a voice booked past the call's buses sounds on the last one
            if (SEND) {
                sd[SEND ? k : 0u] = m.send[v];
                const uint32_t t = m.send_bus[v];
                sq[SEND ? k : 0u] = t < last ? t : last;         // ... and so does its send
            }
            load_row<W>(x[k], m.rows + (size_t)v * m.stride + f0, v < m.n_voices, f0, m.frames);
        }
#pragma unroll
        for (uint32_t q = 0; q < (uint32_t)NB; ++q) {
            if (q > last) break;
            float al[W], ar[W];
#pragma unroll
            for (uint32_t k = 0; k < 16u; ++k) {
                float sl = vb[k] == q ? gl[k] : 0.0f, sr = vb[k] == q ? gr[k] : 0.0f;
                float tl = RAMP && vb[k] == q ? dl[RAMP ? k : 0u] : 0.0f, tr = RAMP && vb[k] == q ? dr[RAMP ? k : 0u] : 0.0f;
                if (SEND) {                                      // gb = M + A: the main gain or +0.0, plus g * s or +0.0 (one rounded add)
                    const bool on = sq[SEND ? k : 0u] == q;
                    const float s = sd[SEND ? k : 0u];
                    const float hl = gl[k] * s, hr = gr[k] * s;
                    sl = sl + (on ? hl : 0.0f); sr = sr + (on ? hr : 0.0f);
                    if (RAMP) {
                        const float el = dl[RAMP ? k : 0u] * s, er = dr[RAMP ? k : 0u] * s;
                        tl = tl + (on ? el : 0.0f); tr = tr + (on ? er : 0.0f);
                    }
                }
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    float el = sl, er = sr;
                    if (RAMP) {                                  // (-ffp-contract=off: the step's product is rounded before the sum)
                        const float ul = fi[RAMP ? j : 0] * tl, ur = fi[RAMP ? j : 0] * tr;
                        el = sl + ul; er = sr + ur;
                    }
                    const float pl = x[k][j] * el, pr = x[k][j] * er;
                    al[j] = k ? al[j] + pl : pl; ar[j] = k ? ar[j] + pr : pr;
                }
            }
            float *dst_l = s_bus + ((size_t)g * (2u * NB) + 2u * q) * TF + fl, *dst_r = dst_l + TF;
            if (W == 4) {
                *reinterpret_cast<f4 *>(dst_l) = (f4){al[0], al[1 % W], al[2 % W], al[3 % W]};
                *reinterpret_cast<f4 *>(dst_r) = (f4){ar[0], ar[1 % W], ar[2 % W], ar[3 % W]};
            } else {
#pragma unroll
                for (int j = 0; j < W; ++j) { dst_l[j] = al[j]; dst_r[j] = ar[j]; }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2u * m.n_buses * TF; i += blockDim.x) {
        const uint32_t c = i / TF, t = i - c * TF, f = blockIdx.x * TF + t;       // c: 2 * bus + channel
        if (f >= m.frames) continue;
        float acc = s_bus[c * TF + t];
        for (uint32_t g = 1; g < n_grp; ++g) acc = acc + s_bus[((size_t)g * (2u * NB) + c) * TF + t];
        m.partials[((size_t)b * (2u * S2R_MAX_BUSES) + c) * m.pstride + f] = acc;
    }
}

__global__ void __launch_bounds__(256) s2r_bus_combine_kernel(const S2rBusMix m) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;    // bus i / (2 * frames); inside it frame r / 2, channel r & 1
    const uint32_t per = 2u * m.frames, q = i / per, r = i - q * per, f = r >> 1, c = 2u * q + (r & 1u);
    if (q >= m.n_buses) return;
    m.out[(size_t)q * m.ostride + r] = combine_partials(m.partials, 2u * S2R_MAX_BUSES, c, m.pstride, f, m.n_blocks, m.blocks_per_group, m.n_groups);
}

// publishes the first timed event of every touched voice
// ... and moves the records from mapped host memory into HBM in one coalesced sweep: the coefficient pass and
// the render kernel follow per-voice chains through them, and a PCIe round trip per hop is what they cannot afford
// (It touches no voice state — a chain's first record that sits at frame 0, the fill's folded untimed events, is applied
// by the render kernel's prologue — so the host may run it beside the previous fill's render kernel.)
// (`ov`: two streams — the copy and the heads are handed to a render kernel that may already be running: write-through stores)
__device__ __forceinline__ void heads_body(int32_t *heads, const S2rTimedEvent *tev, S2rTimedEvent *tev_copy, uint32_t n, uint32_t i, bool ov) {
    if (i >= n) return;
    const S2rTimedEvent e = tev[i];
    if (ov) {
        static_assert(sizeof(S2rTimedEvent) == 32, "two 16-byte stores");
        float *dst = reinterpret_cast<float *>(tev_copy + i);
        ov_store4(dst, (f4){s2r_u2f(e.voice), s2r_u2f(e.frame), s2r_u2f(e.flags), e.pitch});
        ov_store4(dst + 4, (f4){s2r_u2f(e.seed), s2r_u2f((uint32_t)e.next), s2r_u2f(e.program), 0.0f});
        if (e.flags & S2R_TEV_FIRST) ov_store(heads + e.voice, (int32_t)i);
    } else {
        tev_copy[i] = e;
        if (e.flags & S2R_TEV_FIRST) heads[e.voice] = (int32_t)i;
    }
}

__global__ void s2r_tev_heads_kernel(int32_t *heads, const S2rTimedEvent *tev, S2rTimedEvent *tev_copy, uint32_t n, uint32_t *ov_heads_counter) {
    heads_body(heads, tev, tev_copy, n, blockIdx.x * blockDim.x + threadIdx.x, ov_heads_counter != nullptr);
    if (ov_heads_counter != nullptr) ov_signal(ov_heads_counter);
}

// Between two render kernels of a caller with several fills in flight: the PREVIOUS fill's mix (its first `mix_blocks`
// workgroups) and THIS fill's chain heads (the rest) in one launch — the two have nothing to do with each other, and a
// launch boundary costs the stream more than either of them.
__global__ void __launch_bounds__(256) s2r_mix_and_heads_kernel(const S2rMixParams m, uint32_t mix_blocks, int32_t *heads,
                                                                const S2rTimedEvent *tev, S2rTimedEvent *tev_copy, uint32_t n) {
    extern __shared__ float s_run[];
    tl_mark(m.timeline, m.tl_slot, 0);
    if (blockIdx.x < mix_blocks) mix_body(m, blockIdx.x, s_run);
    else {
        heads_body(heads, tev, tev_copy, n, (blockIdx.x - mix_blocks) * blockDim.x + threadIdx.x, m.ov_heads_counter != nullptr);
        if (m.ov_heads_counter != nullptr) ov_signal(m.ov_heads_counter);
    }
    tl_mark(m.timeline, m.tl_slot, 1);
}

// note events folded per voice by the host (synth.rs:61-80)
__global__ void s2r_events_kernel(const S2rVoiceArrays v, const S2rVoiceEvent *ev, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const S2rVoiceEvent e = ev[i];
    const uint32_t vi = e.voice;
    if (e.flags & S2R_EV_RESTART) {                              // *voice = Voice { .. }, synth.rs:63-69
        v.pitch[vi] = e.pitch;
        v.offset[vi] = 0u;
        v.release[vi] = 0u;                                      // a release right after the on is at offset 0
        v.flags[vi] = S2R_VF_STARTED | ((e.flags & S2R_EV_RELEASE) ? S2R_VF_RELEASED : 0u);
        v.phase[vi] = 0.0f;
        v.lpf_last[vi] = 0.0f;
        v.fx1[vi] = 0.0f; v.fx2[vi] = 0.0f; v.fy1[vi] = 0.0f; v.fy2[vi] = 0.0f;
        v.seed[vi] = e.seed;
        v.program[vi] = e.flags >> S2R_EV_PROGRAM_SHIFT;
        v.osc_z[vi] = s2r_u2f(S2R_OSC_Z_NONE);
    } else if (e.flags & S2R_EV_RELEASE) {                       // synth.rs:74-75
        const uint32_t fl = v.flags[vi];
        if ((fl & S2R_VF_STARTED) && !(fl & S2R_VF_RELEASED)) {
            v.release[vi] = v.offset[vi];
            v.flags[vi] = fl | S2R_VF_RELEASED;
        }
    }
}
}  // namespace

hipError_t s2r_launch_onepole_resident_osc0(const S2rRenderArgs &a, const S2rResident &rs, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_onepole_resident_osc1(const S2rRenderArgs &a, const S2rResident &rs, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_onepole_resident_osc2(const S2rRenderArgs &a, const S2rResident &rs, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_onepole_resident_osc3(const S2rRenderArgs &a, const S2rResident &rs, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_onepole_pool_osc0(const S2rRenderArgs &a, const S2rPool &pl, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_onepole_pool_osc1(const S2rRenderArgs &a, const S2rPool &pl, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_onepole_pool_osc2(const S2rRenderArgs &a, const S2rPool &pl, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_onepole_pool_osc3(const S2rRenderArgs &a, const S2rPool &pl, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_onepole_osc0(const S2rRenderArgs &a, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_onepole_osc1(const S2rRenderArgs &a, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_onepole_osc2(const S2rRenderArgs &a, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_onepole_osc3(const S2rRenderArgs &a, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_general_pool_osc0(const S2rRenderArgs &a, const S2rPool &pl, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_general_pool_osc1(const S2rRenderArgs &a, const S2rPool &pl, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_general_pool_osc2(const S2rRenderArgs &a, const S2rPool &pl, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_general_pool_osc3(const S2rRenderArgs &a, const S2rPool &pl, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_general_pool_osc15(const S2rRenderArgs &a, const S2rPool &pl, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_general_osc0(const S2rRenderArgs &a, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_general_osc1(const S2rRenderArgs &a, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_general_osc2(const S2rRenderArgs &a, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_general_osc3(const S2rRenderArgs &a, uint32_t block_voices, hipStream_t stream);
hipError_t s2r_launch_general_osc15(const S2rRenderArgs &a, uint32_t block_voices, hipStream_t stream);   // the patch bank

hipError_t s2r_launch_tables(const S2rTabBuild &b, hipStream_t stream) {
    if (b.n_entries == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(s2r_table_kernel, dim3((b.n_entries + 255u) / 256u), dim3(256), 0, stream, b);
    return hipGetLastError();
}

hipError_t s2r_launch_noise_table(float *table_65536, hipStream_t stream) {
    hipLaunchKernelGGL(s2r_noise_table_kernel, dim3(65536 / 256), dim3(256), 0, stream, table_65536);
    return hipGetLastError();
}

hipError_t s2r_launch_render(const S2rRenderArgs &a, uint32_t block_voices, hipStream_t stream) {
    const S2rRenderParams &p = a.p;
    if (p.n_voices == 0 || p.frames == 0) return hipSuccess;
    if (block_voices < 64 || block_voices > 1024 || (block_voices & 63u)) return hipErrorInvalidValue;
    // patch banks, and the DPW oscillator shapes (which exist in that kernel only): oscillator and filter kind per lane
    if (p.bank_size > 1 || p.osc_kind > S2R_OSC_SINE) return s2r_launch_general_osc15(a, block_voices, stream);
    const bool general = p.lpf_kind != S2R_FILT_ONEPOLE;
    switch (p.osc_kind) {
    case S2R_OSC_SQUARE: return general ? s2r_launch_general_osc0(a, block_voices, stream) : s2r_launch_onepole_osc0(a, block_voices, stream);
    case S2R_OSC_SAW: return general ? s2r_launch_general_osc1(a, block_voices, stream) : s2r_launch_onepole_osc1(a, block_voices, stream);
    case S2R_OSC_TRIANGLE: return general ? s2r_launch_general_osc2(a, block_voices, stream) : s2r_launch_onepole_osc2(a, block_voices, stream);
    case S2R_OSC_SINE: return general ? s2r_launch_general_osc3(a, block_voices, stream) : s2r_launch_onepole_osc3(a, block_voices, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t s2r_launch_resident(const S2rRenderArgs &a, const S2rResident &rs, uint32_t block_voices, hipStream_t stream) {
    const S2rRenderParams &p = a.p;
    if (p.n_voices == 0 || p.frames == 0 || p.bank_size > 1 || p.lpf_kind != S2R_FILT_ONEPOLE) return hipErrorInvalidValue;
    switch (p.osc_kind) {
    case S2R_OSC_SQUARE: return s2r_launch_onepole_resident_osc0(a, rs, block_voices, stream);
    case S2R_OSC_SAW: return s2r_launch_onepole_resident_osc1(a, rs, block_voices, stream);
    case S2R_OSC_TRIANGLE: return s2r_launch_onepole_resident_osc2(a, rs, block_voices, stream);
    case S2R_OSC_SINE: return s2r_launch_onepole_resident_osc3(a, rs, block_voices, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t s2r_launch_pool(const S2rRenderArgs &a, const S2rPool &pl, uint32_t block_voices, hipStream_t stream) {
    const S2rRenderParams &p = a.p;
    if (p.n_voices == 0 || p.frames == 0) return hipErrorInvalidValue;
    // patch banks, and the DPW oscillator shapes: the kernel with oscillator and filter kind per lane
    if (p.bank_size > 1 || p.osc_kind > S2R_OSC_SINE) return s2r_launch_general_pool_osc15(a, pl, block_voices, stream);
    const bool general = p.lpf_kind != S2R_FILT_ONEPOLE;
    switch (p.osc_kind) {
    case S2R_OSC_SQUARE: return general ? s2r_launch_general_pool_osc0(a, pl, block_voices, stream) : s2r_launch_onepole_pool_osc0(a, pl, block_voices, stream);
    case S2R_OSC_SAW: return general ? s2r_launch_general_pool_osc1(a, pl, block_voices, stream) : s2r_launch_onepole_pool_osc1(a, pl, block_voices, stream);
    case S2R_OSC_TRIANGLE: return general ? s2r_launch_general_pool_osc2(a, pl, block_voices, stream) : s2r_launch_onepole_pool_osc2(a, pl, block_voices, stream);
    case S2R_OSC_SINE: return general ? s2r_launch_general_pool_osc3(a, pl, block_voices, stream) : s2r_launch_onepole_pool_osc3(a, pl, block_voices, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t s2r_launch_mix(const S2rMixParams &m, hipStream_t stream) {
    if (m.frames == 0) return hipSuccess;
    const uint32_t runs_per_group = (m.blocks_per_group + kMixRun - 1) / kMixRun;
    const size_t lds = (size_t)runs_per_group * m.n_groups * 16u * sizeof(float);
    if (lds > 64u * 1024u) return hipErrorInvalidValue;          // > 16 k workgroups in one shard
    hipLaunchKernelGGL(s2r_mix_kernel, dim3((m.frames + 15) / 16), dim3(256), lds, stream, m);
    return hipGetLastError();
}

hipError_t s2r_launch_mix_and_heads(const S2rMixParams &m, int32_t *heads, const S2rTimedEvent *tev, S2rTimedEvent *tev_copy, uint32_t n,
                                    hipStream_t stream) {
    if (m.frames == 0) return s2r_launch_tev_heads(heads, tev, tev_copy, n, stream, m.ov_heads_counter);
    if (n == 0) return s2r_launch_mix(m, stream);
    const uint32_t runs_per_group = (m.blocks_per_group + kMixRun - 1) / kMixRun;
    const size_t lds = (size_t)runs_per_group * m.n_groups * 16u * sizeof(float);
    if (lds > 64u * 1024u) return hipErrorInvalidValue;
    const uint32_t mix_blocks = (m.frames + 15) / 16;
    hipLaunchKernelGGL(s2r_mix_and_heads_kernel, dim3(mix_blocks + (n + 255) / 256), dim3(256), lds, stream, m, mix_blocks, heads, tev, tev_copy, n);
    return hipGetLastError();
}

hipError_t s2r_launch_events(const S2rVoiceArrays &v, const S2rVoiceEvent *dev_events, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(s2r_events_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, v, dev_events, n);
    return hipGetLastError();
}

hipError_t s2r_launch_tev_heads(int32_t *heads, const S2rTimedEvent *tev, S2rTimedEvent *tev_copy, uint32_t n, hipStream_t stream,
                                uint32_t *ov_heads_counter) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(s2r_tev_heads_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, heads, tev, tev_copy, n, ov_heads_counter);
    return hipGetLastError();
}

hipError_t s2r_launch_decimate4(float *x_with_history, const float *taps, uint32_t n_out, float *out, hipStream_t stream) {
    if (n_out == 0) return hipSuccess;
    hipLaunchKernelGGL(s2r_decimate4_kernel, dim3((n_out + 255) / 256), dim3(256), 0, stream, x_with_history, taps, n_out, out);
    hipLaunchKernelGGL(s2r_decimate4_history_kernel, dim3(1), dim3(64), 0, stream, x_with_history, n_out);
    return hipGetLastError();
}

hipError_t s2r_launch_sum_rows(const float *rows, uint32_t n_rows, uint32_t frames, uint32_t stride, int stereo, float *out, hipStream_t stream,
                               const S2rDone *done) {
    if (frames == 0) return hipSuccess;
    hipLaunchKernelGGL(s2r_sum_rows_kernel, dim3((frames + 255) / 256), dim3(256), 0, stream, rows, n_rows, frames, stride, stereo, out,
                       done ? *done : S2rDone{nullptr, 0u, nullptr});
    return hipGetLastError();
}

hipError_t s2r_launch_pan_mix(const S2rPanMix &m, hipStream_t stream) {
    if (m.frames == 0 || m.n_voices == 0) return hipSuccess;
    if (m.block_voices < 64 || m.block_voices > 1024 || (m.block_voices & 63u) || m.n_blocks * m.block_voices < m.n_voices || m.n_blocks > 65535u ||
        m.stride < m.frames || m.pstride < m.frames || m.n_groups == 0 || m.blocks_per_group * m.n_groups < m.n_blocks)
        return hipErrorInvalidValue;
    // 16-byte loads where every row starts on a 16-byte boundary and holds whole quads of frames; else a frame per thread
    const bool wide = (m.stride & 3u) == 0 && (m.frames & 3u) == 0 && (reinterpret_cast<uintptr_t>(m.rows) & 15u) == 0;
    const uint32_t tf = kPanLanes * (wide ? 4u : 1u);
    const size_t lds = (size_t)(m.block_voices / 16u) * 2u * tf * sizeof(float);      // at most 64 KiB (1024 voices, wide)
    const dim3 grid((m.frames + tf - 1u) / tf, m.n_blocks);
    if (wide) hipLaunchKernelGGL(s2r_pan_mix_kernel<4>, grid, dim3(256), lds, stream, m);
    else hipLaunchKernelGGL(s2r_pan_mix_kernel<1>, grid, dim3(256), lds, stream, m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(s2r_pan_combine_kernel, dim3((2u * m.frames + 255u) / 256u), dim3(256), 0, stream, m);
    return hipGetLastError();
}

template <int W, bool RAMP, bool SEND>
static void bus_mix_launch(const S2rBusMix &m, uint32_t nb, dim3 grid, dim3 block, size_t lds, hipStream_t stream) {
    switch (nb) {
    case 1: hipLaunchKernelGGL((s2r_bus_mix_kernel<W, 1, RAMP, SEND>), grid, block, lds, stream, m); break;
    case 2: hipLaunchKernelGGL((s2r_bus_mix_kernel<W, 2, RAMP, SEND>), grid, block, lds, stream, m); break;
    case 4: hipLaunchKernelGGL((s2r_bus_mix_kernel<W, 4, RAMP, SEND>), grid, block, lds, stream, m); break;
    default: hipLaunchKernelGGL((s2r_bus_mix_kernel<W, 8, RAMP, SEND>), grid, block, lds, stream, m); break;
    }
}

template <int W>
static void bus_mix_launch(const S2rBusMix &m, uint32_t nb, dim3 grid, dim3 block, size_t lds, hipStream_t stream) {
    const bool ramp = m.d_l != nullptr, send = m.send != nullptr;
    if (ramp && send) bus_mix_launch<W, true, true>(m, nb, grid, block, lds, stream);
    else if (ramp) bus_mix_launch<W, true, false>(m, nb, grid, block, lds, stream);
    else if (send) bus_mix_launch<W, false, true>(m, nb, grid, block, lds, stream);
    else bus_mix_launch<W, false, false>(m, nb, grid, block, lds, stream);
}

hipError_t s2r_launch_bus_mix(const S2rBusMix &in, hipStream_t stream) {
    S2rBusMix m = in;
    if (!m.d_l != !m.d_r || !m.send != !m.send_bus) return hipErrorInvalidValue;     // half a pair
    if (m.frames == 0 || m.n_voices == 0) return hipSuccess;
    if (m.block_voices < 64 || m.block_voices > 1024 || (m.block_voices & 63u) || m.n_blocks * m.block_voices < m.n_voices || m.n_blocks > 65535u ||
        m.stride < m.frames || m.pstride < m.frames || m.n_groups == 0 || m.blocks_per_group * m.n_groups < m.n_blocks ||
        m.n_buses == 0 || m.n_buses > S2R_MAX_BUSES || m.ostride < 2u * (size_t)m.frames)
        return hipErrorInvalidValue;
    // 16-byte loads where every row starts on a 16-byte boundary and holds whole quads of frames; else a frame per thread
    const bool wide = (m.stride & 3u) == 0 && (m.frames & 3u) == 0 && (reinterpret_cast<uintptr_t>(m.rows) & 15u) == 0;
    const uint32_t w = wide ? 4u : 1u, nb = m.n_buses <= 1u ? 1u : m.n_buses <= 2u ? 2u : m.n_buses <= 4u ? 4u : 8u;
    const uint32_t n_grp = m.block_voices / 16u;
    // the frame tile: 32 threads along the frames, halved until the run sums of every bus fit kBusLdsBytes (256 voices: 8 buses
    // 8 lanes, 4 buses 16, fewer 32 — 32 KiB at the most, 16 KiB for 1024 voices and 8 buses on one lane)
    m.lanes = kPanLanes;
    while (m.lanes > 1u && (size_t)n_grp * 2u * nb * m.lanes * w * sizeof(float) > kBusLdsBytes) m.lanes >>= 1;
    const uint32_t tf = m.lanes * w;
    const size_t lds = (size_t)n_grp * 2u * nb * tf * sizeof(float);
    uint32_t threads = (n_grp * m.lanes + 63u) & ~63u;            // a thread per run and lane, whole waves, 256 at the most
    if (threads > 256u) threads = 256u;
    const dim3 grid((m.frames + tf - 1u) / tf, m.n_blocks);
    if (wide) bus_mix_launch<4>(m, nb, grid, dim3(threads), lds, stream);
    else bus_mix_launch<1>(m, nb, grid, dim3(threads), lds, stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(s2r_bus_combine_kernel, dim3((2u * m.frames * m.n_buses + 255u) / 256u), dim3(256), 0, stream, m);
    return hipGetLastError();
}
