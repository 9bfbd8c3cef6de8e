// s2r_pcm.hip — the PCM stage behind the spectrum meters of s2r_fill_master.  Per channel q of the 18 (bus b at 2 b,
// 2 b + 1, the master at 16, 17) and frame n of the call, in frame order, G = 2^(bits - 1):
//   s = clamp(x, -2, 2) * G (+0.0 for a NaN);   f = sum over k = K .. 1 of h[k-1] * e[n-k], from +0.0, descending;   w = s - f;
//   v = w + d[t + n][q];   r = rint(v);   y = clamp(r, -G, G - 1);   sample = (int)y;   e[n] = clamp(y - w, -2, 2)
// binary32, every operation rounded on its own (-ffp-contract=off), denormals kept, no atomics, no order that depends on timing.
//   s2r_pcm_kernel, ONE launch per call.  Workgroup 0 runs the 18 recursions, which are serial in n and independent of one another:
//   the WALKERS are lanes 0 .. 17 of wave 0, one channel each, in the transposed form: Q[i] is the sum for frame n + i as far as the
//   errors up to e[n-1] reach into it, so that once e[n] exists every Q[i] takes its product h[i] * e[n] independently, and the
//   serial path of a frame is one product, one sum, s - f, w + d, the rounding, two v_med3_f32 and one subtraction.  The walk is
//   compiled for 0, 2, 5 and 9 taps (a tap past K is +0.0, whose products leave every sum as the rule has it: +0.0 + (+-0.0) = +0.0);
//   the taps are wave-uniform.  The STAGERS, waves 1 .. 2, a frame per lane, put s and d of tile j of S2R_PCM_TILE frames into LDS —
//   coalesced float2 loads, a product and two hashes a value — while the walkers walk tile j - 1 out of the other LDS buffer, eight
//   frames read ahead of their chain, and then take the walkers' integers of tile j - 2 from LDS to the pinned samples, one int2 per
//   lane and programme: one barrier per tile, and no walker waits for global memory.  LDS is frame-major, 18 + 18 floats a frame on a
//   stride of 37, and 18 integers on a stride of 19: the walkers' 18 lanes hit 18 consecutive banks, and the stagers' lanes, a frame
//   apart, distinct ones.  Workgroups 1 .. copy the master to the pinned output when no meter kernel has.  The next state goes into
//   the copy nobody reads in this launch.
// -DS2R_PCM_SERIAL builds the obvious form for comparison (tools/pcm_time.py, CHANGELOG): a lane per channel steps through global
// memory frame by frame, its dither computed on the way, step 2 as the rule's loop, every sample stored as it is made.
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float pc2 __attribute__((ext_vector_type(2)));
typedef int pi2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kPcTile = S2R_PCM_TILE;
constexpr uint32_t kPcThreads = 64u + kPcTile;                   // the walkers' wave, then a lane per frame of a tile
constexpr uint32_t kPcCh = S2R_PCM_CHANNELS;
constexpr uint32_t kPcIn = 2u * kPcCh + 1u;                      // floats of a frame in LDS: s[18], d[18], and one to make the stride odd
constexpr uint32_t kPcOut = kPcCh + 1u;                          // integers of a frame in LDS, likewise
constexpr uint32_t kPcBlock = 8;                                 // frames a walker reads from LDS ahead of its chain
constexpr uint32_t kPcTaps = S2R_PCM_MAX_TAPS;
static_assert(kPcTile % kPcBlock == 0u && kPcTile % 64u == 0u && kPcThreads == 192u, "three waves: the walkers', and a frame per lane of two");
static_assert(2u * kPcTile * (kPcIn + kPcOut) * 4u <= 64u * 1024u, "both tiles of both kinds fit the LDS a launch gets unasked");
static_assert(S2R_PCM_PROGRAMMES == S2R_MAX_BUSES + 1u && kPcCh == 2u * S2R_PCM_PROGRAMMES, "s2r.h's programmes");

__device__ __forceinline__ uint32_t pc_mix(uint32_t u) {
    u ^= u >> 16; u *= 0x7feb352du; u ^= u >> 15; u *= 0x846ca68bu; u ^= u >> 16;
    return u;
}
// the rule's step 4 behind its inner hash, `inner` = mix(t_n ^ seed): integers alone, exact in binary32
__device__ __forceinline__ float pc_dither(const uint32_t inner, const uint32_t q, const uint32_t kind) {
    const uint32_t k = pc_mix(inner + q);
    const int r1 = (int)(k >> 16), r2 = (int)(k & 0xffffu);
    if (kind == S2R_DITHER_TRI) return (float)(r1 - r2) * 0x1p-16f;
    if (kind == S2R_DITHER_RECT) return (float)(2 * r1 - 65535) * 0x1p-17f;
    return 0.0f;
}
// min(max(v, lo), hi) for lo < hi and a v that is no NaN: one v_med3_f32
__device__ __forceinline__ float pc_med3(const float v, const float lo, const float hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fmed3f(v, lo, hi);
#else
    return v < lo ? lo : (v > hi ? hi : v);
#endif
}
// the rule's step 1
__device__ __forceinline__ float pc_scale(const float x, const float G) {
    const float xc = x != x ? 0.0f : (x < -2.0f ? -2.0f : (x > 2.0f ? 2.0f : x));
    return xc * G;
}

// A walker: KP sums and KP errors in registers, KP >= K.
template <uint32_t KP> struct PcWalk {
    float h[KP ? KP : 1u], Q[KP ? KP : 1u], e[KP ? KP : 1u];     // e[k] = e[n - 1 - k]
    float G, top;
    uint32_t clips;
    __device__ __forceinline__ void load(const S2rPcm &a, const uint32_t q) {
        G = (float)(1u << (a.bits - 1u)); top = G - 1.0f; clips = 0u;
#pragma unroll
        for (uint32_t k = 0; k < KP; k++) { h[k] = k < a.n_taps ? a.h[k] : 0.0f; e[k] = k < a.n_taps ? a.state[q * kPcTaps + k] : 0.0f; }
        // Q[i] = the sum for the frame i ahead of the call's first, over the taps that reach the state: j = KP .. i + 1, descending
#pragma unroll
        for (uint32_t i = 0; i < KP; i++) {
            float f = 0.0f;
#pragma unroll
            for (uint32_t j = KP; j >= i + 1u; j--) {
                const float p = h[j - 1u] * e[j - 1u - i];
                f = f + p;
            }
            Q[i] = f;
        }
    }
    // steps 3, 5 and 6 of one frame behind its f: the sample, and the error it leaves
    __device__ __forceinline__ int quantise(const float s, const float d, const float f, float &en) {
        const float w = s - f;
        const float v = w + d;
        const float r = __builtin_rintf(v);
        const float y = pc_med3(r, -G, top);
        clips += y != r ? 1u : 0u;
        const float diff = y - w;
        en = pc_med3(diff, -2.0f, 2.0f);
        return (int)y;
    }
    __device__ __forceinline__ void push(const float en) {
        if constexpr (KP > 0u) {
#pragma unroll
            for (uint32_t k = KP - 1u; k >= 1u; k--) e[k] = e[k - 1u];
            e[0] = en;
        }
    }
    // one frame of the transposed form: f is ready, and the new error goes into every sum on its own
    __device__ __forceinline__ int frame(const float s, const float d) {
        float en;
        const int y = quantise(s, d, KP ? Q[0] : 0.0f, en);
        if constexpr (KP > 0u) {
#pragma unroll
            for (uint32_t i = 0; i + 1u < KP; i++) {
                const float p = h[i] * en;
                Q[i] = Q[i + 1u] + p;
            }
            const float p = h[KP - 1u] * en;
            Q[KP - 1u] = 0.0f + p;
        }
        push(en);
        return y;
    }
    // one frame of the direct form: the rule's loop over the errors kept
    __device__ __forceinline__ int frame_direct(const float s, const float d) {
        float f = 0.0f, en;
#pragma unroll
        for (uint32_t j = KP; j >= 1u; j--) {
            const float p = h[j - 1u] * e[j - 1u];
            f = f + p;
        }
        const int y = quantise(s, d, f, en);
        push(en);
        return y;
    }
    __device__ __forceinline__ void store(const S2rPcm &a, const uint32_t q) const {
#pragma unroll
        for (uint32_t k = 0; k < kPcTaps; k++) a.next[q * kPcTaps + k] = k < KP && k < a.n_taps ? e[k < KP ? k : 0u] : 0.0f;
        a.clips[q] = clips;
    }
};

// a channel's input in global memory: the programme's frames, or nothing for a bus past the call's
__device__ __forceinline__ const float *pc_source(const S2rPcm &a, const uint32_t q) {
    const uint32_t p = q >> 1, c = q & 1u;
    if (p == S2R_MAX_BUSES) return a.master + c;
    return p < a.n_buses ? a.stems + (size_t)p * 2u * a.frames + c : nullptr;
}

// workgroup 0, for a walk of KP taps
template <uint32_t KP> __device__ __forceinline__ void pc_run(const S2rPcm &a, float (*sd)[kPcTile * kPcIn], int (*yb)[kPcTile * kPcOut]) {
    const uint32_t tid = threadIdx.x, N = a.frames;
    const bool walker = tid < kPcCh;
    const uint32_t q = tid;
    PcWalk<KP> k;
    if (walker) k.load(a, q);
#ifdef S2R_PCM_SERIAL
    if (walker) {
        const float *const src = pc_source(a, q);
        const float G = (float)(1u << (a.bits - 1u));
        int *const to = a.pcm + (size_t)(q >> 1) * 2u * a.pstride + (q & 1u);
        for (uint32_t n = 0; n < N; n++)
            to[2u * (size_t)n] = k.frame_direct(pc_scale(src ? src[2u * (size_t)n] : 0.0f, G), pc_dither(pc_mix((a.t + n) ^ a.seed), q, a.dither));
    }
#else
    const bool stager = tid >= 64u;
    const uint32_t w = tid - 64u;                                // a stager's frame of a tile
    const float G = (float)(1u << (a.bits - 1u));
    const pc2 *const m2 = reinterpret_cast<const pc2 *>(a.master);
    const uint32_t tiles = (N + kPcTile - 1u) / kPcTile;
    for (uint32_t j = 0; j < tiles + 2u; j++) {
        if (stager) {
            if (j < tiles) {                                     // tile j: s and d of every channel of one frame
                const uint32_t n = j * kPcTile + w;
                float *const to = sd[j & 1u] + w * kPcIn;
                pc2 v[S2R_PCM_PROGRAMMES];
#pragma unroll
                for (uint32_t p = 0; p < S2R_MAX_BUSES; p++) {
                    v[p] = pc2{0.0f, 0.0f};                      // a bus past the call's, and a frame past the call (never walked)
                    if (p < a.n_buses && n < N) v[p] = *reinterpret_cast<const pc2 *>(a.stems + ((size_t)p * N + n) * 2u);
                }
                v[S2R_MAX_BUSES] = n < N ? m2[n] : pc2{0.0f, 0.0f};
                const uint32_t inner = pc_mix((a.t + n) ^ a.seed);
#pragma unroll
                for (uint32_t p = 0; p < S2R_PCM_PROGRAMMES; p++) {
                    to[2u * p] = pc_scale(v[p].x, G); to[2u * p + 1u] = pc_scale(v[p].y, G);
                    to[kPcCh + 2u * p] = pc_dither(inner, 2u * p, a.dither); to[kPcCh + 2u * p + 1u] = pc_dither(inner, 2u * p + 1u, a.dither);
                }
            }
            if (j >= 2u) {                                       // tile j - 2: the walkers' integers, out
                const uint32_t n = (j - 2u) * kPcTile + w;
                const int *const from = yb[j & 1u] + w * kPcOut;
                if (n < N) {
#pragma unroll
                    for (uint32_t p = 0; p < S2R_PCM_PROGRAMMES; p++)
                        *reinterpret_cast<pi2 *>(a.pcm + ((size_t)p * a.pstride + n) * 2u) = pi2{from[2u * p], from[2u * p + 1u]};
                }
            }
        } else if (walker && j >= 1u && j <= tiles) {            // tile j - 1
            const uint32_t t0 = (j - 1u) * kPcTile, cnt = N - t0 < kPcTile ? N - t0 : kPcTile;
            const float *const tp = sd[(j - 1u) & 1u] + q;       // frame i of the tile: s at i * 37, d at i * 37 + 18
            int *const yp = yb[(j - 1u) & 1u] + q;
            float cs[kPcBlock], cd[kPcBlock];
#pragma unroll
            for (uint32_t u = 0; u < kPcBlock; u++) { cs[u] = tp[u * kPcIn]; cd[u] = tp[u * kPcIn + kPcCh]; }
            uint32_t i = 0;
            for (; i + kPcBlock <= cnt; i += kPcBlock) {
                const uint32_t nx = i + kPcBlock < kPcTile ? i + kPcBlock : i;   // the next block, read ahead (the last one: itself again)
                float ns[kPcBlock], nd[kPcBlock];
#pragma unroll
                for (uint32_t u = 0; u < kPcBlock; u++) { ns[u] = tp[(nx + u) * kPcIn]; nd[u] = tp[(nx + u) * kPcIn + kPcCh]; }
#pragma unroll
                for (uint32_t u = 0; u < kPcBlock; u++) yp[(i + u) * kPcOut] = k.frame(cs[u], cd[u]);
#pragma unroll
                for (uint32_t u = 0; u < kPcBlock; u++) { cs[u] = ns[u]; cd[u] = nd[u]; }
            }
            for (; i < cnt; i++) yp[i * kPcOut] = k.frame(tp[i * kPcIn], tp[i * kPcIn + kPcCh]);     // the call's last frames, fewer than a block
        }
        __syncthreads();
    }
#endif
    if (walker) k.store(a, q);
}

}  // namespace

__global__ void __launch_bounds__(kPcThreads) s2r_pcm_kernel(const S2rPcm a) {
    if (blockIdx.x > 0) {
        // ---- the copy: frames [f0, f0 + S2R_PCM_COPY_BLOCK) of the master to the pinned output ----
        const uint32_t f0 = (blockIdx.x - 1u) * S2R_PCM_COPY_BLOCK, f1 = f0 + S2R_PCM_COPY_BLOCK < a.frames ? f0 + S2R_PCM_COPY_BLOCK : a.frames;
        for (uint32_t n = f0 + threadIdx.x; n < f1; n += kPcThreads) reinterpret_cast<pc2 *>(a.out)[n] = reinterpret_cast<const pc2 *>(a.master)[n];
        return;
    }
    // ---- workgroup 0: the recursions ----
    __shared__ float sd[2][kPcTile * kPcIn];                     // two tiles of s and d, [frame][channel]
    __shared__ int yb[2][kPcTile * kPcOut];                      // two tiles of samples, likewise
    const uint32_t K = a.n_taps;                                 // (uniform: the whole workgroup takes one branch)
    if (K == 0u) pc_run<0u>(a, sd, yb);
    else if (K <= 2u) pc_run<2u>(a, sd, yb);
    else if (K <= 5u) pc_run<5u>(a, sd, yb);
    else pc_run<9u>(a, sd, yb);
}

hipError_t s2r_launch_pcm(const S2rPcm &a, hipStream_t stream) {
    if (a.frames == 0) return hipSuccess;
    if (a.n_buses > S2R_MAX_BUSES || (a.n_buses && !a.stems) || !a.master || a.out == a.master || !a.state || !a.next || a.next == a.state || !a.pcm || !a.clips ||
        a.pstride < a.frames || a.bits < S2R_PCM_MIN_BITS || a.bits > S2R_PCM_MAX_BITS || a.dither > S2R_DITHER_TRI || a.n_taps > S2R_PCM_MAX_TAPS)
        return hipErrorInvalidValue;
    const dim3 grid(1u + (a.out ? (a.frames + S2R_PCM_COPY_BLOCK - 1u) / S2R_PCM_COPY_BLOCK : 0u)), block(kPcThreads);
    hipLaunchKernelGGL(s2r_pcm_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}
