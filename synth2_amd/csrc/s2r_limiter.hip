// s2r_limiter.hip — the look-ahead limiter behind the master fader of s2r_fill_master: a gain per frame from the
// larger channel magnitude, a sliding minimum over L + H + 1 gains, a box mean of W = L + 1 minima added newest first, the mean held
// to the gain of the frame that comes out, the delayed input times it, clamped.  binary32, every operation rounded on its own
// (-ffp-contract=off), the divisions correctly rounded, denormals kept, no atomics, no order that depends on timing.
//   s2r_limiter_kernel: one workgroup of S2R_LIMITER_BLOCK = 256 threads per 256 frames, one frame per thread, ONE launch per call.
//   With ge = gh followed by the call's g (ge[e] is g[e - G]) the workgroup at frame f0 keeps the window ge[f0 .. f0 + 256 + G) in
//   LDS: the history part read from the state, the call's part computed from float2 loads of x, entries past the call 1.0 (they
//   reach frames past the call only).  The minimum is a sparse table built by doubling between two LDS buffers — A_2q[j] =
//   min(A_q[j], A_q[j + q]) up to the largest power of two q <= K = L + H + 1, then m[j] = min(A_q[j], A_q[j + K - q]) for the
//   workgroup's 256 + L positions: a minimum is idempotent, so the two overlapping spans give the window's.  Every pass reads and
//   writes consecutive addresses per lane: no bank conflicts.  Each thread then adds its W minima from LDS in the rule's order.
//   The next state — the last G of ge and the last L of xh followed by x — is written by all workgroups in a grid-stride loop into
//   the copy of the state that nobody reads in this launch.  min s' and max |y| go through the 64-lane xor butterfly and LDS into
//   one row per workgroup; the host reduces the rows after the fill's synchronise (both are order-free).
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float lf2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kLimThreads = S2R_LIMITER_BLOCK;
static_assert(kLimThreads == 256, "the reduction below is a 64-lane butterfly and four waves");

__device__ __forceinline__ float lim_min(float a, float b) { return a < b ? a : b; }

// step 1 of the rule for one frame
__device__ __forceinline__ float lim_gain(const float *x, uint32_t n, float c) {
    const lf2 v = *reinterpret_cast<const lf2 *>(x + (size_t)n * 2u);
    const float al = __builtin_fabsf(v.x), ar = __builtin_fabsf(v.y);
    const float p = al > ar ? al : ar;
    return p > c ? c / p : 1.0f;
}

}  // namespace

__global__ void __launch_bounds__(kLimThreads) s2r_limiter_kernel(const S2rLimiter a) {
    extern __shared__ float s_win[];                             // two buffers of 256 + G floats
    __shared__ float s_mn[4], s_pk[4];
    const uint32_t L = a.lookahead, H = a.hold, G = 2u * L + H, K = L + H + 1u, len = kLimThreads + G;
    const uint32_t tid = threadIdx.x, f0 = blockIdx.x * kLimThreads, n = f0 + tid;
    const float c = a.ceiling;
    float *src = s_win, *dst = s_win + len;
    for (uint32_t w = tid; w < len; w += kLimThreads) {
        const uint32_t e = f0 + w;
        float g = 1.0f;
        if (e < G) g = a.gh[e];
        else if (e - G < a.frames) g = lim_gain(a.x, e - G, c);
        src[w] = g;
    }
    __syncthreads();
    const float gd = src[tid + L + H];                           // g[n - L]: the gain of the frame that comes out
    uint32_t q = 1u;
    for (; 2u * q <= K; q *= 2u) {
        const uint32_t cnt = len + 1u - 2u * q;                  // A_2q[j] spans 2q entries: j + 2q <= len
        for (uint32_t w = tid; w < cnt; w += kLimThreads) dst[w] = lim_min(src[w], src[w + q]);
        __syncthreads();
        float *t = src; src = dst; dst = t;
    }
    for (uint32_t j = tid; j < kLimThreads + L; j += kLimThreads) dst[j] = lim_min(src[j], src[j + (K - q)]);   // m[f0 - L + j]
    __syncthreads();
    float acc = 0.0f;
    {
        const float *mw = dst + tid + L;                         // m[n], and m[n - k] k entries below it
        for (uint32_t k = 0; k <= L; ++k) acc = acc + mw[-(int)k];
    }
    const float s = acc / (float)(L + 1u);
    const float sp = lim_min(s, gd);
    const bool in = n < a.frames;
    float mn = __builtin_inff(), pk = 0.0f;
    if (in) {
        // x[n - L]: from the state for the call's first L frames
        const lf2 xd = *reinterpret_cast<const lf2 *>(n < L ? a.xh + (size_t)n * 2u : a.x + (size_t)(n - L) * 2u);
        lf2 y = xd * (lf2){sp, sp};
        y.x = y.x < -c ? -c : y.x; y.x = y.x > c ? c : y.x;
        y.y = y.y < -c ? -c : y.y; y.y = y.y > c ? c : y.y;
        *reinterpret_cast<lf2 *>(a.out + (size_t)n * 2u) = y;
        const float al = __builtin_fabsf(y.x), ar = __builtin_fabsf(y.y);
        pk = al > ar ? al : ar;
        mn = sp;
    }
    // the state the call leaves: ge[N + i], i < G, and (xh followed by x)[N + i], i < L, into the copy nobody reads here
    {
        const uint32_t N = a.frames, total = gridDim.x * kLimThreads;
        for (uint32_t i = n; i < G; i += total) {
            const uint32_t e = N + i;
            a.gh_next[i] = e < G ? a.gh[e] : lim_gain(a.x, e - G, c);
        }
        for (uint32_t i = n; i < L; i += total) {
            const uint32_t e = N + i;
            *reinterpret_cast<lf2 *>(a.xh_next + (size_t)i * 2u) = *reinterpret_cast<const lf2 *>(e < L ? a.xh + (size_t)e * 2u : a.x + (size_t)(e - L) * 2u);
        }
    }
    const uint32_t wave = tid >> 6, lane = tid & 63u;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float m2 = __shfl_xor(mn, off, 64), p2 = __shfl_xor(pk, off, 64);
        mn = lim_min(mn, m2);
        pk = pk > p2 ? pk : p2;
    }
    if (lane == 0) { s_mn[wave] = mn; s_pk[wave] = pk; }
    __syncthreads();
    if (tid == 0) {
        const float m01 = lim_min(s_mn[0], s_mn[1]), m23 = lim_min(s_mn[2], s_mn[3]);
        const float p01 = s_pk[0] > s_pk[1] ? s_pk[0] : s_pk[1], p23 = s_pk[2] > s_pk[3] ? s_pk[2] : s_pk[3];
        float *row = a.partials + (size_t)blockIdx.x * 2u;
        row[0] = lim_min(m01, m23);
        row[1] = p01 > p23 ? p01 : p23;
    }
}

hipError_t s2r_launch_limiter(const S2rLimiter &a, hipStream_t stream) {
    if (a.frames == 0) return hipSuccess;
    if (a.lookahead == 0 || a.lookahead > S2R_LIMITER_MAX_LOOKAHEAD || a.hold > S2R_LIMITER_MAX_HOLD || !a.x || !a.out || !a.xh || !a.gh ||
        !a.xh_next || !a.gh_next || a.xh_next == a.xh || a.gh_next == a.gh || !a.partials)
        return hipErrorInvalidValue;
    const uint32_t len = kLimThreads + 2u * a.lookahead + a.hold;
    const dim3 grid((a.frames + kLimThreads - 1u) / kLimThreads), block(kLimThreads);
    hipLaunchKernelGGL(s2r_limiter_kernel, grid, block, (size_t)2u * len * sizeof(float), stream, a);   // at most 51 200 bytes
    return hipGetLastError();
}
