// s2r_limiter_tp.hip — the master limiter with its true-peak detector: s2r_limiter.hip's kernel with step 1 of the rule
// replaced — the magnitude of a frame is the largest of |x[n - 8]| and the four phases of the drive's interpolator g = 4 h over
// x[n - 16 .. n], both channels, the operation sequence of the loudness meter's true peak (s2r_loudness.hip) — and the output taken 8
// frames further back, x[n - L - 8].  binary32, every operation rounded on its own (-ffp-contract=off), the divisions correctly
// rounded, denormals kept, no atomics, no order that depends on timing.
//   s2r_limiter_tp_kernel: one workgroup of 256 threads per 256 frames, one frame per thread, ONE launch per call.  As there, the
//   workgroup at frame f0 keeps ge[f0 .. f0 + 256 + G) in LDS, ge = gh followed by the call's g.  The call's part of that window, frames
//   [lo, hi) of the call, now costs eight sums of 16 or 17 products a gain, so the input it is computed from — frames [lo - 16, hi), the
//   first of them from xh — is staged in LDS first, a float2 per frame, and each thread computes the gains lo + tid, lo + tid + 256, ...
//   from seventeen consecutive frames of it: lanes read consecutive 8-byte slots (stride 1, no bank conflict), the taps are kernel
//   arguments at constant indices (scalar registers).  Every workgroup computes its own window's gains: a call of N frames with G >= N
//   computes N (N / 256 + 1) / 2 gains instead of N, which at the largest G and 1024 frames is 2560 gains of 264 products — less
//   than a launch in front would cost (DESIGN.md 4.30 has the timings).  Minimum, sum, output and meter partials are s2r_limiter.hip's.
//   The next gh is written by the LAST workgroup, whose window holds all of it, from LDS; the next xh by all in a grid-stride loop;
//   both into the copy of the state that nobody reads in this launch.
// -DS2R_LIMITER_TP_NAIVE builds the form one would write first, for comparison (tools/limiter_time.py --true-peak, CHANGELOG): no
// input window, each thread sums its gains straight from global memory.  Never the product build.
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float tf2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kTpThreads = S2R_LIMITER_BLOCK;
constexpr uint32_t kTpHist = S2R_LIMITER_TP_HISTORY, kTpLat = S2R_LIMITER_TP_LATENCY;
constexpr uint32_t kTpMaxLen = kTpThreads + 2u * S2R_LIMITER_MAX_LOOKAHEAD + S2R_LIMITER_MAX_HOLD;
static_assert(kTpThreads == 256, "the reduction below is a 64-lane butterfly and four waves");
static_assert(4u * kTpHist + 1u == S2R_DRIVE_TAPS && 2u * kTpLat == kTpHist && S2R_DRIVE_OVERSAMPLE == 4u, "the interpolator of s2r.h: 65 taps, four phases, centred 8 frames back");
static_assert(sizeof(S2rLimiterTp::g) == (2u * kTpHist + 1u) * sizeof(float), "half of the taps, the centre included");

// the bytes of dynamic LDS: two buffers of len gains, then len + 16 input frames
constexpr size_t tp_lds(uint32_t len) { return (size_t)2u * len * sizeof(float) + (size_t)(len + kTpHist) * sizeof(tf2); }
static_assert(tp_lds(kTpMaxLen) <= 160u * 1024u, "one workgroup's LDS");

__device__ __forceinline__ float tp_min(float a, float b) { return a < b ? a : b; }

// frame q of the limiter's input, q >= -(L + 16): from the state in front of the call
__device__ __forceinline__ tf2 tp_frame(const S2rLimiter &l, int32_t q) {
    return *reinterpret_cast<const tf2 *>(q < 0 ? l.xh + (size_t)((int32_t)(l.lookahead + kTpHist) + q) * 2u : l.x + (size_t)q * 2u);
}

// tap k of g, 0 .. 64, from the half the arguments carry
__device__ __forceinline__ float tp_tap(const S2rLimiterTp &a, const uint32_t k) { return a.g[k <= 2u * kTpHist ? k : S2R_DRIVE_TAPS - 1u - k]; }

// step 1' of the rule for one frame n from x[n - j] at x[j], j = 0 .. 16
__device__ __forceinline__ float tp_gain(const S2rLimiterTp &a, const tf2 (&x)[kTpHist + 1u], const float c) {
    const float al = __builtin_fabsf(x[kTpLat].x), ar = __builtin_fabsf(x[kTpLat].y);
    float d = al > ar ? al : ar;
#pragma unroll
    for (uint32_t p = 0; p < S2R_DRIVE_OVERSAMPLE; p++) {
        tf2 u = tf2{0.0f, 0.0f};
#pragma unroll
        for (uint32_t j = 0; p + 4u * j < S2R_DRIVE_TAPS; j++) {
            const float g = tp_tap(a, p + 4u * j);
            const tf2 t = tf2{g, g} * x[j];
            u = u + t;
        }
        const float ul = __builtin_fabsf(u.x), ur = __builtin_fabsf(u.y);
        d = ul > d ? ul : d; d = ur > d ? ur : d;
    }
    return d > c ? c / d : 1.0f;
}

}  // namespace

__global__ void __launch_bounds__(kTpThreads) s2r_limiter_tp_kernel(const S2rLimiterTp a) {
    extern __shared__ __attribute__((aligned(16))) float s_tp[];      // two buffers of 256 + G gains, then 256 + G + 16 input frames
    __shared__ float s_mn[4], s_pk[4];
    const S2rLimiter &l = a.l;
    const uint32_t L = l.lookahead, H = l.hold, G = 2u * L + H, K = L + H + 1u, len = kTpThreads + G, N = l.frames;
    const uint32_t tid = threadIdx.x, f0 = blockIdx.x * kTpThreads, n = f0 + tid;
    const float c = l.ceiling;
    float *src = s_tp, *dst = s_tp + len;
    // the call's frames whose gains the window holds: entry w is ge[f0 + w], frame f0 + w - G of the call
    const uint32_t lo = f0 > G ? f0 - G : 0u, hi = f0 + kTpThreads < N ? f0 + kTpThreads : N, cnt = hi - lo;      // (lo < hi: f0 < N)
    const uint32_t w0 = lo + G - f0;                             // the entry of frame lo
    for (uint32_t w = tid; w < len; w += kTpThreads)             // the history in front of them, 1.0 behind (they reach frames past the call only)
        if (w < w0 || w >= w0 + cnt) src[w] = f0 + w < G ? l.gh[f0 + w] : 1.0f;
#ifndef S2R_LIMITER_TP_NAIVE
    tf2 *const xw = reinterpret_cast<tf2 *>(s_tp + 2u * len);    // frame lo - 16 + i of the input at i
    for (uint32_t i = tid; i < cnt + kTpHist; i += kTpThreads) xw[i] = tp_frame(l, (int32_t)(lo + i) - (int32_t)kTpHist);
    __syncthreads();
#endif
    for (uint32_t i = tid; i < cnt; i += kTpThreads) {
        tf2 x[kTpHist + 1u];                                     // x[lo + i - j] at j
#ifdef S2R_LIMITER_TP_NAIVE
#pragma unroll
        for (uint32_t j = 0; j <= kTpHist; j++) x[j] = tp_frame(l, (int32_t)(lo + i) - (int32_t)j);
#else
#pragma unroll
        for (uint32_t j = 0; j <= kTpHist; j++) x[j] = xw[i + kTpHist - j];
#endif
        src[w0 + i] = tp_gain(a, x, c);
    }
    __syncthreads();
    const float gd = src[tid + L + H];                           // g[n - L]: the gain of the frame that comes out
    // the gains the call leaves, ge[N + i], i < G: all in the last workgroup's window
    if (blockIdx.x == gridDim.x - 1u)
        for (uint32_t i = tid; i < G; i += kTpThreads) l.gh_next[i] = src[N + i - f0];
    uint32_t q = 1u;
    for (; 2u * q <= K; q *= 2u) {
        const uint32_t m = len + 1u - 2u * q;                    // A_2q[j] spans 2q entries: j + 2q <= len
        for (uint32_t w = tid; w < m; w += kTpThreads) dst[w] = tp_min(src[w], src[w + q]);
        __syncthreads();
        float *t = src; src = dst; dst = t;
    }
    for (uint32_t j = tid; j < kTpThreads + L; j += kTpThreads) dst[j] = tp_min(src[j], src[j + (K - q)]);      // m[f0 - L + j]
    __syncthreads();
    float acc = 0.0f;
    {
        const float *mw = dst + tid + L;                         // m[n], and m[n - k] k entries below it
        for (uint32_t k = 0; k <= L; ++k) acc = acc + mw[-(int)k];
    }
    const float s = acc / (float)(L + 1u);
    const float sp = tp_min(s, gd);
    float mn = __builtin_inff(), pk = 0.0f;
    if (n < N) {
        const tf2 xd = tp_frame(l, (int32_t)n - (int32_t)(L + kTpLat));        // x[n - L - 8]
        tf2 y = xd * (tf2){sp, sp};
        y.x = y.x < -c ? -c : y.x; y.x = y.x > c ? c : y.x;
        y.y = y.y < -c ? -c : y.y; y.y = y.y > c ? c : y.y;
        *reinterpret_cast<tf2 *>(l.out + (size_t)n * 2u) = y;
        const float al = __builtin_fabsf(y.x), ar = __builtin_fabsf(y.y);
        pk = al > ar ? al : ar;
        mn = sp;
    }
    // the input frames the call leaves: (xh followed by x)[N + i], i < L + 16, into the copy nobody reads here
    {
        const uint32_t X = L + kTpHist, total = gridDim.x * kTpThreads;
        for (uint32_t i = n; i < X; i += total)
            *reinterpret_cast<tf2 *>(l.xh_next + (size_t)i * 2u) = tp_frame(l, (int32_t)(N + i) - (int32_t)X);
    }
    const uint32_t wave = tid >> 6, lane = tid & 63u;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float m2 = __shfl_xor(mn, off, 64), p2 = __shfl_xor(pk, off, 64);
        mn = tp_min(mn, m2);
        pk = pk > p2 ? pk : p2;
    }
    if (lane == 0) { s_mn[wave] = mn; s_pk[wave] = pk; }
    __syncthreads();
    if (tid == 0) {
        const float m01 = tp_min(s_mn[0], s_mn[1]), m23 = tp_min(s_mn[2], s_mn[3]);
        const float p01 = s_pk[0] > s_pk[1] ? s_pk[0] : s_pk[1], p23 = s_pk[2] > s_pk[3] ? s_pk[2] : s_pk[3];
        float *row = l.partials + (size_t)blockIdx.x * 2u;
        row[0] = tp_min(m01, m23);
        row[1] = p01 > p23 ? p01 : p23;
    }
}

hipError_t s2r_launch_limiter_tp(const S2rLimiterTp &a, hipStream_t stream) {
    const S2rLimiter &l = a.l;
    if (l.frames == 0) return hipSuccess;
    if (l.lookahead == 0 || l.lookahead > S2R_LIMITER_MAX_LOOKAHEAD || l.hold > S2R_LIMITER_MAX_HOLD || !l.x || !l.out || !l.xh || !l.gh ||
        !l.xh_next || !l.gh_next || l.xh_next == l.xh || l.gh_next == l.gh || !l.partials)
        return hipErrorInvalidValue;
    const uint32_t len = kTpThreads + 2u * l.lookahead + l.hold;
    const size_t lds = tp_lds(len);                              // at most 102 528 bytes
    if (lds > 64u * 1024u) {                                     // (more dynamic LDS than a launch gets unasked, on the current device)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(s2r_limiter_tp_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tp_lds(kTpMaxLen));
        if (e != hipSuccess) return e;
    }
    const dim3 grid((l.frames + kTpThreads - 1u) / kTpThreads), block(kTpThreads);
    hipLaunchKernelGGL(s2r_limiter_tp_kernel, grid, block, lds, stream, a);
    return hipGetLastError();
}
