// s2r_delay.hip — the per-bus feedback delay of s2r_fill_buses and s2r_fill_master, in front of the bus reverbs:
//   t = W_c[n - D], u = W_(1-c)[n - D];   W_c[n] = (x_c[n] + feedback * t) + cross * u;   y_c[n] = (dry * x_c[n]) + (wet * t)
// binary32, every product and every sum rounded on its own (-ffp-contract=off), denormals kept, no add skipped for a zero
// coefficient.  Frames n and n' meet only when n = n' (mod D): one thread owns one residue r < D of one bus and carries BOTH
// channels of W in registers (the cross-feed takes the other channel at the same index, so nothing crosses lanes).  No LDS, no
// barrier, no atomics, nothing that waits for another workgroup.
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float dl2 __attribute__((ext_vector_type(2)));

constexpr int kDelayThreads = 256;
constexpr int kDelayAhead = 8;                                   // x pairs loaded ahead of the dependent chain in a long walk

// one frame of both channels: w is (W_L, W_R)[n - D] going in and (W_L, W_R)[n] coming out; returns (y_L, y_R)
__device__ __forceinline__ dl2 delay_step(const S2rDelayBus &b, const dl2 x, dl2 &w) {
    const float tl = w.x, tr = w.y;
    const float pl = b.feedback * tl, pr = b.feedback * tr;     // p = feedback * t
    const float ql = b.cross * tr, qr = b.cross * tl;           // q = cross * u
    const float sl = x.x + pl, sr = x.y + pr;                   // s = x + p
    w = (dl2){sl + ql, sr + qr};                                 // W = s + q
    const float dl = b.dry * x.x, dr = b.dry * x.y;
    const float wl = b.wet * tl, wr = b.wet * tr;
    return (dl2){dl + wl, dr + wr};
}

}  // namespace

// Workgroups (k, bus).  A bus with a delay: thread r < D starts from the history's frame r (which is W[r - D]), walks n = r, r + D,
// ... < N — one interleaved x pair in, one y pair out per step, 8 bytes each, coalesced along r; in a walk of many steps the loads of
// kDelayAhead steps are issued before the chain that consumes them, so that a step costs its two products and two sums and not a
// memory round trip — and leaves what it holds at the end in frame n - N of the OTHER line, n being the first index past the call:
// the last D of (history, W[0 .. N)).  A thread that made no step (r >= N, a call shorter than the delay) thereby moves its
// history frame N places towards the front: the untouched tail.  A bus without a delay is copied from `in` to `out`.
__global__ void __launch_bounds__(kDelayThreads) s2r_delay_kernel(const S2rDelay a) {
    const uint32_t q = blockIdx.y;
    const S2rDelayBus &b = a.bus[q];
    const uint64_t i = (uint64_t)blockIdx.x * kDelayThreads + threadIdx.x, N = a.frames, D = b.delay;
    const dl2 *x = reinterpret_cast<const dl2 *>(a.in) + (uint64_t)q * N;
    dl2 *y = reinterpret_cast<dl2 *>(a.out) + (uint64_t)q * N;
    if (D == 0) {                                                // (uniform: the whole workgroup)
        for (uint64_t n = i; n < N; n += (uint64_t)gridDim.x * kDelayThreads) y[n] = x[n];
        return;
    }
    if (i >= D) return;
    dl2 w = reinterpret_cast<const dl2 *>(b.line)[i];
    uint64_t n = i;
    while (n + (uint64_t)(kDelayAhead - 1) * D < N) {
        dl2 ahead[kDelayAhead];
#pragma unroll
        for (int j = 0; j < kDelayAhead; ++j) ahead[j] = x[n + (uint64_t)j * D];
#pragma unroll
        for (int j = 0; j < kDelayAhead; ++j) y[n + (uint64_t)j * D] = delay_step(b, ahead[j], w);
        n += (uint64_t)kDelayAhead * D;
    }
    for (; n < N; n += D) y[n] = delay_step(b, x[n], w);
    reinterpret_cast<dl2 *>(b.next)[n - N] = w;                  // (n - D < N <= n: a frame of the line, and every one of them is written once)
}

hipError_t s2r_launch_bus_delay(const S2rDelay &a, hipStream_t stream) {
    if (a.frames == 0 || a.n_buses == 0) return hipSuccess;
    if (a.n_buses > S2R_MAX_BUSES || !a.in || !a.out || a.in == a.out) return hipErrorInvalidValue;
    uint32_t span = 0;
    for (uint32_t q = 0; q < a.n_buses; q++) {
        const S2rDelayBus &b = a.bus[q];
        if (b.delay == 0) continue;
        if (b.delay > S2R_MAX_DELAY_FRAMES || !b.line || !b.next || b.line == b.next) return hipErrorInvalidValue;
        if (b.delay > span) span = b.delay;
    }
    if (span == 0) return hipErrorInvalidValue;                  // (a call without a delay does not come here)
    hipLaunchKernelGGL(s2r_delay_kernel, dim3((span + kDelayThreads - 1u) / kDelayThreads, a.n_buses), dim3(kDelayThreads), 0, stream, a);
    return hipGetLastError();
}
