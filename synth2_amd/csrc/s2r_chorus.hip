// s2r_chorus.hip — the per-bus chorus of s2r_fill_buses and s2r_fill_master, in front of the bus delays: V taps into
// the history of the INPUT at delays d = base + depth * m, m a triangle of an integer phase, each tap the linear interpolation
// a + f * (bb - a) of two neighbours, added in voice order:   y_c[n] = (dry * x_c[n]) + (wet * acc)
// binary32, every product and every sum rounded on its own (-ffp-contract=off), denormals kept, nothing skipped for a zero coefficient
// or for f == 0.  No recursion: a frame's output is a function of the input alone, so one thread owns one frame, both channels and
// all V voices, and the LFO's phase is integer arithmetic on the frame index — nothing is carried from lane to lane.  No LDS, no
// barrier, no atomics, nothing that waits for another workgroup.
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float ch2 __attribute__((ext_vector_type(2)));

constexpr int kChorusThreads = 256;

// x_c[j] of the stream (history, then the call's input): j in [-H, N)
__device__ __forceinline__ float chorus_x(const float *x, const float *line, const int64_t H, const int64_t j, const uint32_t c) {
    return j >= 0 ? x[2 * j + c] : line[2 * (H + j) + c];
}

}  // namespace

// Workgroups (tile, bus), thread t of the tile's 256 frames.  A bus with a chorus: thread t < H stores frame t of the next history —
// frame t + N of (history, x[0 .. N)), the last H of it: in a call shorter than H old history moves to the front — and thread t < N
// computes y[t].  Neighbouring frames read neighbouring addresses (the delay moves by a fraction of a frame per frame), so the taps
// are plain global loads: from `in` where n - i >= 0 and from the history line below it.  A bus without a chorus is copied from `in`
// to `out`.
__global__ void __launch_bounds__(kChorusThreads) s2r_chorus_kernel(const S2rChorus a) {
    const uint32_t q = blockIdx.y;
    const S2rChorusBus &b = a.bus[q];
    const uint32_t t = blockIdx.x * kChorusThreads + threadIdx.x, N = a.frames, H = b.history;
    const ch2 *x2 = reinterpret_cast<const ch2 *>(a.in) + (uint64_t)q * N;
    ch2 *y2 = reinterpret_cast<ch2 *>(a.out) + (uint64_t)q * N;
    if (b.voices == 0) {                                         // (uniform: the whole workgroup)
        if (t < N) y2[t] = x2[t];
        return;
    }
    if (t < H) {                                                 // every frame of the next line, once
        const uint64_t s = (uint64_t)t + N;
        reinterpret_cast<ch2 *>(b.next)[t] = s < H ? reinterpret_cast<const ch2 *>(b.line)[s] : x2[s - H];
    }
    if (t >= N) return;
    const float *x = reinterpret_cast<const float *>(x2);
    const ch2 xn = x2[t];
    const uint32_t p0 = b.phase + b.phase_inc * t;              // (mod 2^32)
    float y[2];
#pragma unroll
    for (uint32_t c = 0; c < 2; c++) {
        float acc = 0.0f;
        for (uint32_t v = 0; v < b.voices; v++) {
            const uint32_t p = p0 + b.off[v] + c * b.spread;
            const uint32_t k = p >> 8;
            const uint32_t h = k < (1u << 23) ? k : (1u << 24) - k;
            const float m = (float)h * 0x1p-23f;                 // exact
            const float dm = b.depth * m;
            const float d = b.base + dm;
            uint32_t i = (uint32_t)d;                            // i <= H - 1 by monotonic rounding ...
            i = i < H - 1u ? i : H - 1u;                         // ... and no load leaves the line whatever a caller of the launcher passes
            const float f = d - (float)i;
            const int64_t j = (int64_t)t - (int64_t)i;
            const float ta = chorus_x(x, b.line, H, j, c), tb = chorus_x(x, b.line, H, j - 1, c);
            const float e = tb - ta;
            const float g = f * e;
            const float tap = ta + g;
            acc = v ? acc + tap : tap;
        }
        const float dx = b.dry * (c ? xn.y : xn.x), wa = b.wet * acc;
        y[c] = dx + wa;
    }
    y2[t] = (ch2){y[0], y[1]};
}

hipError_t s2r_launch_bus_chorus(const S2rChorus &a, hipStream_t stream) {
    if (a.frames == 0 || a.n_buses == 0) return hipSuccess;
    if (a.n_buses > S2R_MAX_BUSES || !a.in || !a.out || a.in == a.out) return hipErrorInvalidValue;
    uint32_t span = 0;
    for (uint32_t q = 0; q < a.n_buses; q++) {
        const S2rChorusBus &b = a.bus[q];
        if (b.voices == 0) continue;
        if (b.voices > S2R_CHORUS_MAX_VOICES || b.history < 2u || b.history > (uint32_t)S2R_CHORUS_MAX_DELAY + 1u || !b.line || !b.next || b.line == b.next)
            return hipErrorInvalidValue;
        if (b.history > span) span = b.history;
    }
    if (span == 0) return hipErrorInvalidValue;                  // (a call without a chorus does not come here)
    if (a.frames > span) span = a.frames;
    hipLaunchKernelGGL(s2r_chorus_kernel, dim3((span + kChorusThreads - 1u) / kChorusThreads, a.n_buses), dim3(kChorusThreads), 0, stream, a);
    return hipGetLastError();
}
