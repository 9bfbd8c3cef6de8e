// s2r_drive.hip — the per-bus drive of s2r_fill_buses and s2r_fill_master, behind the dynamics in the post-mix chain:
// an oversampled waveshaper.  Per frame n of a bus and channel c (x: the bus as it enters, negative indices its history):
//   m = 4 q + p:  u[m] = sum over j, p + 4 j <= 64, of (g[p + 4 j] * x[q - j]);   w[m] = the table at pre * u[m] (drive_shape below)
//   v[n] = sum over k = 0..64 of (h[k] * w[4 n - k]);   out[n] = (dry * x[n - 16]) + (wet * v[n])
// binary32, every operation rounded on its own (-ffp-contract=off), every sum from +0.0 in index order, denormals kept, nothing skipped
// for a zero.  The stage is feed-forward: a frame depends on 33 input frames and on nothing the stage wrote, so the call spreads over
// (tiles of S2R_DRIVE_TILE = 240 frames) x (buses) workgroups of 256 lanes, none of which waits for another.  A workgroup stages in LDS,
// per channel, its tile's input x[t0 - 32 .. t0 + 240) — from the state where the index is negative — and the bus's table.  Phase 1:
// lane l owns frame q = t0 - 16 + l — the tile and the 16 frames in front of it, 256 in all — and computes its four phases w[4 q + p]
// from x[q - 16 .. q], read at stride 1 across lanes, into one of FOUR PHASE PLANES W_p[q].  Barrier.  Phase 2: lane l < 240 owns output
// frame n = t0 + l and walks k = 0..64 in order; w[4 n - k] is W_(-k mod 4)[n - ceil(k / 4)], again stride 1 across lanes: ds_read_b32
// has 32 banks, and an interleaved w[] read at 4 n - k would put lanes l and l + 8 on one bank, a 4-way conflict on each of the 65
// reads (-DS2R_DRIVE_INTERLEAVED builds that form, to be timed once: tools/drive_time.py).  The taps are wave-uniform and arrive in the
// kernel's arguments, which the compiler reads with scalar loads; with both loops unrolled every tap is a register operand — the
// first 33 of each filter only, the taps being symmetric on bits, so that both filters fit the scalar registers without a spill.  The last
// tile may be partial: a lane past the call loads nothing and writes nothing.  The workgroup of tile 0 writes the next state, the last
// 32 frames of history ++ call, into the state's other copy.  Each value sees exactly the rule's operations in the rule's order, so the
// output is the host loop's bit for bit.  Buses of the call without a drive are copied by their workgroups of the same launch.  No
// atomics, no inline assembly.
// -DS2R_DRIVE_SERIAL builds the obvious form for comparison (tools/drive_time.py, CHANGELOG): one lane per output frame recomputes its
// own 65 w from global memory, with no LDS.
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float drv2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kDrvThreads = 256u;
constexpr uint32_t kDrvTile = S2R_DRIVE_TILE;
constexpr uint32_t kDrvLat = S2R_DRIVE_LATENCY, kDrvHist = S2R_DRIVE_HISTORY, kDrvTaps = S2R_DRIVE_TAPS;
constexpr uint32_t kDrvX = kDrvTile + kDrvHist;                  // input frames a tile reads, per channel
constexpr uint32_t kDrvW = kDrvTile + kDrvLat;                   // frames whose four phases a tile computes, per channel
static_assert(kDrvW == kDrvThreads && kDrvTaps == 4u * kDrvLat + 1u && kDrvHist == 2u * kDrvLat, "a frame per lane in phase 1; 65 taps are 16 frames of delay twice over");

// where w[4 f + p] of frame f (counted from t0 - 16) sits in a channel's 4 * kDrvW floats
__device__ __forceinline__ uint32_t drive_w_at(const uint32_t p, const uint32_t f) {
#ifdef S2R_DRIVE_INTERLEAVED
    return 4u * f + p;
#else
    return p * kDrvW + f;
#endif
}

// tap k of a filter given by its first half and its centre
__device__ __forceinline__ float drive_tap(const float (&half)[S2R_DRIVE_HALF_TAPS], const uint32_t k) { return half[k < S2R_DRIVE_HALF_TAPS ? k : kDrvTaps - 1u - k]; }

// the rule's second to fourth lines: one oversampled sample through the table, by sign and magnitude (s2r_rules.h: drive_shape)
__device__ __forceinline__ float drive_shape(const float *curve, const float pre, const float u) {
    const float t = pre * u;
    const float at = __builtin_fabsf(t);
    const float m = at < 1.0f ? at : 1.0f;
    const float a = m * 512.0f;
    const uint32_t ia = (uint32_t)a;
    const uint32_t i = ia < 511u ? ia : 511u;
    const float fr = a - (float)i;
    const bool neg = t < 0.0f;
    const float c0 = curve[neg ? 512u - i : 512u + i], c1 = curve[neg ? 511u - i : 513u + i];
    const float d = c1 - c0;
    const float e = fr * d;
    return c0 + e;
}

}  // namespace

// Workgroup (g, q) computes frames [240 g, 240 g + 240) of bus q, or copies them when the bus carries no drive.
__global__ void __launch_bounds__(kDrvThreads) s2r_drive_kernel(const S2rDrive a) {
    const uint32_t tid = threadIdx.x, N = a.frames, q = blockIdx.y, t0 = blockIdx.x * kDrvTile;
    const S2rDriveBus &b = a.bus[q];
    const drv2 *const x2 = reinterpret_cast<const drv2 *>(a.in) + (uint64_t)q * N;
    drv2 *const y2 = reinterpret_cast<drv2 *>(a.out) + (uint64_t)q * N;
    const uint32_t n = t0 + tid;
    const bool mine = tid < kDrvTile && n < N;                   // this lane has an output frame
    if (!b.curve) {                                              // (uniform: the whole workgroup)
        if (mine) y2[n] = x2[n];
        return;
    }
    const drv2 *const hist = reinterpret_cast<const drv2 *>(b.line);
    const float pre = b.pre, dry = b.dry, wet = b.wet;
    if (blockIdx.x == 0 && tid < kDrvHist) {                     // the next state: from the old one as far as the call did not reach
        const uint32_t at = N + tid;                             // frame N - 32 + tid of the call is entry `at` of history ++ call
        reinterpret_cast<drv2 *>(b.next)[tid] = at < kDrvHist ? hist[at] : x2[at - kDrvHist];
    }
#ifdef S2R_DRIVE_SERIAL
    if (!mine) return;
    float o[2];
    for (uint32_t c = 0; c < 2u; c++) {
        float v = 0.0f;
        for (uint32_t k = 0; k < kDrvTaps; k++) {
            const uint32_t ck = (k + 3u) / 4u, p = 4u * ck - k;  // w[4 n - k] is phase p of frame n - ck
            const int32_t f = (int32_t)n - (int32_t)ck;
            float u = 0.0f;
            for (uint32_t j = 0; p + 4u * j < kDrvTaps; j++) {
                const int32_t fx = f - (int32_t)j;               // >= -32
                const float x = fx < 0 ? b.line[2 * (fx + (int32_t)kDrvHist) + (int32_t)c] : a.in[((uint64_t)q * N + (uint32_t)fx) * 2u + c];
                const float t = drive_tap(a.g, p + 4u * j) * x;
                u = u + t;
            }
            const float t = drive_tap(a.h, k) * drive_shape(b.curve, pre, u);
            v = v + t;
        }
        const int32_t fd = (int32_t)n - (int32_t)kDrvLat;
        const float x = fd < 0 ? b.line[2 * (fd + (int32_t)kDrvHist) + (int32_t)c] : a.in[((uint64_t)q * N + (uint32_t)fd) * 2u + c];
        const float d = dry * x;
        const float e = wet * v;
        o[c] = d + e;
    }
    y2[n] = drv2{o[0], o[1]};
#else
    __shared__ float sx[2][kDrvX];                               // x[t0 - 32 + i] at i
    __shared__ float sc[S2R_DRIVE_CURVE_POINTS + 3u];
    __shared__ float sw[2][4u * kDrvW];                          // the phase planes (drive_w_at)
    for (uint32_t i = tid; i < kDrvX; i += kDrvThreads) {
        const uint32_t at = t0 + i;                              // entry `at` of history ++ call
        drv2 x = drv2{0.0f, 0.0f};
        if (at < kDrvHist) x = hist[at];
        else if (at - kDrvHist < N) x = x2[at - kDrvHist];
        sx[0][i] = x.x; sx[1][i] = x.y;
    }
    for (uint32_t j = tid; j < S2R_DRIVE_CURVE_POINTS; j += kDrvThreads) sc[j] = b.curve[j];
    __syncthreads();
    // phase 1: frame t0 - 16 + tid, whose x[q - j] sits at tid + 16 - j
    if (t0 + tid < N + kDrvLat) {
        float xv[2][kDrvLat + 1u];
#pragma unroll
        for (uint32_t j = 0; j <= kDrvLat; j++) { xv[0][j] = sx[0][tid + kDrvLat - j]; xv[1][j] = sx[1][tid + kDrvLat - j]; }
#pragma unroll
        for (uint32_t p = 0; p < S2R_DRIVE_OVERSAMPLE; p++) {
#pragma unroll
            for (uint32_t c = 0; c < 2u; c++) {                  // (inside: a tap serves both channels)
                float u = 0.0f;
#pragma unroll
                for (uint32_t j = 0; p + 4u * j < kDrvTaps; j++) {
                    const float t = drive_tap(a.g, p + 4u * j) * xv[c][j];
                    u = u + t;
                }
                sw[c][drive_w_at(p, tid)] = drive_shape(sc, pre, u);
            }
        }
    }
    __syncthreads();
    // phase 2: frame t0 + tid, whose w[4 n - k] is phase -k mod 4 of the frame ceil(k / 4) in front of it
    if (!mine) return;
    float v[2] = {0.0f, 0.0f}, o[2];
#pragma unroll
    for (uint32_t k = 0; k < kDrvTaps; k++) {
        const uint32_t ck = (k + 3u) / 4u, p = 4u * ck - k;
#pragma unroll
        for (uint32_t c = 0; c < 2u; c++) {
            const float t = drive_tap(a.h, k) * sw[c][drive_w_at(p, tid + kDrvLat - ck)];
            v[c] = v[c] + t;
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < 2u; c++) {
        const float d = dry * sx[c][tid + kDrvLat];              // x[n - 16]
        const float e = wet * v[c];
        o[c] = d + e;
    }
    y2[n] = drv2{o[0], o[1]};
#endif
}

hipError_t s2r_launch_bus_drive(const S2rDrive &a, hipStream_t stream) {
    if (a.frames == 0 || a.n_buses == 0) return hipSuccess;
    if (a.n_buses > S2R_MAX_BUSES || !a.in || !a.out || a.in == a.out) return hipErrorInvalidValue;
    uint32_t active = 0;
    for (uint32_t q = 0; q < a.n_buses; q++) {
        const S2rDriveBus &b = a.bus[q];
        if (!b.curve) continue;
        if (!b.line || !b.next || b.line == b.next) return hipErrorInvalidValue;
        active++;
    }
    if (active == 0) return hipErrorInvalidValue;                // (a call without a drive does not come here)
    const dim3 grid((a.frames + kDrvTile - 1u) / kDrvTile, a.n_buses);
    hipLaunchKernelGGL(s2r_drive_kernel, grid, dim3(kDrvThreads), 0, stream, a);
    return hipGetLastError();
}
