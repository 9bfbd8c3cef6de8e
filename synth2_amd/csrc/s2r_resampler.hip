// s2r_resampler.hip — the sample-rate converter behind the spectrum meters of s2r_fill_master.  Per channel q of
// the 18 (bus b at 2 b, 2 b + 1, the master at 16, 17) and output frame i < count of the call:
//   u = ph + i * M;   n = u / L;   p = u % L;   a_(k % 4) += h[p][k] * x[n - k] for k = 0 .. T - 1 ascending, each a from +0.0;
//   y[i] = (a_0 + a_1) + (a_2 + a_3)
// x[n] with n < 0 the history, newest first.  binary32, every operation rounded on its own (-ffp-contract=off), denormals kept, no
// atomics, no order that depends on timing: every output frame is one lane's, start to end.
//   s2r_resampler_kernel, ONE launch per call, workgroups of one wave.  Workgroup (programme, tile) makes S2R_RESAMPLER_TILE = 64 output
//   frames of one programme, a lane each, both channels in one lane through the four chains.  It first stages in LDS, with coalesced
//   loads, the tile's input span — the frames n - (T - 1) of its first output to n of its last, history included, a float2 each: at
//   most ceil(63 M / L) + T frames — and the tile's table rows, row (p_0 + j M) mod L for lane j into slot j on a stride of T + 1
//   floats: T is a multiple of 4, so the stride is odd and the 64 lanes, each reading its own slot at the same k, hit distinct banks.
//   A table of at most 64 rows is staged whole instead, row r in slot r, in a loop of its own: fewer loads, and the lanes of one phase
//   read one address.
//   The loop then reads LDS alone: one float and one float2 a tap.  The workgroup behind the tiles writes the next state into the
//   copy nobody reads in this launch; the workgroups behind that copy the master to the pinned output when no meter kernel has.
// -DS2R_RESAMPLER_SERIAL builds the obvious form for comparison (tools/resampler_time.py, CHANGELOG): the same grid, and every lane
// reads its table row and its T input frames from global memory.
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float rs2 __attribute__((ext_vector_type(2)));
typedef float rs4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kRsTile = S2R_RESAMPLER_TILE;
constexpr uint32_t kRsThreads = 64u;
constexpr uint32_t kRsRow = S2R_RESAMPLER_MAX_TAPS + 1u;         // the largest stride of a slot
constexpr uint32_t kRsSpan = (kRsTile - 1u) * 4u + S2R_RESAMPLER_MAX_TAPS + 4u;     // ceil(63 M / L) + T frames at M = 4 L, T = 128, and room to spare
static_assert(kRsTile == kRsThreads, "a lane per output frame of a tile");
static_assert((kRsTile * kRsRow + 2u * kRsSpan) * 4u <= 64u * 1024u, "the slots and the span fit the LDS a launch gets unasked");
static_assert(S2R_RESAMPLER_PROGRAMMES == S2R_MAX_BUSES + 1u && S2R_RESAMPLER_CHANNELS == 2u * S2R_RESAMPLER_PROGRAMMES, "s2r.h's programmes");

// frame n of programme p: of the call for n >= 0 (a bus past the call's: +0.0), of the history, newest first, for n < 0 (n >= -(T - 1))
__device__ __forceinline__ rs2 rs_frame(const S2rResampler &a, const uint32_t p, const int32_t n) {
    if (n < 0) {
        const uint32_t H = a.T - 1u, j = (uint32_t)(-n - 1);
        return rs2{a.state[(2u * p) * H + j], a.state[(2u * p + 1u) * H + j]};
    }
    if (p == S2R_MAX_BUSES) return reinterpret_cast<const rs2 *>(a.master)[n];
    if (p < a.n_buses) return *reinterpret_cast<const rs2 *>(a.stems + ((size_t)p * a.frames + (uint32_t)n) * 2u);
    return rs2{0.0f, 0.0f};
}

// the rule's steps 3 and 4 for both channels: h[k] the row's taps, x[-k] the frame k in front of the output's frame n
template <class Taps, class Frames> __device__ __forceinline__ rs2 rs_sum(const uint32_t T, const Taps h, const Frames x) {
    rs2 a0 = rs2{0.0f, 0.0f}, a1 = a0, a2 = a0, a3 = a0;
    for (uint32_t k = 0; k < T; k += 4u) {
        const float h0 = h(k), h1 = h(k + 1u), h2 = h(k + 2u), h3 = h(k + 3u);
        const rs2 x0 = x(k), x1 = x(k + 1u), x2 = x(k + 2u), x3 = x(k + 3u);
        const rs2 t0 = rs2{h0 * x0.x, h0 * x0.y}, t1 = rs2{h1 * x1.x, h1 * x1.y}, t2 = rs2{h2 * x2.x, h2 * x2.y}, t3 = rs2{h3 * x3.x, h3 * x3.y};
        a0 = rs2{a0.x + t0.x, a0.y + t0.y}; a1 = rs2{a1.x + t1.x, a1.y + t1.y};
        a2 = rs2{a2.x + t2.x, a2.y + t2.y}; a3 = rs2{a3.x + t3.x, a3.y + t3.y};
    }
    const rs2 lo = rs2{a0.x + a1.x, a0.y + a1.y}, hi = rs2{a2.x + a3.x, a2.y + a3.y};
    return rs2{lo.x + hi.x, lo.y + hi.y};
}

}  // namespace

__global__ void __launch_bounds__(kRsThreads) s2r_resampler_kernel(const S2rResampler a) {
    const uint32_t tid = threadIdx.x, T = a.T, H = T - 1u, F = a.frames;
    const uint32_t tiles = (a.count + kRsTile - 1u) / kRsTile, work = S2R_RESAMPLER_PROGRAMMES * tiles;
    if (blockIdx.x > work) {
        // ---- the copy: frames [f0, f0 + S2R_RESAMPLER_COPY_BLOCK) of the master to the pinned output ----
        const uint32_t f0 = (blockIdx.x - work - 1u) * S2R_RESAMPLER_COPY_BLOCK, f1 = f0 + S2R_RESAMPLER_COPY_BLOCK < F ? f0 + S2R_RESAMPLER_COPY_BLOCK : F;
        for (uint32_t n = f0 + tid; n < f1; n += kRsThreads) reinterpret_cast<rs2 *>(a.out)[n] = reinterpret_cast<const rs2 *>(a.master)[n];
        return;
    }
    if (blockIdx.x == work) {
        // ---- the next state: entry j of a channel's row is frame F - 1 - j, of the call or of the history in front of it ----
        for (uint32_t idx = tid; idx < S2R_RESAMPLER_PROGRAMMES * H; idx += kRsThreads) {
            const uint32_t p = idx / H, j = idx % H;
            const rs2 v = rs_frame(a, p, (int32_t)F - 1 - (int32_t)j);
            a.next[(2u * p) * H + j] = v.x; a.next[(2u * p + 1u) * H + j] = v.y;
        }
        return;
    }
    // ---- a tile of one programme ----
    const uint32_t p = blockIdx.x / tiles, i0 = (blockIdx.x % tiles) * kRsTile, cnt = a.count - i0 < kRsTile ? a.count - i0 : kRsTile;
    const uint64_t u0 = (uint64_t)a.ph + (uint64_t)i0 * a.M;
    const int32_t n0 = (int32_t)(u0 / a.L);                      // the frame of the tile's first output
    const uint32_t p0 = (uint32_t)(u0 % a.L);                    // ... and its phase; lane j: n0 + (p0 + j M) / L and (p0 + j M) mod L
    const uint32_t step = p0 + tid * a.M, row = step % a.L;
    const int32_t n = n0 + (int32_t)(step / a.L);
    rs2 y = rs2{0.0f, 0.0f};
#ifdef S2R_RESAMPLER_SERIAL
    if (tid < cnt) {
        const float *const h = a.table + (size_t)row * T;
        y = rs_sum(T, [&](const uint32_t k) { return h[k]; }, [&](const uint32_t k) { return rs_frame(a, p, n - (int32_t)k); });
    }
#else
    __shared__ float rows[kRsTile * kRsRow];                     // slot j: the row of lane j, T floats on a stride of T + 1
    __shared__ rs2 span[kRsSpan];                                // frames base .. of the programme, history included
    const int32_t base = n0 - (int32_t)H;
    const uint32_t len = (uint32_t)(n0 + (int32_t)((p0 + (cnt - 1u) * a.M) / a.L) - base) + 1u;      // <= ceil(63 M / L) + T <= kRsSpan
    for (uint32_t j = tid; j < len; j += kRsThreads) span[j] = rs_frame(a, p, base + (int32_t)j);
    const uint32_t quads = T >> 2, stride = T + 1u;
    if (a.L <= kRsTile) {                                        // (uniform) no more rows than the tile has lanes: the whole table, row r in slot r
        for (uint32_t idx = tid; idx < a.L * quads; idx += kRsThreads) {
            const uint32_t r = idx / quads, c4 = (idx % quads) * 4u;
            const rs4 v = *reinterpret_cast<const rs4 *>(a.table + (size_t)r * T + c4);
            float *const to = rows + r * stride + c4;
            to[0] = v.x; to[1] = v.y; to[2] = v.z; to[3] = v.w;
        }
        __syncthreads();
        if (tid < cnt) {
            const float *const h = rows + row * stride;
            const rs2 *const x = span + (n - base);              // n - base >= T - 1: x[-k] stays inside the span
            y = rs_sum(T, [&](const uint32_t k) { return h[k]; }, [&](const uint32_t k) { return x[-(int32_t)k]; });
        }
    } else {                                                     // the tile's rows, lane j's in slot j
        for (uint32_t idx = tid; idx < cnt * quads; idx += kRsThreads) {
            const uint32_t r = idx / quads, c4 = (idx % quads) * 4u;
            const rs4 v = *reinterpret_cast<const rs4 *>(a.table + (size_t)((p0 + r * a.M) % a.L) * T + c4);
            float *const to = rows + r * stride + c4;
            to[0] = v.x; to[1] = v.y; to[2] = v.z; to[3] = v.w;
        }
        __syncthreads();
        if (tid < cnt) {
            const float *const h = rows + tid * stride;
            const rs2 *const x = span + (n - base);
            y = rs_sum(T, [&](const uint32_t k) { return h[k]; }, [&](const uint32_t k) { return x[-(int32_t)k]; });
        }
    }
#endif
    if (tid < cnt) {
        const uint32_t i = i0 + tid;
        *reinterpret_cast<rs2 *>(a.res + ((size_t)p * a.out_cap + i) * 2u) = y;
        if (a.res_dev) *reinterpret_cast<rs2 *>(a.res_dev + ((size_t)p * a.count + i) * 2u) = y;
    }
}

hipError_t s2r_launch_resampler(const S2rResampler &a, hipStream_t stream) {
    if (a.frames == 0) return hipSuccess;
    const uint64_t span = (uint64_t)a.frames * a.L;
    if (a.n_buses > S2R_MAX_BUSES || (a.n_buses && !a.stems) || !a.master || a.out == a.master || !a.state || !a.next || a.next == a.state || !a.table || !a.res ||
        a.L < 1u || a.L > S2R_RESAMPLER_MAX_FACTOR || a.M < 1u || a.M > S2R_RESAMPLER_MAX_FACTOR || a.L > 4u * a.M || a.M > 4u * a.L ||
        a.T < S2R_RESAMPLER_MIN_TAPS || a.T > S2R_RESAMPLER_MAX_TAPS || a.T % 4u || a.L * a.T > S2R_RESAMPLER_MAX_TABLE || a.ph >= a.M ||
        a.frames > 0x7fffffffu / S2R_RESAMPLER_MAX_FACTOR || a.count != (span <= a.ph ? 0u : (span - a.ph + a.M - 1u) / a.M) || a.out_cap < a.count)
        return hipErrorInvalidValue;
    const uint32_t tiles = (a.count + kRsTile - 1u) / kRsTile;
    const dim3 grid(S2R_RESAMPLER_PROGRAMMES * tiles + 1u + (a.out ? (a.frames + S2R_RESAMPLER_COPY_BLOCK - 1u) / S2R_RESAMPLER_COPY_BLOCK : 0u)), block(kRsThreads);
    hipLaunchKernelGGL(s2r_resampler_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}
