// s2r_fx.hip — the per-bus convolution reverb of s2r_fill_buses: a K-tap FIR per bus channel over the dry bus
// signal and its carried history, summed in segments of S2R_IR_SEGMENT taps.  binary32, a product and the sum that takes it are two
// roundings (-ffp-contract=off), denormals kept, no atomics, no order that depends on timing, no MFMA.
//   s2r_fx_stage_kernel: what the bus combine left in the staging buffer (bus-major, L, R interleaved) goes, for a bus with a
//   reverb, behind the bus's history in its two planar lines, and for a bus without one straight to the caller's output.
//   s2r_fx_convolve_kernel: workgroup (tile, segment, bus channel) computes P_s for kFxTile frames (below).
//   s2r_fx_finish_kernel: adds the P_s in segment order from +0.0, y = dry * x + wet * r, and leaves the last K - 1 frames of the
//   line in the bus's OTHER line, which the host makes the current one (two buffers: the old and the new range overlap when a call
//   is shorter than the history).
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float fx2 __attribute__((ext_vector_type(2)));
typedef float fx4 __attribute__((ext_vector_type(4)));

constexpr int kFxW = 8;                                          // consecutive frames per thread
constexpr int kFxThreads = 128;
constexpr int kFxTile = kFxW * kFxThreads;                       // 1024 frames per workgroup
constexpr int kFxSeg = (int)S2R_IR_SEGMENT;
constexpr int kFxWin = kFxTile + kFxSeg;                         // the tile's samples and the 255 in front of them, one pad in front

}  // namespace

__global__ void __launch_bounds__(256) s2r_fx_stage_kernel(const S2rFx fx) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;    // bus i / (2 * frames); inside it frame r / 2, channel r & 1
    const uint32_t per = 2u * fx.frames, q = i / per, r = i - q * per;
    if (q >= fx.n_buses) return;
    const float v = fx.stage[i];
    const S2rFxBus &b = fx.bus[q];
    if (b.n_taps) b.line[(size_t)(r & 1u) * b.lstride + (b.n_taps - 1u) + (r >> 1)] = v;
    else fx.out[i] = v;
}

// P_s of one segment for a tile of frames of one bus channel.  The tile's kFxTile samples and the 255 in front of them — history
// where the tile or the segment reaches back past the call — are staged in LDS twice, the second copy one sample on, so that every
// pair of neighbouring frames is an aligned pair of registers for an even tap (first copy) and for an odd one (second copy).  A thread
// owns kFxW consecutive frames: per four taps it reads four more samples of each copy (16 bytes each) and slides its two windows
// down in registers; the taps are the same for the whole workgroup (scalar loads).  Per frame the terms are added in tap order from
// +0.0, each product rounded first; taps past K are +0.0 (s2r_set_bus_reverb pads the last segment) and so are samples in front of
// the history, which only such taps meet.
__global__ void __launch_bounds__(kFxThreads) s2r_fx_convolve_kernel(const S2rFx fx) {
    __shared__ __attribute__((aligned(16))) float s_e[kFxWin];   // s_e[m]: line sample base + m
    __shared__ __attribute__((aligned(16))) float s_o[kFxWin];   // s_o[m] = s_e[m + 1]
    const uint32_t seg = blockIdx.y, c = blockIdx.z & 1u;
    const S2rFxBus &b = fx.bus[blockIdx.z >> 1];
    if (b.n_taps == 0u || seg >= b.n_seg) return;                // (uniform: the whole workgroup leaves)
    const uint32_t t0 = blockIdx.x * (uint32_t)kFxTile;
    const float *line = b.line + (size_t)c * b.lstride;
    const int64_t base = (int64_t)(b.n_taps - 1u) + (int64_t)t0 - (int64_t)seg * kFxSeg - kFxSeg;
    const int64_t end = (int64_t)(b.n_taps - 1u) + (int64_t)fx.frames;
    for (int m = (int)threadIdx.x; m < kFxWin; m += kFxThreads) {
        const int64_t li = base + m;
        const float v = (li >= 0 && li < end) ? line[li] : 0.0f;
        s_e[m] = v;
        if (m) s_o[m - 1] = v;
    }
    if (threadIdx.x == 0) s_o[kFxWin - 1] = 0.0f;
    __syncthreads();
    const float *h = b.taps + (size_t)c * b.tstride + (size_t)seg * kFxSeg;
    const int f0 = (int)threadIdx.x * kFxW;
    // frame j of this thread under tap k of the segment takes s_e[f0 + j + kFxSeg - k].  we[m] = s_e[f0 + kFxSeg - k0 - 4 + m] and
    // wo[m] = s_o[same] for the four taps from k0: tap k0 + t, frame j reads we[4 + j - t] = wo[3 + j - t].
    float we[kFxW + 4], wo[kFxW + 4];
#pragma unroll
    for (int q = 0; q < kFxW + 4; q += 4) {
        const fx4 a = *reinterpret_cast<const fx4 *>(s_e + f0 + kFxSeg - 4 + q), o = *reinterpret_cast<const fx4 *>(s_o + f0 + kFxSeg - 4 + q);
#pragma unroll
        for (int j = 0; j < 4; ++j) { we[q + j] = a[j]; wo[q + j] = o[j]; }
    }
    fx2 acc[kFxW / 2];
#pragma unroll
    for (int j = 0; j < kFxW / 2; ++j) acc[j] = (fx2){0.0f, 0.0f};
#pragma unroll
    for (int k0 = 0; k0 < kFxSeg; k0 += 4) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float tap = h[k0 + t];
            const fx2 tt = (fx2){tap, tap};
#pragma unroll
            for (int j = 0; j < kFxW; j += 2) {
                const fx2 x = (t & 1) ? (fx2){wo[3 + j - t], wo[4 + j - t]} : (fx2){we[4 + j - t], we[5 + j - t]};
                const fx2 p = tt * x;                            // (rounded before the sum: -ffp-contract=off)
                acc[j / 2] = acc[j / 2] + p;
            }
        }
        if (k0 + 4 < kFxSeg) {
#pragma unroll
            for (int m = kFxW + 3; m >= 4; --m) { we[m] = we[m - 4]; wo[m] = wo[m - 4]; }
            const fx4 a = *reinterpret_cast<const fx4 *>(s_e + f0 + kFxSeg - k0 - 8), o = *reinterpret_cast<const fx4 *>(s_o + f0 + kFxSeg - k0 - 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) { we[j] = a[j]; wo[j] = o[j]; }
        }
    }
    float *dst = b.partials + ((size_t)c * b.n_seg + seg) * fx.pstride + t0 + (uint32_t)f0;
    const uint32_t i0 = t0 + (uint32_t)f0;
    if (i0 + (uint32_t)kFxW <= fx.frames) {                      // (pstride and t0 + f0 are multiples of 8: 16-byte stores)
        *reinterpret_cast<fx4 *>(dst) = (fx4){acc[0].x, acc[0].y, acc[1].x, acc[1].y};
        *reinterpret_cast<fx4 *>(dst + 4) = (fx4){acc[2].x, acc[2].y, acc[3].x, acc[3].y};
    } else {
#pragma unroll
        for (int j = 0; j < kFxW; ++j) if (i0 + (uint32_t)j < fx.frames) dst[j] = (j & 1) ? acc[j / 2].y : acc[j / 2].x;
    }
}

__global__ void __launch_bounds__(256) s2r_fx_finish_kernel(const S2rFx fx) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y >> 1, c = blockIdx.y & 1u;
    const S2rFxBus &b = fx.bus[q];
    if (b.n_taps == 0u) return;
    const uint32_t hist = b.n_taps - 1u;
    const float *line = b.line + (size_t)c * b.lstride;
    if (i < fx.frames) {
        const float *p = b.partials + (size_t)c * b.n_seg * fx.pstride + i;
        float r = 0.0f;
        for (uint32_t s = 0; s < b.n_seg; ++s) r = r + p[(size_t)s * fx.pstride];
        const float d = b.dry * line[hist + i], w = b.wet * r;
        fx.out[((size_t)q * fx.frames + i) * 2u + c] = d + w;
    }
    if (i < hist) b.next[(size_t)c * b.lstride + i] = line[(size_t)fx.frames + i];   // the last K - 1 of history + call, into the other buffer
}

hipError_t s2r_launch_bus_fx(const S2rFx &fx, hipStream_t stream) {
    if (fx.frames == 0 || fx.n_buses == 0) return hipSuccess;
    if (fx.n_buses > S2R_MAX_BUSES || !fx.stage || !fx.out || fx.pstride < fx.frames || (fx.pstride & 7u)) return hipErrorInvalidValue;
    uint32_t max_seg = 0, max_hist = 0;
    for (uint32_t q = 0; q < fx.n_buses; q++) {
        const S2rFxBus &b = fx.bus[q];
        if (b.n_taps == 0) continue;
        if (b.n_taps > S2R_MAX_IR_TAPS || b.n_seg != (b.n_taps + S2R_IR_SEGMENT - 1u) / S2R_IR_SEGMENT || b.tstride < b.n_seg * S2R_IR_SEGMENT ||
            (size_t)b.lstride < (size_t)(b.n_taps - 1u) + fx.frames || !b.taps || !b.line || !b.next || !b.partials || b.line == b.next)
            return hipErrorInvalidValue;
        if (b.n_seg > max_seg) max_seg = b.n_seg;
        if (b.n_taps - 1u > max_hist) max_hist = b.n_taps - 1u;
    }
    hipLaunchKernelGGL(s2r_fx_stage_kernel, dim3((2u * fx.frames * fx.n_buses + 255u) / 256u), dim3(256), 0, stream, fx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || max_seg == 0) return e;
    hipLaunchKernelGGL(s2r_fx_convolve_kernel, dim3((fx.frames + kFxTile - 1u) / kFxTile, max_seg, 2u * fx.n_buses), dim3(kFxThreads), 0, stream, fx);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t span = fx.frames > max_hist ? fx.frames : max_hist;
    hipLaunchKernelGGL(s2r_fx_finish_kernel, dim3((span + 255u) / 256u, 2u * fx.n_buses), dim3(256), 0, stream, fx);
    return hipGetLastError();
}
