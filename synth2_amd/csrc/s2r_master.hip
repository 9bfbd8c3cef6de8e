// s2r_master.hip — the master section of s2r_fill_master: the buses' stems, post-effect, each times its return, added
// in bus order from +0.0, times the master fader; and the meters of the call — peak and energy of every stem channel (pre-return) and
// of the master.  binary32, a product and the sum that takes it are two roundings (-ffp-contract=off), denormals kept, no atomics, no
// order that depends on timing.
//   s2r_master_kernel<NB>: one workgroup of S2R_METER_BLOCK = 256 threads per meter block, one frame per thread.  The stems come from
//   device memory (S2rMaster.stage: the last stem writer of a master fill writes there, never into the pinned output the host reads);
//   the master goes to mapped host memory, and so do the stems when the caller wants them.  Every thread's |v| and v * v go through a
//   64-lane xor butterfly — lane j and lane j ^ 1 form the same sum, the additions commute, so after six steps every lane holds the
//   adjacent-pair tree's value of its wave — and the four waves' values through LDS as (w0 + w1) + (w2 + w3): levels seven and eight of
//   the tree.  One row of block partials per workgroup; the host adds the rows in block order after the fill's synchronise.
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float ms2 __attribute__((ext_vector_type(2)));

constexpr int kMasterThreads = (int)S2R_METER_BLOCK;
static_assert(kMasterThreads == 256, "the reduction below is a 64-lane butterfly and four waves");

}  // namespace

template <int NB>
__global__ void __launch_bounds__(kMasterThreads) s2r_master_kernel(const S2rMaster m) {
    constexpr int CH = (NB + 1) * 2;                             // bus b at 2 b, 2 b + 1; the master behind them
    __shared__ float s_pk[4][CH], s_en[4][CH];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * (uint32_t)kMasterThreads + tid;       // the frame, counted from the start of the call
    const bool in = i < m.frames;
    const float fi = (float)i;
    float v[CH];
    ms2 t = (ms2){0.0f, 0.0f};
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        ms2 y = (ms2){0.0f, 0.0f};                               // a frame past the call and a bus past n_buses: +0.0
        if (b < (int)m.n_buses) {                                // (uniform: three buses run the 4-bus form)
            const size_t at = ((size_t)b * m.frames + i) * 2u;
            if (in) y = *reinterpret_cast<const ms2 *>(m.stage + at);
            const float step = fi * m.dr[b];                     // (rounded before the sum: -ffp-contract=off)
            const float r = m.r0[b] + step;
            const ms2 p = (ms2){r, r} * y;
            t = t + p;
            if (in && m.stems) *reinterpret_cast<ms2 *>(m.stems + at) = y;
        }
        v[2 * b] = y.x; v[2 * b + 1] = y.y;
    }
    {
        const float step = fi * m.dm;
        const float g = m.m0 + step;
        const ms2 o = (ms2){g, g} * t;
        if (in) *reinterpret_cast<ms2 *>(m.out + (size_t)i * 2u) = o;
        v[2 * NB] = in ? o.x : 0.0f; v[2 * NB + 1] = in ? o.y : 0.0f;
    }
    const uint32_t wave = tid >> 6, lane = tid & 63u;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        float pk = __builtin_fabsf(v[c]), en = v[c] * v[c];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float e2 = __shfl_xor(en, off, 64), p2 = __shfl_xor(pk, off, 64);
            en = en + e2;
            pk = pk > p2 ? pk : p2;
        }
        if (lane == 0) { s_pk[wave][c] = pk; s_en[wave][c] = en; }
    }
    __syncthreads();
    if (tid < (uint32_t)CH) {
        const uint32_t b = tid >> 1;
        if (b < m.n_buses || b == (uint32_t)NB) {
            const uint32_t ch = b == (uint32_t)NB ? 2u * m.n_buses + (tid & 1u) : tid;       // the caller's layout: the master right behind the call's buses
            const float e01 = s_en[0][tid] + s_en[1][tid], e23 = s_en[2][tid] + s_en[3][tid];
            const float p01 = s_pk[0][tid] > s_pk[1][tid] ? s_pk[0][tid] : s_pk[1][tid], p23 = s_pk[2][tid] > s_pk[3][tid] ? s_pk[2][tid] : s_pk[3][tid];
            float *row = m.partials + (size_t)blockIdx.x * S2R_MASTER_ROW;
            row[ch] = p01 > p23 ? p01 : p23;
            row[S2R_MASTER_CH + ch] = e01 + e23;
        }
    }
}

hipError_t s2r_launch_master(const S2rMaster &m, hipStream_t stream) {
    if (m.frames == 0) return hipSuccess;
    if (m.n_buses == 0 || m.n_buses > S2R_MAX_BUSES || !m.stage || !m.out || !m.partials) return hipErrorInvalidValue;
    const dim3 grid((m.frames + (uint32_t)kMasterThreads - 1u) / (uint32_t)kMasterThreads), block(kMasterThreads);
    if (m.n_buses == 1) hipLaunchKernelGGL(s2r_master_kernel<1>, grid, block, 0, stream, m);
    else if (m.n_buses == 2) hipLaunchKernelGGL(s2r_master_kernel<2>, grid, block, 0, stream, m);
    else if (m.n_buses <= 4) hipLaunchKernelGGL(s2r_master_kernel<4>, grid, block, 0, stream, m);
    else hipLaunchKernelGGL(s2r_master_kernel<8>, grid, block, 0, stream, m);
    return hipGetLastError();
}
