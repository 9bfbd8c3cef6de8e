// s2r_spectrum.hip — the spectrum meters behind the loudness meters of s2r_fill_master.  Per programme p of the nine
// (bus b at b, the master at 8) and per hop the call completes, over the N = n_fft most recent frames, oldest first:
//   z[i] = (window[i] * L[i], window[i] * R[i]);   v = radix-2 decimation-in-time FFT of z with the host's twiddle table;
//   p[k] = ((|v[k]|^2) + (|v[(N - k) mod N]|^2)) * 0.5f,   k = 0 .. N / 2
// binary32, every operation rounded on its own (-ffp-contract=off), denormals kept, no atomics, no order that depends on timing.
//   s2r_spectrum_kernel, ONE launch per call.  Workgroup (row r, programme p) gathers its N frames from the state's line and the
//   call's device buffers with coalesced float2 loads, applies the window and writes z into LDS at the bit-reversed index; the
//   twiddles go into LDS beside it.  The transform runs in place in LDS: a thread takes 8 or 16 points whose indices differ in the
//   3 or 4 bits of one pass, runs those radix-2 layers in registers — the very operations of the rule, every product with a
//   twiddle included —, and puts them back: ceil(log2 N / 4) exchanges through LDS, one barrier each (2 at N = 256, 3 at 2048, 4
//   at 8192), not log2 N.  LDS indices are padded by one float2 per 32, which spreads the first pass's stride-8 and stride-16
//   accesses and most of the bit-reversed writes over the banks.  The power row goes straight to the pinned rows.  A bus at or past
//   the call's n_buses gets +0.0 and no transform.  The last S2R_SPECTRUM_COPY_BLOCKS workgroups write the next state — the last N
//   frames of the state followed by the call, per programme — into the copy nobody reads in this launch, and, when no loudness
//   kernel has, the master into the pinned output.
// -DS2R_SPECTRUM_SERIAL builds the obvious form for comparison (tools/spectrum_time.py, CHANGELOG): a barrier per radix-2 layer, no
// padding, one point pair per thread and layer.
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float sp2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kSpMaxThreads = 1024u;
constexpr uint32_t kSpP = S2R_SPECTRUM_PROGRAMMES;
constexpr uint32_t kSpMaxLds = (S2R_SPECTRUM_MAX_FFT + S2R_SPECTRUM_MAX_FFT / 32u + S2R_SPECTRUM_MAX_FFT / 2u) * 8u;
static_assert(kSpMaxLds <= 160u * 1024u, "the largest transform and its twiddles fit the LDS of a compute unit");

// where point i sits in LDS
#ifdef S2R_SPECTRUM_SERIAL
__device__ __forceinline__ uint32_t sp_at(const uint32_t i) { return i; }
#else
__device__ __forceinline__ uint32_t sp_at(const uint32_t i) { return i + (i >> 5); }
#endif

// the rule's butterfly: t = w * b, ten operations, each rounded on its own
__device__ __forceinline__ void sp_fly(const sp2 w, sp2 &a, sp2 &b) {
    const float p0 = w.x * b.x, p1 = w.y * b.y, p2 = w.x * b.y, p3 = w.y * b.x;
    const float tr = p0 - p1, ti = p2 + p3;
    const float ar = a.x, ai = a.y;
    a = sp2{ar + tr, ai + ti};
    b = sp2{ar - tr, ai - ti};
}

#ifndef S2R_SPECTRUM_SERIAL
// layers s0 + 1 .. s0 + C of the transform, in place: a task owns the 2^C points base + (q << s0)
template <uint32_t C>
__device__ __forceinline__ void sp_pass(sp2 *const v, const sp2 *const tw, const uint32_t N, const uint32_t L, const uint32_t s0, const uint32_t tid,
                                        const uint32_t threads) {
    constexpr uint32_t R = 1u << C;
    for (uint32_t t = tid; t < (N >> C); t += threads) {
        const uint32_t lo = t & ((1u << s0) - 1u), base = ((t >> s0) << (s0 + C)) | lo;
        sp2 x[R];
#pragma unroll
        for (uint32_t q = 0; q < R; q++) x[q] = v[sp_at(base + (q << s0))];
#pragma unroll
        for (uint32_t l = 0; l < C; l++) {                       // layer s = s0 + l + 1: h = 2^(s0 + l), w = T[j * N / 2^s]
            const uint32_t shift = L - (s0 + l + 1u);
#pragma unroll
            for (uint32_t q = 0; q < R; q++) {
                if (q & (1u << l)) continue;
                const uint32_t j = ((q & ((1u << l) - 1u)) << s0) | lo;
                sp_fly(tw[j << shift], x[q], x[q | (1u << l)]);
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < R; q++) v[sp_at(base + (q << s0))] = x[q];
    }
}
#endif

}  // namespace

__global__ void __launch_bounds__(kSpMaxThreads) s2r_spectrum_kernel(const S2rSpectrum a, const uint32_t L, const uint32_t n_rows) {
    extern __shared__ __attribute__((aligned(16))) float sp_lds[];
    const uint32_t tid = threadIdx.x, threads = blockDim.x, N = a.n_fft, F = a.frames;
    const sp2 *const st2 = reinterpret_cast<const sp2 *>(a.state);
    const sp2 *const m2 = reinterpret_cast<const sp2 *>(a.master);
    const uint32_t n_fft_blocks = n_rows * kSpP;
    if (blockIdx.x >= n_fft_blocks) {
        // ---- the next state, and the copy: x = the state's N frames followed by the call's, the next state x[F .. F + N) ----
        const uint32_t cb = blockIdx.x - n_fft_blocks, stride = S2R_SPECTRUM_COPY_BLOCKS * threads;
        sp2 *const next2 = reinterpret_cast<sp2 *>(a.next);
        for (uint32_t e = cb * threads + tid; e < kSpP * N; e += stride) {
            const uint32_t p = e >> L, xi = F + (e & (N - 1u));
            sp2 f = sp2{0.0f, 0.0f};                             // a bus past the call's is fed +0.0
            if (xi < N) f = st2[(size_t)p * N + xi];
            else if (p == S2R_MAX_BUSES) f = m2[xi - N];
            else if (p < a.n_buses) f = *reinterpret_cast<const sp2 *>(a.stems + ((size_t)p * F + (xi - N)) * 2u);
            next2[e] = f;
        }
        if (a.out) for (uint32_t n = cb * threads + tid; n < F; n += stride) reinterpret_cast<sp2 *>(a.out)[n] = m2[n];
        return;
    }
    // ---- one row of one programme ----
    const uint32_t r = blockIdx.x / kSpP, p = blockIdx.x - r * kSpP, bins = N / 2u + 1u;
    float *const out = a.rows + ((size_t)r * kSpP + p) * bins;
    if (p < S2R_MAX_BUSES && p >= a.n_buses) {
        for (uint32_t k = tid; k < bins; k += threads) out[k] = 0.0f;
        return;
    }
    sp2 *const v = reinterpret_cast<sp2 *>(sp_lds);              // N points, padded
    sp2 *const tw = v + (N + N / 32u);                           // N / 2 twiddles
    const sp2 *const src2 = p == S2R_MAX_BUSES ? m2 : reinterpret_cast<const sp2 *>(a.stems + (size_t)p * F * 2u);
    const uint32_t first = (r + 1u) * a.hop - a.pos;             // the row's oldest frame in x: it ends at frame (r + 1) hop - pos - 1 of the call
    for (uint32_t i = tid; i < N; i += threads) {
        const uint32_t xi = first + i;
        const sp2 f = xi < N ? st2[(size_t)p * N + xi] : src2[xi - N];
        const float w = a.window[i];
        v[sp_at(__brev(i) >> (32u - L))] = sp2{w * f.x, w * f.y};
    }
    for (uint32_t j = tid; j < N / 2u; j += threads) tw[j] = reinterpret_cast<const sp2 *>(a.twiddles)[j];
    __syncthreads();
#ifdef S2R_SPECTRUM_SERIAL
    for (uint32_t s = 1; s <= L; s++) {
        const uint32_t h = 1u << (s - 1u);
        for (uint32_t t = tid; t < N / 2u; t += threads) {
            const uint32_t j = t & (h - 1u), g = (t >> (s - 1u)) << s;
            sp2 x = v[g + j], y = v[g + j + h];
            sp_fly(tw[j << (L - s)], x, y);
            v[g + j] = x; v[g + j + h] = y;
        }
        __syncthreads();
    }
#else
    const uint32_t passes = (L + 3u) / 4u;                       // L = 8 .. 13: 4 4 | 3 3 3 | 4 3 3 | 4 4 3 | 4 4 4 | 4 3 3 3
    for (uint32_t i = 0, s0 = 0; i < passes; i++) {
        const uint32_t c = L / passes + (i < L % passes ? 1u : 0u);
        if (c == 4u) sp_pass<4>(v, tw, N, L, s0, tid, threads);
        else sp_pass<3>(v, tw, N, L, s0, tid, threads);
        s0 += c;
        __syncthreads();
    }
#endif
    for (uint32_t k = tid; k < bins; k += threads) {
        const sp2 x = v[sp_at(k)], y = v[sp_at((N - k) & (N - 1u))];
        const float x0 = x.x * x.x, x1 = x.y * x.y, y0 = y.x * y.x, y1 = y.y * y.y;
        const float sx = x0 + x1, sy = y0 + y1;
        const float t = sx + sy;
        out[k] = t * 0.5f;
    }
}

hipError_t s2r_launch_spectrum(const S2rSpectrum &a, hipStream_t stream) {
    if (a.frames == 0) return hipSuccess;
    const uint32_t N = a.n_fft;
    if (N < S2R_SPECTRUM_MIN_FFT || N > S2R_SPECTRUM_MAX_FFT || (N & (N - 1u)) != 0u || a.n_buses > S2R_MAX_BUSES || (a.n_buses && !a.stems) || !a.master ||
        a.out == a.master || !a.state || !a.next || a.next == a.state || !a.window || !a.twiddles || !a.rows || a.hop < S2R_SPECTRUM_MIN_HOP ||
        a.hop < N / 8u || a.hop > S2R_SPECTRUM_MAX_HOP || a.pos >= a.hop)
        return hipErrorInvalidValue;
    uint32_t L = 0;
    while ((1u << L) < N) L++;
    const uint32_t n_rows = (uint32_t)(((uint64_t)a.pos + a.frames) / a.hop);
    const uint32_t threads = N / 8u < 64u ? 64u : (N / 8u > kSpMaxThreads ? kSpMaxThreads : N / 8u);
    const size_t lds = (size_t)(N + N / 32u + N / 2u) * 8u;
    if (lds > 64u * 1024u) {                                     // (N = 8192 alone: more dynamic LDS than a launch gets unasked, on the current device)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(s2r_spectrum_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSpMaxLds);
        if (e != hipSuccess) return e;
    }
    const dim3 grid(n_rows * kSpP + S2R_SPECTRUM_COPY_BLOCKS), block(threads);
    hipLaunchKernelGGL(s2r_spectrum_kernel, grid, block, lds, stream, a, L, n_rows);
    return hipGetLastError();
}
