// s2r_loudness.hip — the loudness and true-peak meters behind the master limiter of s2r_fill_master.  Per channel q of
// the 18 (bus b at 2 b, 2 b + 1, the master at 16, 17) and frame n of the call, in frame order:
//   y1 = stage 1 on v[n];   y2 = stage 2 on y1;   z = y2 * y2;   e = e + z;   after the frame pos + 1 == hop: e is the hop's, e = +0.0
// with a stage the nine operations of one EQ band (s2r_eq.hip), and for the master alone the four phases of the drive's interpolator,
//   u_p[n] = sum over j of g[p + 4 j] * x_c[n - j], from +0.0 in ascending j;   tp_c = max over n of |x_c[n]|, |u_p[n]|
// binary32, every operation rounded on its own (-ffp-contract=off), denormals kept, no atomics, no order that depends on timing.
//   s2r_loudness_kernel, ONE launch per call.  Workgroup 0 runs the 18 recursions, which are serial in n and independent of one
//   another: the WALKERS are lanes 0 .. 17 of wave 0, one channel each, both stages' four values and the hop sum in registers; the
//   STAGERS, waves 1 .. 4, a frame per lane, put tile j of S2R_LOUDNESS_TILE frames of all nine programmes into LDS (coalesced float2
//   loads, +0.0 for a bus past the call's) while the walkers walk tile j - 1 out of the other LDS buffer, eight frames read ahead of
//   their chain: one barrier per tile, and no walker waits for global memory.  LDS is frame-major, 18 floats a frame: the 18 walkers
//   read 18 consecutive banks.  The hop position is the same for all lanes: a block of eight frames that ends before the hop does
//   runs without a test.  A completed hop goes to the pinned rows from the walkers' lanes; the host appends the rows after the fill's
//   synchronise.  Workgroups 1 .. run the part that is independent per frame, 256 frames each, one per thread: a window of 256 + 16
//   master frames in LDS, the eight sums of 16 or 17 taps from registers and scalar taps, the copy of the master to the pinned output,
//   and the maxima through the 64-lane xor butterfly and LDS into one pinned row per workgroup (a maximum has one value in any
//   order).  The next state goes into the copy nobody reads in this launch.
// -DS2R_LOUDNESS_SERIAL builds the obvious form of the recursion for comparison (tools/loudness_time.py, CHANGELOG): a lane per channel
// steps through global memory frame by frame.
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float ld2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kLdTile = S2R_LOUDNESS_TILE;
constexpr uint32_t kLdThreads = 64u + kLdTile;                   // the walkers' wave, then a lane per frame of a tile
constexpr uint32_t kLdCh = S2R_LOUDNESS_CHANNELS;                // floats of a frame in LDS
constexpr uint32_t kLdBlock = 8;                                 // frames a walker reads from LDS ahead of their chain
constexpr uint32_t kLdHist = 16;                                 // master frames in front of a true-peak workgroup's
constexpr uint32_t kLdFilt = 0, kLdSums = 72, kLdPast = 90;      // the state's layout (s2r_rules.h)
static_assert(kLdTile == S2R_LOUDNESS_BLOCK && kLdTile % kLdBlock == 0u && kLdThreads == 320u, "five waves: the walkers', and a frame per lane of four");
static_assert(kLdPast + 2u * kLdHist == S2R_LOUDNESS_STATE && 4u * kLdHist + 1u == S2R_DRIVE_TAPS && S2R_LOUDNESS_HALF_TAPS == 2u * kLdHist + 1u, "s2r.h's layout");
static_assert(2u * (kLdTile + kLdHist) <= 2u * kLdTile * kLdCh, "the true-peak window fits the tiles' LDS");

struct LdStage { float b0, b1, b2, a1, a2; };

// one stage, one frame: the rule's nine operations
__device__ __forceinline__ float ld_stage(const LdStage &q, const float x, float &s1, float &s2) {
    const float p0 = q.b0 * x;
    const float y = p0 + s1;
    const float p1 = q.b1 * x, r1 = q.a1 * y;
    const float d1 = p1 - r1;
    const float p2 = q.b2 * x, r2 = q.a2 * y;
    s1 = d1 + s2;
    s2 = p2 - r2;
    return y;
}

struct LdWalk {
    LdStage k1, k2;
    float s[4], e;                                               // stage 1's (s1, s2), stage 2's, the hop sum
    uint32_t pos, row;                                           // (the same in every lane)
    __device__ __forceinline__ void frame(const float v) {
        const float y1 = ld_stage(k1, v, s[0], s[1]);
        const float y2 = ld_stage(k2, y1, s[2], s[3]);
        const float z = y2 * y2;
        e = e + z;
    }
    // after a frame: the hop ends with it, or not
    __device__ __forceinline__ void turn(const uint32_t hop, float *rows, const uint32_t q) {
        if (++pos == hop) { rows[(size_t)row * kLdCh + q] = e; e = 0.0f; row++; pos = 0u; }
    }
};

// tap k of g, 0 .. 64, from the half the arguments carry
__device__ __forceinline__ float ld_tap(const S2rLoudness &a, const uint32_t k) { return a.g[k < S2R_LOUDNESS_HALF_TAPS ? k : S2R_DRIVE_TAPS - 1u - k]; }

}  // namespace

__global__ void __launch_bounds__(kLdThreads) s2r_loudness_kernel(const S2rLoudness a) {
    __shared__ __attribute__((aligned(16))) float xin[2][kLdTile * kLdCh];       // two tiles, [frame][channel]
    const uint32_t tid = threadIdx.x, N = a.frames;
    const ld2 *const m2 = reinterpret_cast<const ld2 *>(a.master);
    if (blockIdx.x > 0) {
        // ---- the true peak and the copy: frames [f0, f0 + 256) ----
        __shared__ float s_pk[kLdThreads / 64u][2];
        ld2 *const win = reinterpret_cast<ld2 *>(&xin[0][0]);    // frame f0 - 16 + i at i
        const uint32_t f0 = (blockIdx.x - 1u) * S2R_LOUDNESS_BLOCK;
        for (uint32_t i = tid; i < S2R_LOUDNESS_BLOCK + kLdHist; i += kLdThreads) {
            const uint32_t f = f0 + i;                           // the frame, counted from 16 in front of the call
            ld2 v = ld2{0.0f, 0.0f};
            if (f < kLdHist) v = *reinterpret_cast<const ld2 *>(a.state + kLdPast + 2u * f);
            else if (f - kLdHist < N) v = m2[f - kLdHist];
            win[i] = v;
        }
        __syncthreads();
        const uint32_t n = f0 + tid;
        float pl = 0.0f, pr = 0.0f;
        if (tid < S2R_LOUDNESS_BLOCK && n < N) {
            ld2 x[kLdHist + 1u];                                 // x[n - j] at j
#pragma unroll
            for (uint32_t j = 0; j <= kLdHist; j++) x[j] = win[tid + kLdHist - j];
            reinterpret_cast<ld2 *>(a.out)[n] = x[0];
            pl = __builtin_fabsf(x[0].x); pr = __builtin_fabsf(x[0].y);
#pragma unroll
            for (uint32_t p = 0; p < S2R_DRIVE_OVERSAMPLE; p++) {
                ld2 u = ld2{0.0f, 0.0f};
#pragma unroll
                for (uint32_t j = 0; p + 4u * j < S2R_DRIVE_TAPS; j++) {
                    const float g = ld_tap(a, p + 4u * j);
                    const ld2 t = ld2{g, g} * x[j];
                    u = u + t;
                }
                const float al = __builtin_fabsf(u.x), ar = __builtin_fabsf(u.y);
                pl = al > pl ? al : pl; pr = ar > pr ? ar : pr;
            }
        }
        const uint32_t wave = tid >> 6, lane = tid & 63u;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float l2 = __shfl_xor(pl, off, 64), r2 = __shfl_xor(pr, off, 64);
            pl = l2 > pl ? l2 : pl; pr = r2 > pr ? r2 : pr;
        }
        if (lane == 0) { s_pk[wave][0] = pl; s_pk[wave][1] = pr; }
        __syncthreads();
        if (tid < 2u) {
            float m = s_pk[0][tid];
            for (uint32_t w = 1; w < kLdThreads / 64u; w++) m = s_pk[w][tid] > m ? s_pk[w][tid] : m;
            a.peaks[(size_t)(blockIdx.x - 1u) * 2u + tid] = m;
        }
        return;
    }
    // ---- workgroup 0: the recursions ----
    const bool walker = tid < kLdCh, stager = tid >= 64u;
    const uint32_t q = tid, w = tid - 64u;                       // a walker's channel, a stager's frame of a tile
    const uint32_t hop = a.hop;
    LdWalk k{};
    if (walker) {
        k.k1 = LdStage{a.c[0], a.c[1], a.c[2], a.c[3], a.c[4]};
        k.k2 = LdStage{a.c[5], a.c[6], a.c[7], a.c[8], a.c[9]};
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) k.s[i] = a.state[kLdFilt + 4u * q + i];
        k.e = a.state[kLdSums + q];
    }
    k.pos = a.pos; k.row = 0u;
    // the master's last 16 frames of what the state held followed by the call: frame N + i of that sequence, i < 16
    if (stager && w < 2u * kLdHist) {
        const uint32_t f = N + (w >> 1), c = w & 1u;
        a.next[kLdPast + w] = f < kLdHist ? a.state[kLdPast + 2u * f + c] : a.master[2u * (size_t)(f - kLdHist) + c];
    }
#ifdef S2R_LOUDNESS_SERIAL
    if (walker) {
        const uint32_t p = q >> 1, c = q & 1u;
        const float *const src = p == S2R_MAX_BUSES ? a.master + c : a.stems + (size_t)p * 2u * N + c;
        const bool fed = p == S2R_MAX_BUSES || p < a.n_buses;
        for (uint32_t n = 0; n < N; n++) {
            k.frame(fed ? src[2u * (size_t)n] : 0.0f);
            k.turn(hop, a.rows, q);
        }
    }
#else
    const uint32_t tiles = (N + kLdTile - 1u) / kLdTile;
    for (uint32_t j = 0; j <= tiles; j++) {
        if (stager && j < tiles) {
            const uint32_t n = j * kLdTile + w;
            float *const to = xin[j & 1u] + w * kLdCh;              // (written as floats, as the walkers read them)
            ld2 v[S2R_LOUDNESS_PROGRAMMES];
#pragma unroll
            for (uint32_t p = 0; p < S2R_MAX_BUSES; p++) {
                v[p] = ld2{0.0f, 0.0f};                          // a bus past the call's, and a frame past the call (never walked)
                if (p < a.n_buses && n < N) v[p] = *reinterpret_cast<const ld2 *>(a.stems + ((size_t)p * N + n) * 2u);
            }
            v[S2R_MAX_BUSES] = n < N ? m2[n] : ld2{0.0f, 0.0f};
#pragma unroll
            for (uint32_t p = 0; p < S2R_LOUDNESS_PROGRAMMES; p++) { to[2u * p] = v[p].x; to[2u * p + 1u] = v[p].y; }
        } else if (walker && j >= 1u) {
            const uint32_t t0 = (j - 1u) * kLdTile, cnt = N - t0 < kLdTile ? N - t0 : kLdTile;
            const float *const tp = xin[(j - 1u) & 1u] + q;      // frame i of the tile at i * 18
            float cur[kLdBlock];
#pragma unroll
            for (uint32_t u = 0; u < kLdBlock; u++) cur[u] = tp[u * kLdCh];
            uint32_t i = 0;
            for (; i + kLdBlock <= cnt; i += kLdBlock) {
                const uint32_t nx = i + kLdBlock < kLdTile ? i + kLdBlock : i;   // the next block, read ahead (the last one: itself again)
                float nxt[kLdBlock];
#pragma unroll
                for (uint32_t u = 0; u < kLdBlock; u++) nxt[u] = tp[(nx + u) * kLdCh];
                if (hop - k.pos > kLdBlock) {                    // no hop ends inside the block
#pragma unroll
                    for (uint32_t u = 0; u < kLdBlock; u++) k.frame(cur[u]);
                    k.pos += kLdBlock;
                } else {
#pragma unroll
                    for (uint32_t u = 0; u < kLdBlock; u++) { k.frame(cur[u]); k.turn(hop, a.rows, q); }
                }
#pragma unroll
                for (uint32_t u = 0; u < kLdBlock; u++) cur[u] = nxt[u];
            }
            for (; i < cnt; i++) { k.frame(tp[i * kLdCh]); k.turn(hop, a.rows, q); }       // the call's last frames, fewer than a block
        }
        __syncthreads();
    }
#endif
    if (walker) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) a.next[kLdFilt + 4u * q + i] = k.s[i];
        a.next[kLdSums + q] = k.e;
    }
}

hipError_t s2r_launch_loudness(const S2rLoudness &a, hipStream_t stream) {
    if (a.frames == 0) return hipSuccess;
    if (a.n_buses > S2R_MAX_BUSES || (a.n_buses && !a.stems) || !a.master || !a.out || a.out == a.master || !a.state || !a.next || a.next == a.state || !a.rows ||
        !a.peaks || a.hop < S2R_LOUDNESS_MIN_HOP || a.hop > S2R_LOUDNESS_MAX_HOP || a.pos >= a.hop)
        return hipErrorInvalidValue;
    const dim3 grid(1u + (a.frames + S2R_LOUDNESS_BLOCK - 1u) / S2R_LOUDNESS_BLOCK), block(kLdThreads);
    hipLaunchKernelGGL(s2r_loudness_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}
