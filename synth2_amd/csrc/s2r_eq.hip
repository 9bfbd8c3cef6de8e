// s2r_eq.hip — the per-bus parametric EQ of s2r_fill_buses and s2r_fill_master, at the head of the post-mix chain: a
// cascade of up to four biquads in transposed direct form II, per channel c and band k with x the previous band's y:
//   y = (b0 * x) + s1;   s1' = ((b1 * x) - (a1 * y)) + s2;   s2' = (b2 * x) - (a2 * y)
// binary32, every product and every sum rounded on its own (-ffp-contract=off), denormals kept, nothing skipped for a zero
// coefficient.  Frame n needs frame n - 1: the first stage of the chain that is serial in time, so its cost is latency per frame and
// one thread per frame is no recipe.  The kernel is systolic: ONE wavefront, one lane per (bus, channel, band) — 8 x 2 x 4 = 64, the
// four bands of a channel in one quad — and at step t the lane of band k works on frame t - k, taking as x what its left neighbour
// produced one step earlier through a quad-permute DPP move (band 0: the staged input).  A step is the nine operations of ONE band
// whatever the number of bands and buses; a call takes N + bands - 1 steps.  Each lane does exactly the operations of the rule in
// the rule's order, so the output is the sequential cascade's bit for bit.  Memory stays off the dependent chain: the wave loads
// the input one tile of S2R_EQ_TILE frames ahead (global -> registers -> LDS, coalesced), reads x from LDS eight steps at a time,
// puts y into an LDS ring — at the slot of the STEP, so that the eight addresses of a block are one base and eight immediates — and
// stores it to `out` one tile behind, coalesced.  No atomics, nothing that waits for another workgroup.
// -DS2R_EQ_SERIAL builds the obvious form for comparison (tools/eq_time.py, CHANGELOG): the lane of band 0 runs the whole cascade.
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float eq2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kEqLanes = 64;                                // one wavefront
constexpr uint32_t kEqTile = S2R_EQ_TILE;                        // frames staged at a time
constexpr uint32_t kEqRing = 2u * kEqTile;                       // frames of the output ring: a tile being flushed and a tile being written
constexpr uint32_t kEqRows = 2u * S2R_MAX_BUSES;                 // (bus, channel) rows of the staged tiles
constexpr uint32_t kEqPer = kEqRows * kEqTile / kEqLanes;        // floats of a tile per lane
constexpr uint32_t kEqUnroll = 8;                                // steps whose x is read from LDS ahead of their chain
constexpr uint32_t kEqCopyFrames = 4u * kEqLanes;                // frames per workgroup of the copy of a bus without an EQ
static_assert(S2R_MAX_BUSES * 2u * S2R_EQ_MAX_BANDS == kEqLanes && S2R_EQ_MAX_BANDS == 4u, "one lane per (bus, channel, band), a quad per channel");
static_assert(kEqTile == 64u && kEqTile % kEqUnroll == 0u, "the tile's lane mapping below is written for 64 frames");

struct EqBand { float b0, b1, b2, a1, a2; };

// one band, one frame: the rule's nine operations
__device__ __forceinline__ float eq_band(const EqBand &q, const float x, const float s1, const float s2, float &n1, float &n2) {
    const float p0 = q.b0 * x;
    const float y = p0 + s1;
    const float p1 = q.b1 * x, r1 = q.a1 * y;
    const float d1 = p1 - r1;
    const float p2 = q.b2 * x, r2 = q.a2 * y;
    n1 = d1 + s2;
    n2 = p2 - r2;
    return y;
}

// what the left neighbour of the quad holds (lane 0 of a quad: its own, unused): quad_perm [0, 0, 1, 2]
__device__ __forceinline__ float eq_from_left(const float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x90, 0xf, 0xf, true));
}

// element e = j * 64 + lane of a tile: bus j / 2, and inside the bus 2 * 64 floats, frame-major, L then R — as in global memory
__device__ __forceinline__ void eq_tile_elem(const uint32_t j, const uint32_t lane, uint32_t &bus, uint32_t &fr, uint32_t &c) {
    const uint32_t off = (j & 1u) * kEqLanes + lane;
    bus = j >> 1; fr = off >> 1; c = off & 1u;
}

}  // namespace

// Workgroup (0, 0) is the systolic wave.  Workgroups (1 + g, bus) exist when a bus of the call carries no EQ, and copy that bus from
// `in` to `out`, 256 frames each; every other workgroup returns at once.  `depth`: the most bands of any bus of the call.
__global__ void __launch_bounds__(kEqLanes) s2r_eq_kernel(const S2rEq a, const uint32_t depth) {
    const uint32_t lane = threadIdx.x, N = a.frames;
    if (blockIdx.x > 0) {
        const uint32_t q = blockIdx.y;
        if (a.bus[q].n_bands) return;                            // (uniform: the whole workgroup)
        const eq2 *x2 = reinterpret_cast<const eq2 *>(a.in) + (uint64_t)q * N;
        eq2 *y2 = reinterpret_cast<eq2 *>(a.out) + (uint64_t)q * N;
        for (uint32_t j = 0; j < kEqCopyFrames / kEqLanes; j++) {
            const uint32_t n = (blockIdx.x - 1u) * kEqCopyFrames + j * kEqLanes + lane;
            if (n < N) y2[n] = x2[n];
        }
        return;
    }
    if (blockIdx.y > 0) return;

    __shared__ float xin[2][kEqRows * (kEqTile + 1u)];           // the input, two tiles: [row][frame of the tile], padded against bank conflicts
    __shared__ float ring[kEqRows * (kEqRing + 1u)];             // the output: [row][step mod kEqRing]: frame f of a cascade of nb bands leaves at step f + nb - 1
    __shared__ float trash[kEqLanes * (kEqUnroll + 1u)];         // where a lane that emits nothing writes in a full block, so that the store needs no branch
    const uint32_t bus = lane >> 3, ch = (lane >> 2) & 1u, k = lane & 3u, row = lane >> 2;
    const uint32_t nb = bus < a.n_buses ? a.bus[bus].n_bands : 0u;
#ifdef S2R_EQ_SERIAL
    const bool mine = k == 0u && nb != 0u;                       // the lane of band 0 runs the cascade
    const uint32_t sk = 0u;
    EqBand q[S2R_EQ_MAX_BANDS];
    float s1[S2R_EQ_MAX_BANDS], s2[S2R_EQ_MAX_BANDS];
#pragma unroll
    for (uint32_t kk = 0; kk < S2R_EQ_MAX_BANDS; kk++) {
        const bool has = mine && kk < nb;
        const float *c = a.bus[bus].c[kk];
        q[kk] = has ? EqBand{c[0], c[1], c[2], c[3], c[4]} : EqBand{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        s1[kk] = has ? a.bus[bus].line[4u * kk + ch] : 0.0f;
        s2[kk] = has ? a.bus[bus].line[4u * kk + 2u + ch] : 0.0f;
    }
    (void)depth;
#else
    const bool mine = k < nb;                                    // a lane past its bus's bands, or of a bus without an EQ, is idle: it writes nothing
    const bool emit = mine && k + 1u == nb;                      // the last band's lane puts y into the ring
    const uint32_t sk = depth - 1u;                              // the skew of the deepest cascade: band k is k frames behind band 0
    const float *c = a.bus[bus].c[k];
    const EqBand q = mine ? EqBand{c[0], c[1], c[2], c[3], c[4]} : EqBand{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float s1 = mine ? a.bus[bus].line[4u * k + ch] : 0.0f, s2 = mine ? a.bus[bus].line[4u * k + 2u + ch] : 0.0f;
    float y = 0.0f;
#endif
    const uint32_t steps = N + sk, tiles = (steps + kEqTile - 1u) / kEqTile;
    float *const my_ring = ring + row * (kEqRing + 1u);
    float *const my_trash = trash + lane * (kEqUnroll + 1u);

    float ahead[kEqPer];
    // frames [i * T, i * T + T) of every bus with an EQ, as far as the call has them, into registers: issued a tile ahead of their use
    auto load_tile = [&](const uint32_t i) {
#pragma unroll
        for (uint32_t j = 0; j < kEqPer; j++) {
            uint32_t tb, fr, tc;
            eq_tile_elem(j, lane, tb, fr, tc);
            const uint32_t f = i * kEqTile + fr;
            ahead[j] = (tb < a.n_buses && a.bus[tb].n_bands && f < N) ? a.in[(uint64_t)tb * 2u * N + 2u * (uint64_t)f + tc] : 0.0f;
        }
    };
    auto stage_tile = [&](const uint32_t i) {
#pragma unroll
        for (uint32_t j = 0; j < kEqPer; j++) {
            uint32_t tb, fr, tc;
            eq_tile_elem(j, lane, tb, fr, tc);
            xin[i & 1u][(tb * 2u + tc) * (kEqTile + 1u) + fr] = ahead[j];
        }
    };
    load_tile(0);
    stage_tile(0);
    for (uint32_t i = 0; i < tiles; i++) {
        if (i + 1u < tiles) load_tile(i + 1u);
        __syncthreads();
        const float *xr = xin[i & 1u] + row * (kEqTile + 1u);
        const uint32_t t0 = i * kEqTile, tend = t0 + kEqTile < steps ? t0 + kEqTile : steps;
        for (uint32_t tb = t0; tb < tend; tb += kEqUnroll) {
            float xs[kEqUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kEqUnroll; u++) xs[u] = xr[tb - t0 + u];
#ifdef S2R_EQ_SERIAL
#pragma unroll
            for (uint32_t u = 0; u < kEqUnroll; u++) {
                const uint32_t t = tb + u;
                if (!mine || t >= N) continue;
                float x = xs[u];
#pragma unroll
                for (uint32_t kk = 0; kk < S2R_EQ_MAX_BANDS; kk++)
                    if (kk < nb) { float n1, n2; x = eq_band(q[kk], x, s1[kk], s2[kk], n1, n2); s1[kk] = n1; s2[kk] = n2; }
                my_ring[t & (kEqRing - 1u)] = x;                 // (the serial form has no skew: frame t leaves at step t)
            }
#else
            if (tb >= sk && tb + kEqUnroll <= N) {               // every band of every cascade has a frame of the call at each of these steps
                float *const w = emit ? my_ring + (tb & (kEqRing - 1u)) : my_trash;      // (tb is a multiple of 8, and so is the ring: no wrap inside a block)
#pragma unroll
                for (uint32_t u = 0; u < kEqUnroll; u++) {
                    const float left = eq_from_left(y);
                    const float x = k == 0u ? xs[u] : left;
                    float n1, n2;
                    y = eq_band(q, x, s1, s2, n1, n2);
                    s1 = n1; s2 = n2;                            // (an idle lane computes on whatever it holds, and writes nothing)
                    w[u] = y;
                }
            } else {                                             // the pipeline fills or drains: a lane whose frame t - k is not of the call keeps its state
#pragma unroll
                for (uint32_t u = 0; u < kEqUnroll; u++) {
                    const float left = eq_from_left(y);
                    const float x = k == 0u ? xs[u] : left;
                    const uint32_t f = tb + u - k;               // (wraps past N for t < k)
                    const bool act = f < N;
                    float n1, n2;
                    y = eq_band(q, x, s1, s2, n1, n2);
                    s1 = act ? n1 : s1; s2 = act ? n2 : s2;
                    if (emit && act) my_ring[(tb + u) & (kEqRing - 1u)] = y;
                }
            }
#endif
        }
        __syncthreads();
        // frames [t0 - sk, t0 + T - sk) of the call are complete in the ring: every band has passed them.  (Their slots, steps
        // t0 - sk .. t0 + T - 1, are not written again before tile i + 2: the ring holds two tiles.)
        const int64_t f0 = (int64_t)t0 - (int64_t)sk;
        const int64_t hi = (int64_t)t0 + kEqTile - sk < (int64_t)N ? (int64_t)t0 + kEqTile - sk : (int64_t)N;
#pragma unroll
        for (uint32_t j = 0; j < kEqPer; j++) {
            uint32_t tb, fr, tc;
            eq_tile_elem(j, lane, tb, fr, tc);
            const int64_t f = f0 + fr;
            if (tb < a.n_buses && a.bus[tb].n_bands && f >= 0 && f < hi) {
#ifdef S2R_EQ_SERIAL
                const uint32_t left_at = (uint32_t)f;
#else
                const uint32_t left_at = (uint32_t)f + a.bus[tb].n_bands - 1u;
#endif
                a.out[(uint64_t)tb * 2u * N + 2u * (uint64_t)f + tc] = ring[(tb * 2u + tc) * (kEqRing + 1u) + (left_at & (kEqRing - 1u))];
            }
        }
        if (i + 1u < tiles) stage_tile(i + 1u);
    }
#ifdef S2R_EQ_SERIAL
#pragma unroll
    for (uint32_t kk = 0; kk < S2R_EQ_MAX_BANDS; kk++)
        if (mine && kk < nb) { a.bus[bus].next[4u * kk + ch] = s1[kk]; a.bus[bus].next[4u * kk + 2u + ch] = s2[kk]; }
#else
    if (mine) { a.bus[bus].next[4u * k + ch] = s1; a.bus[bus].next[4u * k + 2u + ch] = s2; }
#endif
}

hipError_t s2r_launch_bus_eq(const S2rEq &a, hipStream_t stream) {
    if (a.frames == 0 || a.n_buses == 0) return hipSuccess;
    if (a.n_buses > S2R_MAX_BUSES || !a.in || !a.out || a.in == a.out) return hipErrorInvalidValue;
    uint32_t depth = 0, plain = 0;
    for (uint32_t q = 0; q < a.n_buses; q++) {
        const S2rEqBus &b = a.bus[q];
        if (b.n_bands == 0) { plain++; continue; }
        if (b.n_bands > S2R_EQ_MAX_BANDS || !b.line || !b.next || b.line == b.next) return hipErrorInvalidValue;
        if (b.n_bands > depth) depth = b.n_bands;
    }
    if (depth == 0) return hipErrorInvalidValue;                 // (a call without an EQ does not come here)
    const dim3 grid = plain ? dim3(1u + (a.frames + kEqCopyFrames - 1u) / kEqCopyFrames, a.n_buses) : dim3(1u, 1u);
    hipLaunchKernelGGL(s2r_eq_kernel, grid, dim3(kEqLanes), 0, stream, a, depth);
    return hipGetLastError();
}
