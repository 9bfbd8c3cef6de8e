// s2r_flanger.hip — the per-bus flanger of s2r_fill_buses and s2r_fill_master, behind the drive in the post-mix chain: a
// modulated feedback comb.  Per frame n of a bus (x: the bus as it enters; w: the stage's line signal, negative indices its history),
// first for both channels c
//   p = phase + c * spread + phase_inc * n;   q = p >> 8;   h = q < 2^23 ? q : 2^24 - q;   m = (float)h * 2^-23
//   d = base + (depth * m);   i = (uint32)d;   f = d - (float)i
//   a = w_c[n - i];   bb = w_c[n - i - 1];   e = bb - a;   g = f * e;   tap_c = a + g
// then for both channels
//   w_c[n] = x_c[n] + ((feedback * tap_c) + (cross * tap_(1-c)));   y_c[n] = (dry * x_c[n]) + (wet * tap_c)
// binary32, every operation rounded on its own (-ffp-contract=off), denormals kept, nothing skipped for a zero or for f == 0.
// The recursion is real, but d >= base >= S2R_FLANGER_MIN_DELAY = 32: frame n reads w[n - i] and w[n - i - 1] with i >= 32, nothing
// younger than 33 frames.  Inside a tile of S2R_FLANGER_TILE = 32 frames every frame of both channels therefore reads only what earlier
// tiles wrote: 64 independent lanes, ONE wavefront per bus with a flanger, walking the call tile by tile (three more waves of its workgroup only help it carry
// the line in and out of LDS, behind one barrier each way); lane l owns channel l & 1 of
// frame l >> 1 of the tile, the order of the interleaved buffers.  The wave keeps the line's last 4096 frames — at least H, the history,
// which is at most 4096 — in LDS as a ring indexed by the frame's place in (history, then call) modulo 4096: loaded from the state once,
// read twice and written once per tile and lane, and copied out once at the end, its last H frames being the next state whether the call
// was longer than H or shorter (the old history's tail is still in the ring then, in front).  At H = 4096 frame n's oldest tap and its
// own w share a slot: the same lane reads it before it writes it, and no other lane of the tile touches it.
// The stage's critical path is (tiles) x (two LDS reads, e, g, tap, the lane exchange, two products' sum, w, the LDS write).  Everything
// that does not depend on w is off it: p, m, d, i, f and the three LDS addresses of tile t + 1 are computed while tile t's reads are in
// flight, x is loaded kFlAhead = 8 tiles ahead into registers, and dry * x waits there.  `cross` takes the other channel's tap of the
// same frame from the neighbouring lane (l ^ 1: a DPP move, no LDS, no memory).  LDS operations of one wave execute in issue order, so
// the walking wave needs no barrier between a tile's write and the next tile's reads; a wavefront-scope fence, which emits no instruction, keeps
// the compiler from moving one across the other.  The last tile may be partial: a lane past the call loads the call's last frame again, uses nothing of it and writes nothing.
// The kernel clamps i into [32, H - 1] — under the rule the clamp never acts —, so that no argument of the launcher makes a lane read
// outside the line's window or inside its own tile.  Each value sees exactly the rule's operations in the rule's order, so the output is
// the host loop's bit for bit.  Buses of the call without a flanger are copied by other workgroups of the same launch.  No atomics,
// nothing that waits for another workgroup, no inline assembly.
// -DS2R_FLANGER_SERIAL builds the obvious form for comparison (tools/flanger_time.py, CHANGELOG): one lane per bus and channel steps
// frame by frame, the line in global memory (the call's w overwrites x in the stage's own staging buffer).
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float fl2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kFlWave = 64u;                                // the wavefront that walks the call
#ifdef S2R_FLANGER_SERIAL
constexpr uint32_t kFlThreads = kFlWave;
#else
constexpr uint32_t kFlThreads = 256u;                            // with three more that help it carry the line in and out of LDS
#endif
constexpr uint32_t kFlLoad = 16u;                                // frames of the history a lane loads, all of them in flight at once
constexpr uint32_t kFlTile = S2R_FLANGER_TILE;
constexpr uint32_t kFlMinTap = 32u;                              // S2R_FLANGER_MIN_DELAY, as a frame count
constexpr uint32_t kFlRing = 4096u;                              // frames of the line in LDS: the largest H
constexpr uint32_t kFlMask = kFlRing - 1u;
constexpr uint32_t kFlAhead = 8u;                                // tiles the input is loaded ahead
constexpr uint32_t kFlCopyFrames = 4u * kFlThreads;              // frames per workgroup of the copy of a bus without a flanger
static_assert(2u * kFlTile == kFlWave, "a lane per channel and frame of a tile");
static_assert(256u * kFlLoad >= kFlRing, "the workgroup loads the longest history in one pass");
static_assert(kFlTile <= kFlMinTap, "no tap of a tile may reach into the tile");
static_assert((kFlRing & kFlMask) == 0u && (float)kFlRing >= S2R_FLANGER_MAX_DELAY + 1.0f && (float)kFlMinTap == S2R_FLANGER_MIN_DELAY, "the ring holds every history");

// what a lane knows of its frame of a tile before it has seen w
struct FlPrep {
    uint32_t aa, ab, wa;          // the ring's floats of w[n - i], w[n - i - 1] and w[n]
    float f;
};

// the rule's first three lines for channel c of frame n, and the places in the ring they lead to (frame n sits at H + n)
__device__ __forceinline__ FlPrep fl_prep(const S2rFlangerBus &b, const uint32_t H, const uint32_t c, const uint32_t n) {
    const uint32_t p = b.phase + c * b.spread + b.phase_inc * n;
    const uint32_t q = p >> 8;
    const uint32_t h = q < (1u << 23) ? q : (1u << 24) - q;
    const float m = (float)h * 0x1p-23f;
    const float dm = b.depth * m;
    const float d = b.base + dm;
    const uint32_t id = (uint32_t)d;
    const uint32_t i = id < kFlMinTap ? kFlMinTap : id > H - 1u ? H - 1u : id;   // (never acts under the rule)
    FlPrep r;
    r.f = d - (float)i;
    const uint32_t ja = H + n - i;                               // >= n + 1
    r.aa = 2u * (ja & kFlMask) + c;
    r.ab = 2u * ((ja - 1u) & kFlMask) + c;
    r.wa = 2u * ((H + n) & kFlMask) + c;
    return r;
}

// the value the neighbouring lane l ^ 1 holds: a DPP move inside the quad
__device__ __forceinline__ float fl_other(const float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1 /* quad_perm: [1, 0, 3, 2] */, 0xF, 0xF, false));
}

}  // namespace

// Workgroup (0, q) runs the flanger of bus q.  Workgroups (1 + g, q) exist when a bus of the call has none, and copy that bus from `in`
// to `out`, kFlCopyFrames frames each; every other workgroup returns at once.
__global__ void __launch_bounds__(kFlThreads) s2r_flanger_kernel(const S2rFlanger a) {
    const uint32_t lane = threadIdx.x, N = a.frames, q = blockIdx.y;
    const S2rFlangerBus &b = a.bus[q];
    if (blockIdx.x > 0) {
        if (b.line) return;                                      // (uniform: the whole workgroup)
        const fl2 *const x2 = reinterpret_cast<const fl2 *>(a.in) + (uint64_t)q * N;
        fl2 *const y2 = reinterpret_cast<fl2 *>(a.out) + (uint64_t)q * N;
        const uint32_t n0 = (blockIdx.x - 1u) * kFlCopyFrames;
        for (uint32_t n = n0 + lane; n < n0 + kFlCopyFrames && n < N; n += kFlThreads) y2[n] = x2[n];
        return;
    }
    if (!b.line) return;
    const uint32_t H = b.history < kFlMinTap + 1u ? kFlMinTap + 1u : b.history > kFlRing ? kFlRing : b.history;   // (the launcher's range)
    const uint32_t c = lane & 1u;
    const float feedback = b.feedback, cross = b.cross, dry = b.dry, wet = b.wet;
#ifdef S2R_FLANGER_SERIAL
    // lanes 0 and 1: a channel each, frame by frame; w[n] takes x[n]'s place in the staging buffer
    float *const xw = a.in + (uint64_t)q * N * 2u;
    float *const y = a.out + (uint64_t)q * N * 2u;
    if (lane < 2u) {
        for (uint32_t n = 0; n < N; n++) {
            const uint32_t p = b.phase + c * b.spread + b.phase_inc * n;
            const uint32_t qq = p >> 8;
            const uint32_t h = qq < (1u << 23) ? qq : (1u << 24) - qq;
            const float m = (float)h * 0x1p-23f;
            const float dm = b.depth * m;
            const float d = b.base + dm;
            const uint32_t id = (uint32_t)d;
            const uint32_t i = id < kFlMinTap ? kFlMinTap : id > H - 1u ? H - 1u : id;
            const float f = d - (float)i;
            const uint32_t ja = H + n - i;                       // the place in (history, then call) of w[n - i]
            const float va = ja < H ? b.line[2u * ja + c] : xw[2u * (size_t)(ja - H) + c];
            const float vb = ja - 1u < H ? b.line[2u * (ja - 1u) + c] : xw[2u * (size_t)(ja - 1u - H) + c];
            const float e = vb - va;
            const float g = f * e;
            const float tap = va + g;
            const float other = __shfl_xor(tap, 1);
            const float x = xw[2u * (size_t)n + c];
            const float pf = feedback * tap;
            const float pc = cross * other;
            const float s = pf + pc;
            xw[2u * (size_t)n + c] = x + s;
            const float dx = dry * x;
            const float wt = wet * tap;
            y[2u * (size_t)n + c] = dx + wt;
        }
        for (uint32_t m = 0; m < H; m++)                         // the next state: the last H frames of (history, then w)
            b.next[2u * m + c] = N + m < H ? b.line[2u * (N + m) + c] : xw[2u * (size_t)(N + m - H) + c];
    }
#else
    const uint32_t k = lane >> 1;
    const float *const x = a.in + (uint64_t)q * N * 2u;
    float *const y = a.out + (uint64_t)q * N * 2u;
    __shared__ __attribute__((aligned(16))) float ring[2u * kFlRing];
    {   // the history: frame m of it at slot m; every load of a lane is issued before the first is waited for
        const fl2 *const l2 = reinterpret_cast<const fl2 *>(b.line);
        fl2 *const r2 = reinterpret_cast<fl2 *>(ring);
        fl2 v[kFlLoad];
#pragma unroll
        for (uint32_t j = 0; j < kFlLoad; j++) { const uint32_t m = j * kFlThreads + lane; v[j] = l2[m < H ? m : H - 1u]; }
#pragma unroll
        for (uint32_t j = 0; j < kFlLoad; j++) { const uint32_t m = j * kFlThreads + lane; if (m < H) r2[m] = v[j]; }
    }
    __syncthreads();
    if (lane < kFlWave) {                                        // (uniform: the first wave, whole)
    const uint32_t tiles = (N + kFlTile - 1u) / kFlTile;
    // the input of the first kFlAhead tiles; lane l's float of tile t is float 64 t + l of the bus
    float xq[kFlAhead];
#pragma unroll
    for (uint32_t u = 0; u < kFlAhead; u++) {
        const uint32_t n = u * kFlTile + k;
        xq[u] = x[2u * (size_t)(n < N ? n : N - 1u) + c];         // (a lane past the call loads the call's last frame, and uses nothing of it)
    }
    FlPrep cur = fl_prep(b, H, c, k);
    // one tile: frame n of this lane, its input xv; `full`: the whole tile lies inside the call
    auto tile = [&](const uint32_t n, const float xv, const bool full) {
        const float va = ring[cur.aa], vb = ring[cur.ab];        // on the path: the two reads ...
        const float dx = dry * xv;                               // ... and beside it this tile's dry part and tile t + 1's places
        const FlPrep nxt = fl_prep(b, H, c, n + kFlTile);
        const float e = vb - va;
        const float g = cur.f * e;
        const float tap = va + g;
        const float other = fl_other(tap);                       // the other channel's tap of the same frame
        const float pf = feedback * tap;
        const float pc = cross * other;
        const float s = pf + pc;
        const float w = xv + s;
        if (full || n < N) ring[cur.wa] = w;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the next tile's reads stay behind this write
        const float wt = wet * tap;
        if (full || n < N) y[2u * (size_t)n + c] = dx + wt;
        cur = nxt;
    };
    // groups of kFlAhead whole tiles: a group's loads of the NEXT group's input come first and stay there, a whole group ahead of their use ...
    const uint32_t groups = (N / kFlTile) / kFlAhead;
    uint32_t n = k;
    for (uint32_t g = 0; g < groups; g++) {
        float xn[kFlAhead];
#pragma unroll
        for (uint32_t u = 0; u < kFlAhead; u++) {
            const uint32_t nl = n + (kFlAhead + u) * kFlTile;
            xn[u] = x[2u * (size_t)(nl < N ? nl : N - 1u) + c];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (uint32_t u = 0; u < kFlAhead; u++) {
            tile(n, xq[u], true);
            n += kFlTile;
        }
#pragma unroll
        for (uint32_t u = 0; u < kFlAhead; u++) xq[u] = xn[u];
    }
    // ... and the call's last tiles, fewer than kFlAhead whole ones and a partial one, whose inputs are all loaded
#pragma unroll
    for (uint32_t u = 0; u < kFlAhead; u++) {
        if (groups * kFlAhead + u < tiles) {                     // (uniform)
            tile(n, xq[u], false);
            n += kFlTile;
        }
    }
    }
    __syncthreads();
    {   // the next state: the last H frames of (history, then w), places N .. N + H - 1, all of them in the ring
        fl2 *const n2 = reinterpret_cast<fl2 *>(b.next);
        const fl2 *const r2 = reinterpret_cast<const fl2 *>(ring);
        for (uint32_t m = lane; m < H; m += kFlThreads) n2[m] = r2[(N + m) & kFlMask];
    }
#endif
}

hipError_t s2r_launch_bus_flanger(const S2rFlanger &a, hipStream_t stream) {
    if (a.frames == 0 || a.n_buses == 0) return hipSuccess;
    if (a.n_buses > S2R_MAX_BUSES || !a.in || !a.out || a.in == a.out) return hipErrorInvalidValue;
    uint32_t active = 0, plain = 0;
    for (uint32_t q = 0; q < a.n_buses; q++) {
        const S2rFlangerBus &b = a.bus[q];
        if (!b.line) { plain++; continue; }
        if (!b.next || b.line == b.next || b.history < kFlMinTap + 1u || b.history > kFlRing) return hipErrorInvalidValue;
        active++;
    }
    if (active == 0) return hipErrorInvalidValue;                // (a call without a flanger does not come here)
    const dim3 grid = plain ? dim3(1u + (a.frames + kFlCopyFrames - 1u) / kFlCopyFrames, a.n_buses) : dim3(1u, a.n_buses);
    hipLaunchKernelGGL(s2r_flanger_kernel, grid, dim3(kFlThreads), 0, stream, a);
    return hipGetLastError();
}
