// s2r_dyn.hip — the per-bus dynamics of s2r_fill_buses and s2r_fill_master, behind the EQ in the post-mix chain: a
// sidechain compressor.  Per frame n of a bus with key bus k:
//   p = max(|x_kL|, |x_kR|);   t = the curve at p, by table and one linear step (dyn_target below);
//   a = (t < y) ? a_att : a_rel;   y = t + (a * (y - t));   out_c = x_c * y
// binary32, every operation rounded on its own (-ffp-contract=off), denormals kept, nothing skipped for a zero.  Only the third line
// needs frame n - 1, and its coefficient depends on the direction of the move, so no scan removes the recursion.  The kernel is a
// software pipeline of three stages inside ONE workgroup per bus with dynamics (buses are independent: they run on different CUs), a
// tile of S2R_DYN_TILE frames apart: in pass j the PRODUCER — one lane per frame, waves 1 .. 4 — turns the key bus's frames of tile j
// into targets in LDS (coalesced float2 loads; the curve sits in LDS); the WALKER — lane 0 of wave 0, alone in its wave — walks tile
// j - 1: it takes the targets eight at a time from LDS into registers a block ahead of the chain, carries y and the running minimum
// in registers and leaves y[n] in LDS; the CONSUMER — the producer's lanes — multiplies tile j - 2 of the bus by its y[n] (coalesced
// loads and stores).  Targets and gains are double-buffered, so one barrier per pass suffices, and memory stays off the dependent
// chain.  The pipeline fills and drains over two extra passes; the last tile may be partial: a lane past the call computes on what it
// holds and writes nothing.  Each frame sees exactly the rule's operations in the rule's order, so the output is the host loop's bit
// for bit.  The final y goes to the state's other copy, the minimum to the pinned meter row.  Buses of the call without dynamics (or
// with idle ones) are copied by other workgroups of the same launch.  No atomics, nothing that waits for another workgroup.
// -DS2R_DYN_SERIAL builds the obvious form for comparison (tools/dyn_time.py, CHANGELOG): one thread per bus does all four steps.
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float dyn2 __attribute__((ext_vector_type(2)));
typedef float dyn4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kDynTile = S2R_DYN_TILE;                      // frames per pipeline stage: one per producer / consumer lane
constexpr uint32_t kDynThreads = 64u + kDynTile;                 // the walker's wave, then a lane per frame of a tile
constexpr uint32_t kDynBlock = 8;                                // targets the walker reads from LDS ahead of their chain
constexpr uint32_t kDynCopyFrames = 4u * kDynThreads;            // frames per workgroup of the copy of a bus without dynamics
constexpr uint32_t kDynLo = 0x33800000u;                         // the bits of 2^-24; 2^8 is kDynLo + (512 << 19)
static_assert(kDynTile % (2u * kDynBlock) == 0u && kDynThreads <= 1024u, "whole blocks of targets, and one workgroup");

// the rule's step 2: the target gain at level p >= 0 (a NaN, outside the contract, reads curve[0])
__device__ __forceinline__ float dyn_target(const float *curve, const float p) {
    const uint32_t u = __float_as_uint(p) - kDynLo;
    const uint32_t i = (p >= 5.9604644775390625e-08f && p < 256.0f) ? u >> 19 : 0u;      // (in range whatever p holds)
    const float f = (float)(u & 0x7ffffu) * 1.9073486328125e-06f;
    const float c0 = curve[i], c1 = curve[i + 1u];
    const float d = c1 - c0;
    const float m = f * d;
    const float t = c0 + m;
    return !(p >= 5.9604644775390625e-08f) ? curve[0] : (p >= 256.0f ? curve[S2R_DYN_CURVE_POINTS - 1u] : t);
}

__device__ __forceinline__ float dyn_level(const dyn2 k) {
    const float l = __builtin_fabsf(k.x), r = __builtin_fabsf(k.y);
    return l > r ? l : r;
}

// the rule's step 3, and the meter
__device__ __forceinline__ void dyn_step(const float t, const float a_att, const float a_rel, float &y, float &mn) {
    const float a = t < y ? a_att : a_rel;
    const float d = y - t;
    const float m = a * d;
    y = t + m;
    mn = y < mn ? y : mn;
}

}  // namespace

// Workgroup (0, q) runs the dynamics of bus q.  Workgroups (1 + g, q) exist when a bus of the call runs none, and copy that bus from
// `in` to `out`, kDynCopyFrames frames each; every other workgroup returns at once.
__global__ void __launch_bounds__(kDynThreads) s2r_dyn_kernel(const S2rDyn a) {
    const uint32_t tid = threadIdx.x, N = a.frames, q = blockIdx.y;
    const S2rDynBus &b = a.bus[q];
    const dyn2 *const x2 = reinterpret_cast<const dyn2 *>(a.in) + (uint64_t)q * N;
    dyn2 *const y2 = reinterpret_cast<dyn2 *>(a.out) + (uint64_t)q * N;
    if (blockIdx.x > 0) {
        if (b.curve) return;                                     // (uniform: the whole workgroup)
        const uint32_t n0 = (blockIdx.x - 1u) * kDynCopyFrames;
        for (uint32_t n = n0 + tid; n < n0 + kDynCopyFrames && n < N; n += kDynThreads) y2[n] = x2[n];
        return;
    }
    if (!b.curve) return;
    const dyn2 *const k2 = reinterpret_cast<const dyn2 *>(a.in) + (uint64_t)b.key * N;
    const float a_att = b.a_att, a_rel = b.a_rel;
#ifdef S2R_DYN_SERIAL
    if (tid != 0) return;
    float y = b.line[0], mn = __builtin_inff();
    for (uint32_t n = 0; n < N; n++) {
        const float t = dyn_target(b.curve, dyn_level(k2[n]));
        dyn_step(t, a_att, a_rel, y, mn);
        const dyn2 x = x2[n];
        y2[n] = dyn2{x.x * y, x.y * y};
    }
    b.next[0] = y;
    a.meter[q] = mn;
#else
    __shared__ __attribute__((aligned(16))) float curve[S2R_DYN_CURVE_POINTS + 3u];
    __shared__ __attribute__((aligned(16))) float tg[2][kDynTile];       // targets: the tile being walked and the tile being produced
    __shared__ __attribute__((aligned(16))) float yg[2][kDynTile];       // gains: the tile being walked and the tile being applied
    for (uint32_t j = tid; j < S2R_DYN_CURVE_POINTS; j += kDynThreads) curve[j] = b.curve[j];
    __syncthreads();
    const bool walker = tid == 0u, worker = tid >= 64u;
    const uint32_t w = tid - 64u;                                // a worker's frame of a tile
    const uint32_t tiles = (N + kDynTile - 1u) / kDynTile;
    float y = b.line[0], mn = __builtin_inff();                  // (the walker's)
    for (uint32_t j = 0; j < tiles + 2u; j++) {
        if (worker) {
            dyn2 k = dyn2{0.0f, 0.0f}, x = dyn2{0.0f, 0.0f};
            const uint32_t np = j * kDynTile + w, nc = (j - 2u) * kDynTile + w;      // (nc wraps past N for j < 2)
            const bool produce = j < tiles, consume = j >= 2u && nc < N;
            if (produce && np < N) k = k2[np];
            if (consume) x = x2[nc];
            if (produce) tg[j & 1u][w] = dyn_target(curve, dyn_level(k));             // (past the call: the target of silence, never walked)
            if (consume) { const float g = yg[j & 1u][w]; y2[nc] = dyn2{x.x * g, x.y * g}; }
        } else if (walker && j >= 1u && j <= tiles) {
            const uint32_t t0 = (j - 1u) * kDynTile, cnt = N - t0 < kDynTile ? N - t0 : kDynTile;
            const float *const tp = tg[(j - 1u) & 1u];
            float *const yp = yg[(j - 1u) & 1u];
            const dyn4 *const tp4 = reinterpret_cast<const dyn4 *>(tp);
            dyn4 *const yp4 = reinterpret_cast<dyn4 *>(yp);
            dyn4 c0 = tp4[0], c1 = tp4[1];
            uint32_t k = 0;
            for (; k + kDynBlock <= cnt; k += kDynBlock) {
                const uint32_t nx = k + kDynBlock < kDynTile ? k + kDynBlock : k;    // the next block, read ahead (the last one: itself again)
                const dyn4 n0 = tp4[nx / 4u], n1 = tp4[nx / 4u + 1u];
                dyn4 g0, g1;
                dyn_step(c0.x, a_att, a_rel, y, mn); g0.x = y;
                dyn_step(c0.y, a_att, a_rel, y, mn); g0.y = y;
                dyn_step(c0.z, a_att, a_rel, y, mn); g0.z = y;
                dyn_step(c0.w, a_att, a_rel, y, mn); g0.w = y;
                dyn_step(c1.x, a_att, a_rel, y, mn); g1.x = y;
                dyn_step(c1.y, a_att, a_rel, y, mn); g1.y = y;
                dyn_step(c1.z, a_att, a_rel, y, mn); g1.z = y;
                dyn_step(c1.w, a_att, a_rel, y, mn); g1.w = y;
                yp4[k / 4u] = g0; yp4[k / 4u + 1u] = g1;
                c0 = n0; c1 = n1;
            }
            for (; k < cnt; k++) { dyn_step(tp[k], a_att, a_rel, y, mn); yp[k] = y; }     // the call's last frames, fewer than a block
        }
        __syncthreads();
    }
    if (walker) { b.next[0] = y; a.meter[q] = mn; }
#endif
}

hipError_t s2r_launch_bus_dyn(const S2rDyn &a, hipStream_t stream) {
    if (a.frames == 0 || a.n_buses == 0) return hipSuccess;
    if (a.n_buses > S2R_MAX_BUSES || !a.in || !a.out || a.in == a.out || !a.meter) return hipErrorInvalidValue;
    uint32_t active = 0, plain = 0;
    for (uint32_t q = 0; q < a.n_buses; q++) {
        const S2rDynBus &b = a.bus[q];
        if (!b.curve) { plain++; continue; }
        if (!b.line || !b.next || b.line == b.next || b.key >= a.n_buses) return hipErrorInvalidValue;
        active++;
    }
    if (active == 0) return hipErrorInvalidValue;                // (a call without dynamics does not come here)
    const dim3 grid = plain ? dim3(1u + (a.frames + kDynCopyFrames - 1u) / kDynCopyFrames, a.n_buses) : dim3(1u, a.n_buses);
    hipLaunchKernelGGL(s2r_dyn_kernel, grid, dim3(kDynThreads), 0, stream, a);
    return hipGetLastError();
}
