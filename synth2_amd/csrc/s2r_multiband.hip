// s2r_multiband.hip — the master's multiband compressor of s2r_fill_master, behind the master kernel and in front of the
// limiter: a tree of crossover sections splits the master into B bands, every band gets a gain of its own by the bus dynamics' rule, and
// the bands are added in band order.  A section is the bus EQ's band, per channel c:
//   y = (b0 * x) + s1;   s1' = ((b1 * x) - (a1 * y)) + s2;   s2' = (b2 * x) - (a2 * y)
// and a band's gain the bus dynamics', per frame: p = max(|band_L|, |band_R|); t = the curve at p; a = (t < y) ? a_att : a_rel;
// y = t + (a * (y - t)); o_c = band_c * y.  binary32, every operation rounded on its own (-ffp-contract=off), denormals kept, nothing
// skipped for a zero.  Every section and every gain needs frame n - 1, and a frame passes up to six sections and a gain: one thread per
// channel would run some 15 x 9 dependent operations a frame.  The kernel is ONE workgroup of four parts, a tile of S2R_MULTIBAND_TILE
// frames apart, with one barrier per pass:
//   the CROSSOVER WAVE — wave 0, one lane per (channel, section), up to 30 — is systolic: a lane `depth` sections behind the input works
//   kMbEdge * depth frames behind it and takes its x from the lane in front of it by ds_bpermute.  A value is sent at the end of the step
//   that made it and used two steps later, so that the move's latency is off every dependent chain: a step costs a lane the recurrence
//   of ONE section.  The input comes from LDS, staged a tile ahead by the worker lanes and read eight steps at a time; the lanes that
//   leave a band put it into an LDS ring at slot frame + kMbSkew, so that a slot is complete once the steps up to it have run;
//   the PRODUCER — the worker lanes, a frame each — turns the four bands of the tile behind that into targets, the curves in LDS;
//   the WALKERS — lanes 0 .. B - 1 of wave 1, in lockstep — walk the tile behind that: targets eight at a time from LDS into registers,
//   y and the running minimum in registers, y[n] left in LDS;
//   the CONSUMER — the worker lanes again — multiplies the tile behind that by its gains, adds the bands in band order and stores
//   float2, coalesced.
// Each lane does exactly the rule's operations in the rule's order, so the output is the host loop's bit for bit.  A lane whose frame is
// not of the call (the pipeline fills or drains) keeps its state and writes nothing.  The state's other copy receives every section's
// (s1, s2) and every band's y, the pinned meter row the minima.  No atomics, nothing that waits for another workgroup.
// -DS2R_MULTIBAND_SERIAL builds the obvious form for comparison (tools/multiband_time.py, CHANGELOG): a lane per channel runs every
// section of a frame, then the four gains.
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float mb2 __attribute__((ext_vector_type(2)));
typedef float mb4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kMbTile = S2R_MULTIBAND_TILE;                 // frames per pipeline stage: one per worker lane
constexpr uint32_t kMbThreads = 128u + kMbTile;                  // the crossover wave, the walkers' wave, then a lane per frame of a tile
constexpr uint32_t kMbEdge = 2;                                  // steps between a section and the section behind it
constexpr uint32_t kMbMaxDepth = 5;                              // the deepest section of four bands has five in front of it
constexpr uint32_t kMbLagMax = kMbEdge * kMbMaxDepth;            // the most steps a lane works behind the input
constexpr uint32_t kMbSkew = 16;                                 // a band's frame f lies at slot f + kMbSkew of the ring
constexpr uint32_t kMbRing = 8u * kMbTile;                       // slots of the ring: the tiles under way in four stages, and a power of two
constexpr uint32_t kMbBlock = 8;                                 // inputs and targets read from LDS ahead of their chains
constexpr uint32_t kMbLo = 0x33800000u;                          // the bits of 2^-24; 2^8 is kMbLo + (512 << 19)
constexpr uint32_t kMbCurveRow = S2R_DYN_CURVE_POINTS + 3u;
static_assert(kMbSkew >= kMbLagMax && kMbSkew % kMbBlock == 0u && kMbTile % (2u * kMbBlock) == 0u, "whole blocks in front of the first slot and in a tile");
static_assert((kMbRing & (kMbRing - 1u)) == 0u && kMbThreads <= 1024u && S2R_MULTIBAND_MAX_BANDS == 4u, "the ring is masked; one workgroup; four walkers");

struct MbSection { float b0, b1, b2, a1, a2; };

// one section, one frame: the rule's nine operations
__device__ __forceinline__ float mb_section(const MbSection &q, const float x, const float s1, const float s2, float &n1, float &n2) {
    const float p0 = q.b0 * x;
    const float y = p0 + s1;
    const float p1 = q.b1 * x, r1 = q.a1 * y;
    const float d1 = p1 - r1;
    const float p2 = q.b2 * x, r2 = q.a2 * y;
    n1 = d1 + s2;
    n2 = p2 - r2;
    return y;
}

// the dynamics' step 2: the target gain at level p >= 0 (a NaN, outside the contract, reads curve[0])
__device__ __forceinline__ float mb_target(const float *curve, const float p) {
    const uint32_t u = __float_as_uint(p) - kMbLo;
    const uint32_t i = (p >= 5.9604644775390625e-08f && p < 256.0f) ? u >> 19 : 0u;      // (in range whatever p holds)
    const float f = (float)(u & 0x7ffffu) * 1.9073486328125e-06f;
    const float c0 = curve[i], c1 = curve[i + 1u];
    const float d = c1 - c0;
    const float m = f * d;
    const float t = c0 + m;
    return !(p >= 5.9604644775390625e-08f) ? curve[0] : (p >= 256.0f ? curve[S2R_DYN_CURVE_POINTS - 1u] : t);
}

__device__ __forceinline__ float mb_level(const float xl, const float xr) {
    const float l = __builtin_fabsf(xl), r = __builtin_fabsf(xr);
    return l > r ? l : r;
}

// the dynamics' step 3, and the meter
__device__ __forceinline__ void mb_step(const float t, const float a_att, const float a_rel, float &y, float &mn) {
    const float a = t < y ? a_att : a_rel;
    const float d = y - t;
    const float m = a * d;
    y = t + m;
    mn = y < mn ? y : mn;
}

#ifdef S2R_MULTIBAND_SERIAL
// The obvious form: lane c of the wave runs channel c's sections in the state's order, takes the other channel's band values from its
// neighbour, and walks the four gains (both lanes the same walk), frame by frame from global memory.
// (75 uniform coefficients would not fit the scalar registers and would be spilled from them: they are kept in vector registers)
__device__ __forceinline__ float mb_in_vgpr(const float x) {
    float v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
    return v;
}
template <uint32_t B> __device__ void mb_serial(const S2rMultiband &a, const uint32_t c) {
    constexpr uint32_t S = S2R_MULTIBAND_SECTIONS(B);
    MbSection q[S ? S : 1u];
    float s1[S ? S : 1u], s2[S ? S : 1u], y[B], mn[B], att[B], rel[B];
#pragma unroll
    for (uint32_t i = 0; i < S; i++) {
        q[i] = MbSection{mb_in_vgpr(a.c[i][0]), mb_in_vgpr(a.c[i][1]), mb_in_vgpr(a.c[i][2]), mb_in_vgpr(a.c[i][3]), mb_in_vgpr(a.c[i][4])};
        s1[i] = a.state[4u * i + c]; s2[i] = a.state[4u * i + 2u + c];
    }
#pragma unroll
    for (uint32_t j = 0; j < B; j++) { y[j] = a.state[4u * S + j]; mn[j] = __builtin_inff(); att[j] = mb_in_vgpr(a.a_att[j]); rel[j] = mb_in_vgpr(a.a_rel[j]); }
    auto run = [&](const uint32_t i, const float x) {
        float n1, n2;
        const float v = mb_section(q[i], x, s1[i], s2[i], n1, n2);
        s1[i] = n1; s2[i] = n2;
        return v;
    };
    for (uint32_t n = 0; n < a.frames; n++) {
        float band[B];
        float r = a.in[2u * (uint64_t)n + c];
#pragma unroll
        for (uint32_t k = 0; k + 1u < B; k++) {
            band[k] = run(4u * k + 1u, run(4u * k, r));
            r = run(4u * k + 3u, run(4u * k + 2u, r));
        }
        band[B - 1u] = r;
        uint32_t at = 4u * (B - 1u);
#pragma unroll
        for (uint32_t j = 0; j + 2u < B; j++)
#pragma unroll
            for (uint32_t k = j + 1u; k + 1u < B; k++) band[j] = run(at++, band[j]);
        float out = 0.0f;
#pragma unroll
        for (uint32_t j = 0; j < B; j++) {
            const float other = __shfl_xor(band[j], 1);
            const float t = mb_target(a.curves + (size_t)j * S2R_DYN_CURVE_POINTS, mb_level(band[j], other));
            mb_step(t, att[j], rel[j], y[j], mn[j]);
            const float o = band[j] * y[j];
            out = j ? out + o : o;
        }
        a.out[2u * (uint64_t)n + c] = out;
    }
#pragma unroll
    for (uint32_t i = 0; i < S; i++) { a.next[4u * i + c] = s1[i]; a.next[4u * i + 2u + c] = s2[i]; }
    if (c == 0u) {
#pragma unroll
        for (uint32_t j = 0; j < B; j++) { a.next[4u * S + j] = y[j]; a.meter[j] = mn[j]; }
    }
}
#endif

}  // namespace

__global__ void __launch_bounds__(kMbThreads) s2r_multiband_kernel(const S2rMultiband a) {
    const uint32_t tid = threadIdx.x, N = a.frames, B = a.n_bands, S = a.n_sections;
#ifdef S2R_MULTIBAND_SERIAL
    if (tid >= 2u) return;
    if (B == 1u) mb_serial<1>(a, tid);
    else if (B == 2u) mb_serial<2>(a, tid);
    else if (B == 3u) mb_serial<3>(a, tid);
    else mb_serial<4>(a, tid);
#else
    __shared__ __attribute__((aligned(16))) float curve[S2R_MULTIBAND_MAX_BANDS][kMbCurveRow];
    __shared__ __attribute__((aligned(16))) float xin[2][2][kMbTile];                       // the input, two tiles, a row per channel
    __shared__ __attribute__((aligned(16))) mb2 ring[S2R_MULTIBAND_MAX_BANDS][kMbRing];     // the bands in front of the gains: [band][slot] (L, R)
    __shared__ __attribute__((aligned(16))) float tg[2][S2R_MULTIBAND_MAX_BANDS][kMbTile];  // targets: the tile being walked and the tile being produced
    __shared__ __attribute__((aligned(16))) float yg[2][S2R_MULTIBAND_MAX_BANDS][kMbTile];  // gains: the tile being walked and the tile being applied
    __shared__ float trash[64];                                  // where a crossover lane that leaves no band writes, so that the store needs no branch
    for (uint32_t j = tid; j < B * S2R_DYN_CURVE_POINTS; j += kMbThreads) curve[j / S2R_DYN_CURVE_POINTS][j % S2R_DYN_CURVE_POINTS] = a.curves[j];
    __syncthreads();

    const mb2 *const in2 = reinterpret_cast<const mb2 *>(a.in);
    mb2 *const out2 = reinterpret_cast<mb2 *>(a.out);
    const uint32_t steps = N + kMbLagMax;                        // of the crossover wave: the deepest lane's last frame
    const uint32_t tiles_x = (steps + kMbTile - 1u) / kMbTile, tiles_s = (N + kMbSkew + kMbTile - 1u) / kMbTile;

    // the crossover wave's lanes: lane ch * 16 + sec.  With one band there is no section: lane `ch * 16` passes x on as band 0.
    const uint32_t ch = (tid >> 4) & 1u, sec = tid & 15u;
    const bool xwave = tid < 64u;
    const bool mine = tid < 32u && sec < S, ident = tid < 32u && S == 0u && sec == 0u;
    const uint32_t si = mine ? sec : 0u;
    const MbSection q = mine ? MbSection{a.c[si][0], a.c[si][1], a.c[si][2], a.c[si][3], a.c[si][4]} : MbSection{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float s1 = mine ? a.state[4u * si + ch] : 0.0f, s2 = mine ? a.state[4u * si + 2u + ch] : 0.0f;
    const int32_t from = mine ? a.src[si] : -1;
    const bool root = from < 0;
    const int src_addr = (int)((ch * 16u + (root ? sec : (uint32_t)from)) * 4u);        // ds_bpermute's byte address of the lane in front
    const uint32_t lag = mine ? kMbEdge * a.depth[si] : 0u;
    int32_t band = -1;
    for (uint32_t j = 0; j < B; j++) if ((mine && a.leaf[j] == (int32_t)sec) || (ident && a.leaf[j] < 0)) band = (int32_t)j;
    const bool emit = band >= 0;
    float *const my_ring = reinterpret_cast<float *>(ring[emit ? band : 0]) + ch;          // slot s of it: my_ring[2 s]
    float inbox = 0.0f, flight = 0.0f;                           // what the lane in front made two steps ago, and one step ago

    // the walkers: lane j of wave 1 carries y_j
    const uint32_t wl = tid - 64u;
    const bool walker = tid >= 64u && wl < B;
    const float a_att = walker ? a.a_att[wl] : 0.0f, a_rel = walker ? a.a_rel[wl] : 0.0f;
    float y = walker ? a.state[4u * S + wl] : 0.0f, mn = __builtin_inff();

    const bool worker = tid >= 128u;
    const uint32_t w = tid - 128u;                               // a worker's frame of a tile

    for (uint32_t j = 0; j < tiles_s + 4u; j++) {
        if (worker) {
            if (j * kMbTile < N) {                               // the input of tile j
                const uint32_t n = j * kMbTile + w;
                const mb2 v = n < N ? in2[n] : mb2{0.0f, 0.0f};
                xin[j & 1u][0][w] = v.x; xin[j & 1u][1][w] = v.y;
            }
            if (j >= 2u && j - 2u < tiles_s) {                   // the targets of slots [(j - 2) T, (j - 1) T)
                const uint32_t u = (j - 2u) * kMbTile + w, f = u - kMbSkew;              // (f wraps past N for u < kMbSkew)
                if (f < N) {
#pragma unroll
                    for (uint32_t jb = 0; jb < S2R_MULTIBAND_MAX_BANDS; jb++)
                        if (jb < B) { const mb2 v = ring[jb][u & (kMbRing - 1u)]; tg[j & 1u][jb][w] = mb_target(curve[jb], mb_level(v.x, v.y)); }
                }
            }
            if (j >= 4u && j - 4u < tiles_s) {                   // the outputs of slots [(j - 4) T, (j - 3) T)
                const uint32_t u = (j - 4u) * kMbTile + w, f = u - kMbSkew;
                if (f < N) {
                    mb2 acc = mb2{0.0f, 0.0f};
#pragma unroll
                    for (uint32_t jb = 0; jb < S2R_MULTIBAND_MAX_BANDS; jb++)
                        if (jb < B) {
                            const mb2 v = ring[jb][u & (kMbRing - 1u)];
                            const float g = yg[j & 1u][jb][w];
                            const mb2 o = mb2{v.x * g, v.y * g};
                            acc = jb ? mb2{acc.x + o.x, acc.y + o.y} : o;
                        }
                    out2[f] = acc;
                }
            }
        } else if (xwave) {
            if (j >= 1u && j - 1u < tiles_x) {                   // steps [(j - 1) T, j T): the lane works on frame step - lag
                const uint32_t i = j - 1u, t0 = i * kMbTile, tend = t0 + kMbTile < steps ? t0 + kMbTile : steps;
                const float *const xr = xin[i & 1u][ch];
                for (uint32_t tb = t0; tb < tend; tb += kMbBlock) {
                    float xs[kMbBlock];
#pragma unroll
                    for (uint32_t u = 0; u < kMbBlock; u++) xs[u] = xr[tb - t0 + u];
                    const uint32_t slot0 = tb - lag + kMbSkew;   // the slot of the lane's frame at the block's first step
                    if (tb >= kMbLagMax && tb + kMbBlock <= N) { // every lane has a frame of the call at each of these steps
#pragma unroll
                        for (uint32_t u = 0; u < kMbBlock; u++) {
                            const float x = root ? xs[u] : inbox;
                            float n1, n2;
                            const float v = mb_section(q, x, s1, s2, n1, n2);
                            const float yo = ident ? x : v;
                            s1 = n1; s2 = n2;                    // (an idle lane computes on whatever it holds, and writes nothing that is read)
                            float *const at = emit ? my_ring + 2u * ((slot0 + u) & (kMbRing - 1u)) : trash + tid;
                            *at = yo;
                            inbox = flight;
                            flight = __int_as_float(__builtin_amdgcn_ds_bpermute(src_addr, __float_as_int(yo)));
                        }
                    } else {                                     // the pipeline fills or drains: a lane whose frame is not of the call keeps its state
#pragma unroll
                        for (uint32_t u = 0; u < kMbBlock; u++) {
                            const float x = root ? xs[u] : inbox;
                            const uint32_t f = tb + u - lag;     // (wraps past N for a step in front of the lane's first)
                            const bool act = f < N;
                            float n1, n2;
                            const float v = mb_section(q, x, s1, s2, n1, n2);
                            const float yo = ident ? x : v;
                            s1 = act ? n1 : s1; s2 = act ? n2 : s2;
                            if (emit && act) my_ring[2u * ((slot0 + u) & (kMbRing - 1u))] = yo;
                            inbox = flight;
                            flight = __int_as_float(__builtin_amdgcn_ds_bpermute(src_addr, __float_as_int(yo)));
                        }
                    }
                }
            }
        } else if (walker && j >= 3u && j - 3u < tiles_s) {      // slots [(j - 3) T, (j - 2) T), as far as they hold frames of the call
            const uint32_t i = j - 3u, u0 = i * kMbTile;
            const uint32_t lo = i == 0u ? kMbSkew : 0u, hi = N + kMbSkew - u0 < kMbTile ? N + kMbSkew - u0 : kMbTile;
            const float *const tp = tg[i & 1u][wl];
            float *const yp = yg[i & 1u][wl];
            const mb4 *const tp4 = reinterpret_cast<const mb4 *>(tp);
            mb4 *const yp4 = reinterpret_cast<mb4 *>(yp);
            uint32_t k = lo;
            if (k + kMbBlock <= hi) {
                mb4 c0 = tp4[k / 4u], c1 = tp4[k / 4u + 1u];
                for (; k + kMbBlock <= hi; k += kMbBlock) {
                    const uint32_t nx = k + kMbBlock < kMbTile ? k + kMbBlock : k;       // the next block, read ahead (the last one: itself again)
                    const mb4 n0 = tp4[nx / 4u], n1 = tp4[nx / 4u + 1u];
                    mb4 g0, g1;
                    mb_step(c0.x, a_att, a_rel, y, mn); g0.x = y;
                    mb_step(c0.y, a_att, a_rel, y, mn); g0.y = y;
                    mb_step(c0.z, a_att, a_rel, y, mn); g0.z = y;
                    mb_step(c0.w, a_att, a_rel, y, mn); g0.w = y;
                    mb_step(c1.x, a_att, a_rel, y, mn); g1.x = y;
                    mb_step(c1.y, a_att, a_rel, y, mn); g1.y = y;
                    mb_step(c1.z, a_att, a_rel, y, mn); g1.z = y;
                    mb_step(c1.w, a_att, a_rel, y, mn); g1.w = y;
                    yp4[k / 4u] = g0; yp4[k / 4u + 1u] = g1;
                    c0 = n0; c1 = n1;
                }
            }
            for (; k < hi; k++) { mb_step(tp[k], a_att, a_rel, y, mn); yp[k] = y; }      // the call's last frames, fewer than a block
        }
        __syncthreads();
    }
    if (mine) { a.next[4u * sec + ch] = s1; a.next[4u * sec + 2u + ch] = s2; }
    if (walker) { a.next[4u * S + wl] = y; a.meter[wl] = mn; }
#endif
}

hipError_t s2r_launch_multiband(const S2rMultiband &a, hipStream_t stream) {
    if (a.frames == 0) return hipSuccess;
    if (a.n_bands < 1u || a.n_bands > S2R_MULTIBAND_MAX_BANDS || a.n_sections != S2R_MULTIBAND_SECTIONS(a.n_bands) || !a.in || !a.out || a.in == a.out ||
        !a.state || !a.next || a.state == a.next || !a.curves || !a.meter)
        return hipErrorInvalidValue;
    for (uint32_t i = 0; i < a.n_sections; i++)                  // a section's input lies in front of it, and no lane works further behind than the ring allows
        if (a.src[i] >= (int32_t)i || a.src[i] < -1 || a.depth[i] > 5u) return hipErrorInvalidValue;
    for (uint32_t j = 0; j < a.n_bands; j++)
        if (a.leaf[j] >= (int32_t)a.n_sections || a.leaf[j] < -1 || (a.leaf[j] < 0) != (a.n_sections == 0u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(s2r_multiband_kernel, dim3(1u), dim3(kMbThreads), 0, stream, a);
    return hipGetLastError();
}
