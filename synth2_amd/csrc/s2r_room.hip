// s2r_room.hip — the per-bus room reverb of s2r_fill_buses and s2r_fill_master, the last stem writer of the post-mix
// chain: eight damped feedback combs in parallel and four allpasses in series per channel.  Per frame n of a bus:
//   in = (xL + xR) * gain
//   per channel c:  acc = +0.0
//     comb i:     o = C_ci[n - D_ci];  f_ci = (o * d1) + (f_ci * damp);  C_ci[n] = in + (f_ci * feedback);  acc = acc + o
//     allpass j:  b = A_cj[n - E_cj];  y = b - acc;  A_cj[n] = acc + (b * g);  acc = y
//   out_c = (dry * x_c) + ((wet * v_c) + (cross * v_(1-c)))
// binary32, every operation rounded on its own (-ffp-contract=off), denormals kept, nothing skipped for a zero.  Only f needs frame
// n - 1: two dependent operations per frame and comb.  Every other value a frame reads was written at least S2R_ROOM_MIN_DELAY = 64
// frames earlier, so inside a tile of S2R_ROOM_TILE = 32 frames everything else is frame-parallel, and — the tile being HALF the least
// delay — what tile p + 1 reads of the lines is complete before tile p begins: every load is issued a whole tile ahead of its use and
// no memory latency sits between two tiles.  ONE workgroup of 16 x 32 lanes per bus with a room (buses are independent and run on
// different CUs; both channels together, since `cross` couples them); lane (r, t) owns frame t of comb row r = c * 8 + i.  Per tile p:
//   A  every lane writes C of tile p - 1 (in + f * feedback, f from LDS) to the work area and puts o of tile p, loaded during tile
//      p - 1, into LDS.  Barrier.
//   B  every lane issues its loads for tile p + 1 (o, the bus's frame; a consumer lane also its four allpass frames).  Meanwhile sixteen
//      WALKER lanes, one per comb row, take their row's o from LDS into registers, carry f through the tile and leave f[n] in LDS; and
//      64 CONSUMER lanes, one per channel and frame, in another wave, sum the eight o in comb order, run the four allpasses on
//      registers, write the allpass lines and the output — none of which needs f.  Barrier.
// A line's frames of this call live in the work area (row l of [24][wstride]); frame n - D is read from the state for n < D and from
// the work area otherwise, never from the state's other copy, which is written once, at the end: each line's last D frames and each
// f.  The last tile may be partial: a lane past the call loads nothing and writes nothing, and the walker stops at the call's last
// frame.  Each value sees exactly the rule's operations in the rule's order, so the output is the host loop's bit for bit.  Buses of
// the call without a room are copied by other workgroups of the same launch.  No atomics, nothing that waits for another workgroup.
// -DS2R_ROOM_SERIAL builds the obvious form for comparison (tools/room_time.py, CHANGELOG): one thread per comb does its own loads,
// recursion and stores, frame by frame.
#include <hip/hip_runtime.h>
#include "s2r_device.h"

namespace {

typedef float room2 __attribute__((ext_vector_type(2)));
typedef float room4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kRoomTile = S2R_ROOM_TILE;
constexpr uint32_t kRoomRows = 2u * S2R_ROOM_COMBS;              // comb rows: channel-major
#ifdef S2R_ROOM_SERIAL
constexpr uint32_t kRoomThreads = 64u;
#else
constexpr uint32_t kRoomThreads = kRoomRows * kRoomTile;         // 512: a lane per comb row and frame of a tile
#endif
constexpr uint32_t kRoomPitch = kRoomTile + 4u;                  // floats per LDS row: 16-byte rows, and the walkers' rows on different banks
constexpr uint32_t kRoomCopyFrames = 4u * kRoomThreads;          // frames per workgroup of the copy of a bus without a room
static_assert(2u * kRoomTile <= S2R_ROOM_MIN_DELAY, "a tile's reads must be complete a whole tile ahead");
static_assert(kRoomTile == 32u && S2R_ROOM_LINES == kRoomRows + 2u * S2R_ROOM_ALLPASSES, "lane (r, t) = (tid >> 5, tid & 31); 16 comb and 8 allpass lines");

// frame n - len of a line: from the state while the call has not yet turned the line over, else from this call's frames
__device__ __forceinline__ float room_read(const float *line, const float *work, const uint32_t len, const uint32_t n) {
    return n < len ? line[n] : work[n - len];
}

}  // namespace

// Workgroup (0, q) runs the room of bus q.  Workgroups (1 + g, q) exist when a bus of the call has none, and copy that bus from `in`
// to `out`, kRoomCopyFrames frames each; every other workgroup returns at once.
__global__ void __launch_bounds__(kRoomThreads) s2r_room_kernel(const S2rRoom a) {
    const uint32_t tid = threadIdx.x, N = a.frames, q = blockIdx.y;
    const S2rRoomBus &b = a.bus[q];
    const room2 *const x2 = reinterpret_cast<const room2 *>(a.in) + (uint64_t)q * N;
    if (blockIdx.x > 0) {
        if (b.line) return;                                      // (uniform: the whole workgroup)
        room2 *const y2 = reinterpret_cast<room2 *>(a.out) + (uint64_t)q * N;
        const uint32_t n0 = (blockIdx.x - 1u) * kRoomCopyFrames;
        for (uint32_t n = n0 + tid; n < n0 + kRoomCopyFrames && n < N; n += kRoomThreads) y2[n] = x2[n];
        return;
    }
    if (!b.line) return;
    float *const out = a.out + (uint64_t)q * N * 2u;
    const float *const line = b.line;
    float *const work = b.work;
    const uint32_t ws = a.wstride;
    const float feedback = b.feedback, damp = b.damp, d1 = b.d1, g = b.g, gain = b.gain, dry = b.dry, wet = b.wet, cross = b.cross;
    __shared__ uint32_t slen[S2R_ROOM_LINES], soff[S2R_ROOM_LINES];
    if (tid < S2R_ROOM_LINES) { slen[tid] = b.len[tid]; soff[tid] = b.off[tid]; }
#ifdef S2R_ROOM_SERIAL
    __shared__ float so1[kRoomRows], sv1[2];
    __syncthreads();
    const bool comb = tid < kRoomRows, chan = tid < 2u;
    const uint32_t r = comb ? tid : 0u;
    const uint32_t len = slen[r];
    const float *const cl = line + soff[r];
    float *const cw = work + (size_t)r * ws;
    float f = cl[len];
    for (uint32_t n = 0; n < N; n++) {
        const room2 x = x2[n];
        const float s = x.x + x.y;
        const float in = s * gain;
        if (comb) {
            const float o = room_read(cl, cw, len, n);
            const float p = o * d1;
            const float m = f * damp;
            f = p + m;
            const float u = f * feedback;
            cw[n] = in + u;
            so1[r] = o;
        }
        __syncthreads();
        if (chan) {
            float acc = 0.0f;
            for (uint32_t i = 0; i < S2R_ROOM_COMBS; i++) acc = acc + so1[tid * 8u + i];
            for (uint32_t j = 0; j < S2R_ROOM_ALLPASSES; j++) {
                const uint32_t l = kRoomRows + tid * 4u + j;
                const float bb = room_read(line + soff[l], work + (size_t)l * ws, slen[l], n);
                const float y = bb - acc;
                const float m = bb * g;
                work[(size_t)l * ws + n] = acc + m;
                acc = y;
            }
            sv1[tid] = acc;
        }
        __syncthreads();
        if (chan) {
            const float v = sv1[tid], vo = sv1[tid ^ 1u];
            const float d = dry * (tid ? x.y : x.x);
            const float w = wet * v;
            const float c = cross * vo;
            const float e = w + c;
            out[2u * (size_t)n + tid] = d + e;
        }
    }
    if (comb) b.next[soff[r] + len] = f;
    __syncthreads();
#else
    __shared__ __attribute__((aligned(16))) float so[kRoomRows][kRoomPitch];     // o of the tile in hand
    __shared__ __attribute__((aligned(16))) float sf[kRoomRows][kRoomPitch];     // f of the tile in hand, read a phase later
    __syncthreads();
    const uint32_t r = tid >> 5, t = tid & 31u;
    const bool walker = tid < kRoomRows, consumer = tid >= 64u && tid < 128u;
    const uint32_t c = r & 1u;                                   // a consumer's channel: rows 2 and 3 are wave 1's halves
    const uint32_t len = slen[r];
    const float *const cl = line + soff[r];
    float *const cw = work + (size_t)r * ws;
    const uint32_t tiles = (N + kRoomTile - 1u) / kRoomTile;
    // a consumer's four allpass lines
    const float *al[S2R_ROOM_ALLPASSES]; float *aw[S2R_ROOM_ALLPASSES]; uint32_t alen[S2R_ROOM_ALLPASSES];
#pragma unroll
    for (uint32_t j = 0; j < S2R_ROOM_ALLPASSES; j++) {
        const uint32_t l = kRoomRows + c * 4u + j;
        al[j] = line + soff[l]; aw[j] = work + (size_t)l * ws; alen[j] = slen[l];
    }
    float f = walker ? line[soff[tid] + slen[tid]] : 0.0f;       // (the walker's: row tid)
    // tile 0's loads: all of them history
    float o_cur = 0.0f, bq_cur[S2R_ROOM_ALLPASSES] = {0.0f, 0.0f, 0.0f, 0.0f};
    room2 x_cur = room2{0.0f, 0.0f};
    if (t < N) {
        o_cur = room_read(cl, cw, len, t);
        x_cur = x2[t];
        if (consumer) {
#pragma unroll
            for (uint32_t j = 0; j < S2R_ROOM_ALLPASSES; j++) bq_cur[j] = room_read(al[j], aw[j], alen[j], t);
        }
    }
    float in_prev = 0.0f;
    for (uint32_t p = 0; p <= tiles; p++) {
        // A: the comb lines' frames of tile p - 1, and o of tile p for the walkers and consumers
        if (p >= 1u) {
            const uint32_t np = (p - 1u) * kRoomTile + t;
            const float u = sf[r][t] * feedback;
            if (np < N) cw[np] = in_prev + u;
        }
        if (p < tiles) so[r][t] = o_cur;
        __syncthreads();
        if (p == tiles) break;
        // B: the loads of tile p + 1 first: what they read is complete up to tile p - 1, and nothing below waits for them
        const uint32_t t0 = p * kRoomTile, n = t0 + t, n1 = n + kRoomTile;
        float o_next = 0.0f, bq_next[S2R_ROOM_ALLPASSES] = {0.0f, 0.0f, 0.0f, 0.0f};
        room2 x_next = room2{0.0f, 0.0f};
        if (n1 < N) {
            o_next = room_read(cl, cw, len, n1);
            x_next = x2[n1];
            if (consumer) {
#pragma unroll
                for (uint32_t j = 0; j < S2R_ROOM_ALLPASSES; j++) bq_next[j] = room_read(al[j], aw[j], alen[j], n1);
            }
        }
        const float s = x_cur.x + x_cur.y;
        const float in = s * gain;
        if (walker) {
            const uint32_t cnt = N - t0 < kRoomTile ? N - t0 : kRoomTile;
            if (cnt == kRoomTile) {
                const room4 *const o4 = reinterpret_cast<const room4 *>(so[tid]);
                room4 *const f4 = reinterpret_cast<room4 *>(sf[tid]);
                room4 ov[kRoomTile / 4u];
#pragma unroll
                for (uint32_t k = 0; k < kRoomTile / 4u; k++) ov[k] = o4[k];
#pragma unroll
                for (uint32_t k = 0; k < kRoomTile / 4u; k++) {
                    room4 fo;
                    { const float pp = ov[k].x * d1; const float m = f * damp; f = pp + m; fo.x = f; }
                    { const float pp = ov[k].y * d1; const float m = f * damp; f = pp + m; fo.y = f; }
                    { const float pp = ov[k].z * d1; const float m = f * damp; f = pp + m; fo.z = f; }
                    { const float pp = ov[k].w * d1; const float m = f * damp; f = pp + m; fo.w = f; }
                    f4[k] = fo;
                }
            } else {
                for (uint32_t k = 0; k < cnt; k++) { const float pp = so[tid][k] * d1; const float m = f * damp; f = pp + m; sf[tid][k] = f; }   // the call's last frames
            }
        } else if (consumer) {                                   // (wave 1, whole: the exchange below is among its lanes)
            float acc = 0.0f;
#pragma unroll
            for (uint32_t i = 0; i < S2R_ROOM_COMBS; i++) acc = acc + so[c * 8u + i][t];
#pragma unroll
            for (uint32_t j = 0; j < S2R_ROOM_ALLPASSES; j++) {
                const float bb = bq_cur[j];
                const float y = bb - acc;
                const float m = bb * g;
                if (n < N) aw[j][n] = acc + m;
                acc = y;
            }
            const float vo = __shfl_xor(acc, 32);                // the other channel's v of the same frame
            const float d = dry * (c ? x_cur.y : x_cur.x);
            const float w = wet * acc;
            const float e = cross * vo;
            const float h = w + e;
            if (n < N) out[2u * (size_t)n + c] = d + h;
        }
        __syncthreads();
        in_prev = in; o_cur = o_next; x_cur = x_next;
#pragma unroll
        for (uint32_t j = 0; j < S2R_ROOM_ALLPASSES; j++) bq_cur[j] = bq_next[j];
    }
    if (walker) b.next[soff[tid] + slen[tid]] = f;
#endif
    // the next state: each line's last frames, from the old state as far as the call did not reach, else from the work area
    for (uint32_t l = 0; l < S2R_ROOM_LINES; l++) {
        const uint32_t D = slen[l], at = soff[l];
        const float *const ll = line + at;
        const float *const lw = work + (size_t)l * ws;
        for (uint32_t m = tid; m < D; m += kRoomThreads) b.next[at + m] = N + m < D ? ll[N + m] : lw[N + m - D];
    }
}

hipError_t s2r_launch_bus_room(const S2rRoom &a, hipStream_t stream) {
    if (a.frames == 0 || a.n_buses == 0) return hipSuccess;
    if (a.n_buses > S2R_MAX_BUSES || !a.in || !a.out || a.in == a.out || a.frames > a.wstride) return hipErrorInvalidValue;
    uint32_t active = 0, plain = 0;
    for (uint32_t q = 0; q < a.n_buses; q++) {
        const S2rRoomBus &b = a.bus[q];
        if (!b.line) { plain++; continue; }
        if (!b.next || b.line == b.next || !b.work) return hipErrorInvalidValue;
        for (uint32_t l = 0; l < S2R_ROOM_LINES; l++)            // the layout the kernel indexes by: lines in range, inside the state
            if (b.len[l] < S2R_ROOM_MIN_DELAY || b.len[l] > S2R_ROOM_MAX_DELAY || b.off[l] > b.floats ||
                b.len[l] + (l < 2u * S2R_ROOM_COMBS ? 1u : 0u) > b.floats - b.off[l]) return hipErrorInvalidValue;
        active++;
    }
    if (active == 0) return hipErrorInvalidValue;                // (a call without a room does not come here)
    const dim3 grid = plain ? dim3(1u + (a.frames + kRoomCopyFrames - 1u) / kRoomCopyFrames, a.n_buses) : dim3(1u, a.n_buses);
    hipLaunchKernelGGL(s2r_room_kernel, grid, dim3(kRoomThreads), 0, stream, a);
    return hipGetLastError();
}
