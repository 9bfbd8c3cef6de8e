// s2r_post_route.h — which stages run in one call of the post-mix chain (s2r_post.h) and who reads and writes what in it: plain
// pointers and integers, nothing of HIP, so that the rule is checked by a program of its own on the CPU (tests/native/post_route.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

// the bus stages — per-bus effects that read the buses' stems from one staging buffer and write them to the next — in the order the
// chain launches them, between the bus combine in front and the master stages behind
enum S2rBusStage { S2R_BUS_EQ, S2R_BUS_DYN, S2R_BUS_DRIVE, S2R_BUS_FLANGER, S2R_BUS_CHORUS, S2R_BUS_DELAY, S2R_BUS_REVERB, S2R_BUS_ROOM, S2R_BUS_STAGES };
// the master stages of a master fill, in the order the chain launches them: three writers — the master kernel, which mixes the stems
// to the master's two channels, and the two that work on those in turn — and behind them, from S2R_MASTER_LOUDNESS on, four readers
enum S2rMasterStage { S2R_MASTER_MIX, S2R_MASTER_MULTIBAND, S2R_MASTER_LIMITER, S2R_MASTER_LOUDNESS, S2R_MASTER_SPECTRUM, S2R_MASTER_RESAMPLER, S2R_MASTER_PCM,
                      S2R_MASTER_STAGES };
constexpr int S2R_MASTER_WRITERS = S2R_MASTER_LOUDNESS, S2R_MASTER_READERS = S2R_MASTER_STAGES - S2R_MASTER_LOUDNESS;

// every pointer of one call (s2r_post_route): the bus combine's and each stage's kernels'
struct S2rPostRoute {
    float *combine_out;
    struct { float *in, *out; } stage[S2R_BUS_STAGES];
    float *master_stems;                                         // where the master kernel copies the stems for the caller
    struct { float *in, *out; } writer[S2R_MASTER_WRITERS];      // by S2rMasterStage; the master kernel's `in` are the stems
    struct { float *stems, *in, *out; } reader[S2R_MASTER_READERS];      // by S2rMasterStage - S2R_MASTER_LOUDNESS; `out`: its copy of the master for the caller
    float *res_dev;                                              // the resampler's second output, in device memory for the PCM stage
};
struct S2rPostCall {                             // one fill, as prepare leaves it
    uint32_t n_buses = 0, frames = 0;            // n_buses 0: a panned fill, which runs no stage
    bool master = false, stems = false;          // s2r_fill_master; the caller wants the stems too
    bool on[S2R_BUS_STAGES] = {};                // the stage's effect runs on one of the call's buses (S2rPostChain::runs)
    bool run[S2R_MASTER_STAGES] = {};            // a master fill (the master kernel) with the stage set; the PCM stage only where it has a frame to convert
    bool pcm_idle = false;                       // ... and where it has none — it is set, behind a resampler that makes no frame in this call
    S2rPostRoute route{};
};

// Who reads and writes what, the only place that decides it.  One rule: every running writer reads its OWN buffer and writes the next
// running writer's; the combine writes the first one's, and whoever writes LAST writes where the call wants it: the pinned stems in a
// bus fill; in a master fill the pinned master, or `tail_in` when a reader runs behind.  The master kernel, whose own buffer is the
// stems' device stage, copies the stems out itself when the caller wants them (master_stems = bus_out_dev then, else null).  Every
// writer needs a buffer of its own because a kernel must not read pinned memory back: the writer in front of one that ran in place
// might have written a pinned output.  The readers all read the stems' stage and what the last writer wrote, and the first of them
// copies that to the pinned master (`out`; null for the others) — but a PCM stage behind the resampler reads the resampler's device
// output (`res_dev`: the buses' frames, and at `res_master_at` the master's) and copies nothing.  A stage that does not run has null
// pointers: a master stage in a bus fill, an effect on a bus past the call's in any; a panned fill (no buses) has no route.  `own[k]`:
// bus stage k's staging buffer, which only a call that runs the stage looks at; so the master stages' own.
inline S2rPostRoute s2r_post_route(const S2rPostCall &call, float *const own[S2R_BUS_STAGES], float *master_stage, float *multiband_in, float *limiter_in,
                                   float *tail_in, float *res_dev, size_t res_master_at, float *bus_out_dev, float *out_host_dev) {
    S2rPostRoute r{};
    if (!call.n_buses) return r;
    float *const own_master[S2R_MASTER_WRITERS] = {master_stage, multiband_in, limiter_in};
    float **writer = &r.combine_out;                             // the destination of whoever wrote last so far
    for (int k = 0; k < S2R_BUS_STAGES; k++)
        if (call.on[k]) { *writer = r.stage[k].in = own[k]; writer = &r.stage[k].out; }
    for (int k = 0; k < S2R_MASTER_WRITERS; k++)
        if (call.run[k]) { *writer = r.writer[k].in = own_master[k]; writer = &r.writer[k].out; }
    bool tail = false;
    for (int k = S2R_MASTER_WRITERS; k < S2R_MASTER_STAGES; k++) tail = tail || call.run[k];
    float *const last = *writer = !call.master ? bus_out_dev : (tail ? tail_in : out_host_dev);
    if (call.master && call.stems) r.master_stems = bus_out_dev;
    float *copy = out_host_dev;
    for (int k = 0; k < S2R_MASTER_READERS; k++)
        if (call.run[S2R_MASTER_WRITERS + k]) { r.reader[k].stems = master_stage; r.reader[k].in = last; r.reader[k].out = copy; copy = nullptr; }
    if (call.run[S2R_MASTER_RESAMPLER] && call.run[S2R_MASTER_PCM]) {
        r.res_dev = res_dev;
        r.reader[S2R_MASTER_PCM - S2R_MASTER_WRITERS] = {res_dev, res_dev + res_master_at, nullptr};
    }
    return r;
}
