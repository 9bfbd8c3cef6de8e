// s2r_post_route.h — who reads and writes what in one call of the post-mix chain (s2r_post.h): plain pointers and integers, nothing of
// HIP, so that the rule is checked by a program of its own on the CPU (tests/native/post_route.cpp).
#pragma once
#include <cstdint>

// the bus stages — per-bus effects that read the buses' stems from one staging buffer and write them to the next — in the order the
// chain launches them, between the bus combine in front and the master kernel and the limiter behind
enum S2rBusStage { S2R_BUS_EQ, S2R_BUS_DYN, S2R_BUS_DRIVE, S2R_BUS_FLANGER, S2R_BUS_CHORUS, S2R_BUS_DELAY, S2R_BUS_REVERB, S2R_BUS_ROOM, S2R_BUS_STAGES };

// every pointer of one call (s2r_post_route): the bus combine's, each bus stage's kernels', the master kernel's and the limiter's
struct S2rPostRoute {
    float *combine_out;
    struct { float *in, *out; } stage[S2R_BUS_STAGES];
    float *master_in, *master_out, *master_stems, *limiter_in, *limiter_out;
};
struct S2rPostCall {                             // one fill, as prepare leaves it
    uint32_t n_buses = 0, frames = 0;            // n_buses 0: a panned fill, which runs no stage
    bool master = false, stems = false;          // s2r_fill_master; the caller wants the stems too
    bool on[S2R_BUS_STAGES] = {};                // the stage's effect runs on one of the call's buses (S2rPostChain::runs)
    bool limited = false;                        // a master fill with the limiter set
    S2rPostRoute route{};
};

// Who reads and writes what, the only place that decides it.  One rule: every running stage reads its OWN staging buffer and writes
// the next running stage's; the combine writes the first running stage's, and whoever writes the stems LAST writes them where the call
// wants them: the pinned output in a bus fill; the master's device stage in a master fill, whose kernel copies them out itself when the
// caller wants them (master_stems = bus_out_dev then, else null).  Every stage needs a buffer of its own because a kernel must not read
// pinned memory back: in a bus fill the writer in front of a stage that ran in place would have written the pinned output.  The
// master kernel's two channels go to the pinned output unless the limiter follows and writes there in its place.  A stage that does
// not run has null pointers: a limiter that is set is idle in a bus fill, an effect on a bus past the call's in any; a panned fill (no
// buses) has no route.  `own[k]`: stage k's staging buffer, which only a call that runs the stage looks at.
inline S2rPostRoute s2r_post_route(const S2rPostCall &call, float *const own[S2R_BUS_STAGES], float *master_stage, float *limiter_in, float *bus_out_dev,
                                   float *out_host_dev) {
    S2rPostRoute r{};
    if (!call.n_buses) return r;
    float **writer = &r.combine_out;                             // the destination of whoever wrote the stems last so far
    for (int k = 0; k < S2R_BUS_STAGES; k++)
        if (call.on[k]) { *writer = r.stage[k].in = own[k]; writer = &r.stage[k].out; }
    *writer = call.master ? master_stage : bus_out_dev;
    if (call.master) { r.master_in = master_stage; r.master_out = call.limited ? limiter_in : out_host_dev; r.master_stems = call.stems ? bus_out_dev : nullptr; }
    if (call.limited) { r.limiter_in = limiter_in; r.limiter_out = out_host_dev; }
    return r;
}
