// s2r_post_route.h — who reads and writes what in one call of the post-mix chain (s2r_post.h): plain pointers and integers, nothing of
// HIP, so that the rule is checked by a program of its own on the CPU (tests/native/post_route.cpp).  The route grows by inserts, each a
// struct on top of the last and a function applied after the last: the EQ, the dynamics, the room, the drive and the flanger, in the
// order they came; the chain launches combine, EQ, dynamics, drive, flanger, the stem stages, room, master, limiter.
#pragma once
#include <cstdint>

// the stem stages — per-bus effects that read the buses' stems from one staging buffer and write them to the next — in chain order
enum S2rStemStage { S2R_STEM_CHORUS, S2R_STEM_DELAY, S2R_STEM_REVERB, S2R_STEM_STAGES };

// every pointer of one call (s2r_post_route): the bus combine's, each stem stage's kernels', the master kernel's and the limiter's
struct S2rPostRoute {
    float *combine_out;
    struct { float *in, *out; } stem[S2R_STEM_STAGES];
    struct { float *in, *out; } eq;              // the EQ insert at the head of the stem chain (s2r_post_route_eq): null unless the call runs it
    float *master_in, *master_out, *master_stems, *limiter_in, *limiter_out;
};
// ... and the dynamics insert behind the EQ (s2r_post_route_dyn): null unless the call runs it.  A struct of its own on top of the
// route, whose layout stays what it was
struct S2rPostRouteDyn : S2rPostRoute {
    struct { float *in, *out; } dyn;
};
// ... and the room insert at the other end, behind the last stem stage (s2r_post_route_room): null unless the call runs it.  Again a
// struct of its own on top
struct S2rPostRouteRoom : S2rPostRouteDyn {
    struct { float *in, *out; } room;
};
// ... and the drive insert behind the dynamics (s2r_post_route_drive): null unless the call runs it.  Again a struct of its own on top
struct S2rPostRouteDrive : S2rPostRouteRoom {
    struct { float *in, *out; } drive;
};
// ... and the flanger insert behind the drive (s2r_post_route_flanger): null unless the call runs it.  Again a struct of its own on top
struct S2rPostRouteFlanger : S2rPostRouteDrive {
    struct { float *in, *out; } flanger;
};
struct S2rPostCall {                             // one fill, as prepare leaves it
    uint32_t n_buses = 0, frames = 0;            // n_buses 0: a panned fill, which runs no stage
    bool master = false, stems = false;          // s2r_fill_master; the caller wants the stems too
    bool on[S2R_STEM_STAGES] = {};               // the stage's effect sits on one of the call's buses
    bool limited = false;                        // a master fill with the limiter set
    bool eq = false;                             // an EQ sits on one of the call's buses
    bool dyn = false;                            // dynamics sit on one of the call's buses, their key bus among them too
    bool room = false;                           // a room sits on one of the call's buses
    bool drive = false;                          // a drive sits on one of the call's buses
    bool flanger = false;                        // a flanger sits on one of the call's buses
    S2rPostRouteFlanger route{};
};

// Who reads and writes what, the only place that decides it.  The combine writes into the first stem stage that runs, each running
// stage into the next running stage's input, and whichever of them writes the stems LAST writes them where the call wants them: the
// pinned output in a bus fill; the master's device stage in a master fill, whose kernel must not read pinned memory back and copies
// them out itself when the caller wants them (master_stems = bus_out_dev then, else null).  The master kernel's two channels go to
// the pinned output unless the limiter follows and writes there in its place.  A stage that does not run has null pointers: a
// limiter that is set is idle in a bus fill, an effect on a bus past the call's in any; a panned fill (no buses) has no route.
// `stem_stage[k]`: stage k's staging buffer, which only a call that runs the stage looks at.
inline S2rPostRoute s2r_post_route(const S2rPostCall &call, float *const stem_stage[S2R_STEM_STAGES], float *master_stage, float *limiter_in, float *bus_out_dev,
                                   float *out_host_dev) {
    S2rPostRoute r{};
    if (!call.n_buses) return r;
    float **writer = &r.combine_out;                             // the destination of whoever wrote the stems last so far
    for (int k = 0; k < S2R_STEM_STAGES; k++)
        if (call.on[k]) { *writer = r.stem[k].in = stem_stage[k]; writer = &r.stem[k].out; }
    *writer = call.master ? master_stage : bus_out_dev;
    if (call.master) { r.master_in = master_stage; r.master_out = call.limited ? limiter_in : out_host_dev; r.master_stems = call.stems ? bus_out_dev : nullptr; }
    if (call.limited) { r.limiter_in = limiter_in; r.limiter_out = out_host_dev; }
    return r;
}

// The EQ is an insert at the head of the stem chain, not a stem stage: given the finished route of a call that runs it and the EQ's
// staging buffer, the EQ reads its own buffer and writes where the combine would have written, and the combine is redirected into
// the EQ's buffer.  The buffer is needed in every route: in a bus fill with no stem stage the combine's destination is pinned host
// memory, which a kernel must not read back, so the EQ cannot run in place there.  A call without an EQ, or without buses, keeps its
// route as it is.
inline S2rPostRoute s2r_post_route_eq(const S2rPostCall &call, S2rPostRoute r, float *eq_stage) {
    if (!call.eq || !call.n_buses) return r;
    r.eq.in = eq_stage; r.eq.out = r.combine_out;
    r.combine_out = eq_stage;
    return r;
}

// The dynamics are the second insert, behind the EQ and in front of the stem stages, applied to the route after s2r_post_route_eq: the
// stage reads its own staging buffer and writes where the stage in front of it — the EQ if the call runs it, else the combine —
// would have written, and that writer is redirected into the dynamics' buffer.  A call without dynamics, or without buses, keeps its
// route as it is, with a null dyn pair.
inline S2rPostRouteDyn s2r_post_route_dyn(const S2rPostCall &call, const S2rPostRoute &route, float *dyn_stage) {
    S2rPostRouteDyn r{};
    static_cast<S2rPostRoute &>(r) = route;
    if (!call.dyn || !call.n_buses) return r;
    float *&writer = call.eq ? r.eq.out : r.combine_out;
    r.dyn.in = dyn_stage; r.dyn.out = writer;
    writer = dyn_stage;
    return r;
}

// The room is the third insert, at the other end of the stem chain: the last stem writer of a call that runs it.  Applied to the route
// after s2r_post_route_dyn: the room reads its own staging buffer and writes where the last stem writer would have written — the call's
// destination: the pinned output in a bus fill, the master's device stage in a master fill —, and that writer — the last running stem
// stage, else the dynamics, else the EQ, else the combine — is redirected into the room's buffer.  A call without a room, or without
// buses, keeps its route as it is, with a null room pair.
inline S2rPostRouteRoom s2r_post_route_room(const S2rPostCall &call, const S2rPostRouteDyn &route, float *room_stage) {
    S2rPostRouteRoom r{};
    static_cast<S2rPostRouteDyn &>(r) = route;
    if (!call.room || !call.n_buses) return r;
    float **writer = call.dyn ? &r.dyn.out : call.eq ? &r.eq.out : &r.combine_out;
    for (int k = 0; k < S2R_STEM_STAGES; k++) if (call.on[k]) writer = &r.stem[k].out;
    r.room.in = room_stage; r.room.out = *writer;
    *writer = room_stage;
    return r;
}

// The drive is the fourth insert, behind the dynamics and in front of the stem stages.  Applied to the route after s2r_post_route_room:
// the drive reads its own staging buffer and writes where the stage in front of it — the dynamics if the call runs them, else the EQ,
// else the combine — writes by now, which may already be the room's buffer, and that writer is redirected into the drive's buffer.  A
// call without a drive, or without buses, keeps its route as it is, with a null drive pair.
inline S2rPostRouteDrive s2r_post_route_drive(const S2rPostCall &call, const S2rPostRouteRoom &route, float *drive_stage) {
    S2rPostRouteDrive r{};
    static_cast<S2rPostRouteRoom &>(r) = route;
    if (!call.drive || !call.n_buses) return r;
    float *&writer = call.dyn ? r.dyn.out : call.eq ? r.eq.out : r.combine_out;
    r.drive.in = drive_stage; r.drive.out = writer;
    writer = drive_stage;
    return r;
}

// The flanger is the fifth insert, behind the drive and in front of the stem stages.  Applied to the route after s2r_post_route_drive:
// the flanger reads its own staging buffer and writes where the stage in front of it — the drive if the call runs it, else the dynamics,
// else the EQ, else the combine — writes by now, and that writer is redirected into the flanger's buffer.  A call without a flanger, or
// without buses, keeps its route as it is, with a null flanger pair.
inline S2rPostRouteFlanger s2r_post_route_flanger(const S2rPostCall &call, const S2rPostRouteDrive &route, float *flanger_stage) {
    S2rPostRouteFlanger r{};
    static_cast<S2rPostRouteDrive &>(r) = route;
    if (!call.flanger || !call.n_buses) return r;
    float *&writer = call.drive ? r.drive.out : call.dyn ? r.dyn.out : call.eq ? r.eq.out : r.combine_out;
    r.flanger.in = flanger_stage; r.flanger.out = writer;
    writer = flanger_stage;
    return r;
}
