// post_route_flanger.cpp — s2r_post_route_flanger (csrc/s2r_post_route.h, which includes nothing of HIP) over every call there is, under
// ASan + UBSan (tests/test_flanger_native.py): the 24 routes of post_route.cpp — bus fills x the 8 subsets of running stem stages, master
// fills x 8 subsets x limiter on or off, each for both values of `stems` —, each with the EQ, the dynamics, the room, the drive and the
// flanger off and on.  The route is walked as the chain launches it — combine, EQ, dynamics, drive, flanger, chorus, delay, reverb, room,
// master, limiter — and the walk checks that the combine writes first, that every buffer a stage reads is the one the stage in front of
// it wrote, that the last writer of the stems hits the call's destination, and that no kernel reads one of the two pinned outputs.
// Without a flanger the route is pointer for pointer the drive's.  Prints "route flanger ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "s2r_post_route.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "post_route_flanger.cpp:%d: %s (%s)\n", __LINE__, #cond, what); std::exit(1); } } while (0)

// the twelve buffers of a call: chorus, delay and fx stages, master_stage, limiter_in, bus_out_dev, out_host_dev, the EQ's stage, the
// dynamics', the room's, the drive's, the flanger's
enum Buf { CH, DL, FX, MS, LI, BO, OH, EQ, DY, RM, DR, FL, N_BUF };

}  // namespace

int main() {
    float cells[N_BUF] = {};                             // one float per buffer, never touched
    float *const stage[S2R_STEM_STAGES] = {cells + CH, cells + DL, cells + FX};
    float *const pinned[2] = {cells + BO, cells + OH};
    char what[200] = "a panned call";
    auto route_drive = [&](const S2rPostCall &call) {
        return s2r_post_route_drive(call, s2r_post_route_room(call, s2r_post_route_dyn(call, s2r_post_route_eq(call, s2r_post_route(call, stage, cells + MS, cells + LI, cells + BO, cells + OH),
                                                                                                               cells + EQ), cells + DY), cells + RM), cells + DR);
    };
    {
        S2rPostCall call;                                // no buses, no route: the flags change nothing
        call.frames = 64; call.eq = true; call.dyn = true; call.room = true; call.drive = true; call.flanger = true;
        const S2rPostRouteFlanger r = s2r_post_route_flanger(call, route_drive(call), cells + FL);
        CHECK(!r.combine_out && !r.eq.in && !r.eq.out && !r.dyn.in && !r.dyn.out && !r.room.in && !r.room.out && !r.drive.in && !r.drive.out && !r.flanger.in &&
              !r.flanger.out && !r.master_in && !r.limiter_in);
    }
    CHECK(!S2rPostCall{}.flanger);                       // off unless prepare finds a flanger
    int routes = 0, calls = 0;
    for (int master = 0; master < 2; master++)
        for (int subset = 0; subset < 1 << S2R_STEM_STAGES; subset++)
            for (int limited = 0; limited <= master; limited++) {
                for (int stems = 0; stems <= master; stems++)
                    for (int flags = 0; flags < 32; flags++) {
                        const int eq = flags & 1, dyn = flags >> 1 & 1, room = flags >> 2 & 1, drive = flags >> 3 & 1, flanger = flags >> 4 & 1;
                        S2rPostCall call;
                        call.n_buses = 3; call.frames = 64; call.master = master != 0; call.stems = stems != 0; call.limited = limited != 0;
                        call.eq = eq != 0; call.dyn = dyn != 0; call.room = room != 0; call.drive = drive != 0; call.flanger = flanger != 0;
                        for (int k = 0; k < S2R_STEM_STAGES; k++) call.on[k] = (subset >> k & 1) != 0;
                        std::snprintf(what, sizeof what, "%s fill, stages %d%d%d, limiter %d, stems %d, eq %d, dyn %d, room %d, drive %d, flanger %d",
                                      master ? "master" : "bus", (int)call.on[0], (int)call.on[1], (int)call.on[2], limited, stems, eq, dyn, room, drive, flanger);
                        const S2rPostRouteDrive before = route_drive(call);
                        const S2rPostRouteFlanger r = s2r_post_route_flanger(call, before, cells + FL);
                        const S2rPostRouteDrive &base = r;
                        float *const dest = call.master ? cells + MS : cells + BO;
                        if (!flanger) {                      // pointer for pointer the drive's route
                            CHECK(std::memcmp(&base, &before, sizeof before) == 0 && !r.flanger.in && !r.flanger.out);
                        } else {
                            // exactly one pointer of the route moved: the writer in front of the flanger now writes the flanger's buffer,
                            // and the flanger writes where that writer wrote
                            float *const *moved = drive ? &r.drive.out : dyn ? &r.dyn.out : eq ? &r.eq.out : &r.combine_out;
                            const float *const *was = drive ? &before.drive.out : dyn ? &before.dyn.out : eq ? &before.eq.out : &before.combine_out;
                            CHECK(r.flanger.in == cells + FL && *moved == cells + FL && r.flanger.out == *was);
                            S2rPostRouteDrive undone = base;
                            *(drive ? &undone.drive.out : dyn ? &undone.dyn.out : eq ? &undone.eq.out : &undone.combine_out) = r.flanger.out;
                            CHECK(std::memcmp(&undone, &before, sizeof before) == 0);
                            // where it writes: the first running stem stage's buffer, else the room's, else the call's destination
                            float *next = room ? cells + RM : dest;
                            for (int k = S2R_STEM_STAGES - 1; k >= 0; k--) if (call.on[k]) next = stage[k];
                            CHECK(r.flanger.out == next);
                        }
                        // the walk, in launch order: `written` is where the stems are
                        float *written = r.combine_out;
                        CHECK(written != nullptr);           // the combine writes first
                        bool seen[N_BUF] = {};               // every buffer is written before it is read, and once
                        auto writes = [&](float *out) {
                            CHECK(out >= cells && out < cells + N_BUF && !seen[out - cells]);
                            seen[out - cells] = true;
                            written = out;
                        };
                        writes(r.combine_out);
                        auto reads = [&](float *in) {
                            CHECK(in == written && seen[in - cells]);
                            for (float *p : pinned) CHECK(in != p);
                        };
                        if (eq) { CHECK(r.eq.in == cells + EQ); reads(r.eq.in); CHECK(r.eq.out && r.eq.out != r.eq.in); writes(r.eq.out); }
                        else CHECK(!r.eq.in && !r.eq.out);
                        if (dyn) { CHECK(r.dyn.in == cells + DY); reads(r.dyn.in); CHECK(r.dyn.out && r.dyn.out != r.dyn.in); writes(r.dyn.out); }
                        else CHECK(!r.dyn.in && !r.dyn.out);
                        if (drive) { CHECK(r.drive.in == cells + DR); reads(r.drive.in); CHECK(r.drive.out && r.drive.out != r.drive.in); writes(r.drive.out); }
                        else CHECK(!r.drive.in && !r.drive.out);
                        if (flanger) { reads(r.flanger.in); CHECK(r.flanger.out && r.flanger.out != r.flanger.in); writes(r.flanger.out); }
                        for (int k = 0; k < S2R_STEM_STAGES; k++) {
                            if (!call.on[k]) { CHECK(!r.stem[k].in && !r.stem[k].out); continue; }
                            CHECK(r.stem[k].in == stage[k]);
                            reads(r.stem[k].in);
                            CHECK(r.stem[k].out && r.stem[k].out != r.stem[k].in);
                            writes(r.stem[k].out);
                        }
                        if (room) { CHECK(r.room.in == cells + RM); reads(r.room.in); CHECK(r.room.out != r.room.in); writes(r.room.out); }
                        else CHECK(!r.room.in && !r.room.out);
                        CHECK(written == dest);              // the last writer hits the call's destination
                        if (call.master) {
                            reads(r.master_in);
                            CHECK(r.master_out == (call.limited ? cells + LI : cells + OH));
                            CHECK(r.master_stems == (call.stems ? cells + BO : nullptr));
                            if (call.limited) { CHECK(r.limiter_in == r.master_out); for (float *p : pinned) CHECK(r.limiter_in != p); CHECK(r.limiter_out == cells + OH); }
                            else CHECK(!r.limiter_in && !r.limiter_out);
                        } else {
                            CHECK(!r.master_in && !r.master_out && !r.master_stems && !r.limiter_in && !r.limiter_out);
                        }
                        calls++;
                    }
                routes++;
            }
    std::snprintf(what, sizeof what, "all calls");
    CHECK(routes == 24 && calls == 32 * (8 + 8 * 2 * 2));
    static_assert(sizeof(S2rPostRouteFlanger) == sizeof(S2rPostRouteDrive) + 2 * sizeof(float *), "the flanger's pair on top of the route, pointers alone");
    std::printf("route flanger ok\n");
    return 0;
}
