// post_route.cpp — s2r_post_route (csrc/s2r_post_route.h, which includes nothing of HIP) over every call there is, under ASan + UBSan
// (tests/test_rules_native.py): a panned call, and the 256 subsets of running bus stages x (a bus fill + master fills x limiter on or
// off x stems wanted or not), 1280 calls.  Each route is held (a) against the 24 routes written out by hand, one row per call, where
// the EQ, the dynamics, the drive, the flanger and the room are off; (b) against the rule, walked in launch order without the table;
// and (c) against the route of the same call with one more stage on, for every stage that is off in it: that stage takes exactly one
// pointer over and nothing else moves.  Prints "route ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "s2r_post_route.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "post_route.cpp:%d: %s (%s)\n", __LINE__, #cond, what); std::exit(1); } } while (0)

// the twelve buffers of a call, and none: chorus_stage, delay_stage, fx_stage, master_stage, limiter_in, bus_out_dev, out_host_dev, then
// the stages of the EQ, the dynamics, the drive, the flanger and the room
enum Buf { NIL, CH, DL, FX, MS, LI, BO, OH, EQ, DY, DR, FL, RM, N_BUF };
float *cells = nullptr;                                  // main's array: one float per buffer, never touched
float *ptr(int b) { return b == NIL ? nullptr : cells + b; }
const int kOwn[S2R_BUS_STAGES] = {EQ, DY, DR, FL, CH, DL, FX, RM};      // each stage's own buffer, by S2rBusStage
const int kTabled = 1 << S2R_BUS_CHORUS | 1 << S2R_BUS_DELAY | 1 << S2R_BUS_REVERB;      // the stages the table knows

struct Row {
    bool master, chorus, delay, reverb, limiter;
    int combine_out, chorus_in, chorus_out, delay_in, delay_out, fx_in, fx_out, master_in, master_out, limiter_in, limiter_out;
};
// call        chorus delay  reverb limiter | combine_out  chorus_in -> _out  delay_in -> _out  fx_in -> _out  master_in  master_out  limiter_in -> _out
const Row kTable[24] = {
    {false, false, false, false, false, BO, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL},
    {false, false, false, true,  false, FX, NIL, NIL, NIL, NIL, FX,  BO,  NIL, NIL, NIL, NIL},
    {false, false, true,  false, false, DL, NIL, NIL, DL,  BO,  NIL, NIL, NIL, NIL, NIL, NIL},
    {false, false, true,  true,  false, DL, NIL, NIL, DL,  FX,  FX,  BO,  NIL, NIL, NIL, NIL},
    {true,  false, false, false, false, MS, NIL, NIL, NIL, NIL, NIL, NIL, MS,  OH,  NIL, NIL},
    {true,  false, false, true,  false, FX, NIL, NIL, NIL, NIL, FX,  MS,  MS,  OH,  NIL, NIL},
    {true,  false, true,  false, false, DL, NIL, NIL, DL,  MS,  NIL, NIL, MS,  OH,  NIL, NIL},
    {true,  false, true,  true,  false, DL, NIL, NIL, DL,  FX,  FX,  MS,  MS,  OH,  NIL, NIL},
    {true,  false, false, false, true,  MS, NIL, NIL, NIL, NIL, NIL, NIL, MS,  LI,  LI,  OH},
    {true,  false, false, true,  true,  FX, NIL, NIL, NIL, NIL, FX,  MS,  MS,  LI,  LI,  OH},
    {true,  false, true,  false, true,  DL, NIL, NIL, DL,  MS,  NIL, NIL, MS,  LI,  LI,  OH},
    {true,  false, true,  true,  true,  DL, NIL, NIL, DL,  FX,  FX,  MS,  MS,  LI,  LI,  OH},
    {false, true,  false, false, false, CH, CH,  BO,  NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL},
    {false, true,  false, true,  false, CH, CH,  FX,  NIL, NIL, FX,  BO,  NIL, NIL, NIL, NIL},
    {false, true,  true,  false, false, CH, CH,  DL,  DL,  BO,  NIL, NIL, NIL, NIL, NIL, NIL},
    {false, true,  true,  true,  false, CH, CH,  DL,  DL,  FX,  FX,  BO,  NIL, NIL, NIL, NIL},
    {true,  true,  false, false, false, CH, CH,  MS,  NIL, NIL, NIL, NIL, MS,  OH,  NIL, NIL},
    {true,  true,  false, true,  false, CH, CH,  FX,  NIL, NIL, FX,  MS,  MS,  OH,  NIL, NIL},
    {true,  true,  true,  false, false, CH, CH,  DL,  DL,  MS,  NIL, NIL, MS,  OH,  NIL, NIL},
    {true,  true,  true,  true,  false, CH, CH,  DL,  DL,  FX,  FX,  MS,  MS,  OH,  NIL, NIL},
    {true,  true,  false, false, true,  CH, CH,  MS,  NIL, NIL, NIL, NIL, MS,  LI,  LI,  OH},
    {true,  true,  false, true,  true,  CH, CH,  FX,  NIL, NIL, FX,  MS,  MS,  LI,  LI,  OH},
    {true,  true,  true,  false, true,  CH, CH,  DL,  DL,  MS,  NIL, NIL, MS,  LI,  LI,  OH},
    {true,  true,  true,  true,  true,  CH, CH,  DL,  DL,  FX,  FX,  MS,  MS,  LI,  LI,  OH},
};
int hits[24];

S2rPostRoute route_of(const S2rPostCall &call) {
    float *own[S2R_BUS_STAGES];
    for (int k = 0; k < S2R_BUS_STAGES; k++) own[k] = ptr(kOwn[k]);
    return s2r_post_route(call, own, ptr(MS), ptr(LI), ptr(BO), ptr(OH));
}

// the route as its pointers in the order the struct declares them: combine_out, each stage's in and out, the master's three, the limiter's two
constexpr int kPointers = 1 + 2 * S2R_BUS_STAGES + 5;
static_assert(sizeof(S2rPostRoute) == kPointers * sizeof(float *), "one route, pointers alone");
struct Flat { float *p[kPointers]; };
Flat flat(const S2rPostRoute &r) { Flat f; std::memcpy(&f, &r, sizeof r); return f; }
constexpr int in_of(int k) { return 1 + 2 * k; }
constexpr int out_of(int k) { return 2 + 2 * k; }

// (a) the row of the table that names this call, and no other; for a call whose other five stages are off
void against_table(const S2rPostCall &call, const S2rPostRoute &r, const char *what) {
    int found = -1;
    for (int i = 0; i < 24; i++) {
        const Row &t = kTable[i];
        if (t.master != call.master || t.chorus != call.on[S2R_BUS_CHORUS] || t.delay != call.on[S2R_BUS_DELAY] || t.reverb != call.on[S2R_BUS_REVERB] ||
            t.limiter != call.limited) continue;
        CHECK(found < 0);
        found = i;
    }
    CHECK(found >= 0);
    hits[found]++;
    const Row &t = kTable[found];
    CHECK(r.combine_out == ptr(t.combine_out));
    CHECK(r.stage[S2R_BUS_CHORUS].in == ptr(t.chorus_in) && r.stage[S2R_BUS_CHORUS].out == ptr(t.chorus_out));
    CHECK(r.stage[S2R_BUS_DELAY].in == ptr(t.delay_in) && r.stage[S2R_BUS_DELAY].out == ptr(t.delay_out));
    CHECK(r.stage[S2R_BUS_REVERB].in == ptr(t.fx_in) && r.stage[S2R_BUS_REVERB].out == ptr(t.fx_out));
    for (int k = 0; k < S2R_BUS_STAGES; k++) if (!(kTabled >> k & 1)) CHECK(!call.on[k] && !r.stage[k].in && !r.stage[k].out);
    CHECK(r.master_in == ptr(t.master_in) && r.master_out == ptr(t.master_out));
    CHECK(r.limiter_in == ptr(t.limiter_in) && r.limiter_out == ptr(t.limiter_out));
    CHECK(r.master_stems == (call.master && call.stems ? ptr(BO) : nullptr));
}

// (b) the rule, walked as the chain launches: combine, the bus stages in enum order, master, limiter
void against_rule(const S2rPostCall &call, const S2rPostRoute &r, const char *what) {
    float *const pinned[2] = {ptr(BO), ptr(OH)};
    float *const dest = call.master ? ptr(MS) : ptr(BO);
    float *written = nullptr;                            // where the last writer so far has put the stems
    bool seen[N_BUF] = {};                               // every buffer is written before it is read, and once
    auto writes = [&](float *out) {
        CHECK(out > cells && out < cells + N_BUF && !seen[out - cells]);
        seen[out - cells] = true;
        written = out;
    };
    auto reads = [&](float *in) {
        CHECK(in != nullptr && in == written && seen[in - cells]);
        for (float *p : pinned) CHECK(in != p);          // no kernel reads pinned memory back
    };
    CHECK(r.combine_out != nullptr);                     // the combine writes first
    writes(r.combine_out);
    for (int k = 0; k < S2R_BUS_STAGES; k++) {
        if (!call.on[k]) { CHECK(r.stage[k].in == nullptr && r.stage[k].out == nullptr); continue; }
        CHECK(r.stage[k].in == ptr(kOwn[k]));            // its own buffer, which the writer in front wrote
        reads(r.stage[k].in);
        CHECK(r.stage[k].out != nullptr && r.stage[k].out != r.stage[k].in);
        writes(r.stage[k].out);
    }
    CHECK(written == dest);                              // the last writer hits the call's destination
    if (call.master) {
        CHECK(r.master_in == ptr(MS));
        reads(r.master_in);
        CHECK(r.master_out == (call.limited ? ptr(LI) : ptr(OH)));
        CHECK(r.master_stems == (call.stems ? ptr(BO) : nullptr));
    } else {
        CHECK(!r.master_in && !r.master_out && !r.master_stems);
    }
    if (call.limited) {
        CHECK(r.limiter_in == ptr(LI) && r.limiter_in == r.master_out && r.limiter_out == ptr(OH));
        for (float *p : pinned) CHECK(r.limiter_in != p);
    } else {
        CHECK(r.limiter_in == nullptr && r.limiter_out == nullptr);
    }
}

// (c) stage k, off in `call`, turned on: the nearest running stage in front of it — the combine if there is none — now writes k's
// buffer, k writes where that one wrote — the next running stage's buffer, else the call's destination —, and every other pointer of
// the route is what it was: without the stage, pointer for pointer the same route
void against_one_more(const S2rPostCall &call, const S2rPostRoute &r, int k, const char *what) {
    S2rPostCall with = call;
    with.on[k] = true;
    const Flat before = flat(r), after = flat(route_of(with));
    int moved = 0;                                       // combine_out
    for (int j = 0; j < k; j++) if (call.on[j]) moved = out_of(j);
    float *next = call.master ? ptr(MS) : ptr(BO);
    for (int j = S2R_BUS_STAGES - 1; j > k; j--) if (call.on[j]) next = ptr(kOwn[j]);
    for (int i = 0; i < kPointers; i++) {
        if (i == in_of(k)) CHECK(!before.p[i] && after.p[i] == ptr(kOwn[k]));
        else if (i == out_of(k)) CHECK(!before.p[i] && after.p[i] == before.p[moved] && after.p[i] == next);
        else if (i == moved) CHECK(after.p[i] == ptr(kOwn[k]) && before.p[i] != after.p[i]);
        else CHECK(after.p[i] == before.p[i]);
    }
}

}  // namespace

int main() {
    float buffers[N_BUF] = {};
    cells = buffers;
    char what[128] = "a default call";
    {
        S2rPostCall call;                                // off unless prepare finds the stage's effect
        for (int k = 0; k < S2R_BUS_STAGES; k++) CHECK(!call.on[k]);
    }
    std::snprintf(what, sizeof what, "a panned call");
    {
        S2rPostCall call;                                // (whatever else is set: no buses, no route)
        call.frames = 64; call.master = true; call.stems = true; call.limited = true;
        for (int k = 0; k < S2R_BUS_STAGES; k++) call.on[k] = true;
        const Flat f = flat(route_of(call));
        for (int i = 0; i < kPointers; i++) CHECK(f.p[i] == nullptr);
    }
    int calls = 0;
    for (int master = 0; master < 2; master++)
        for (int subset = 0; subset < 1 << S2R_BUS_STAGES; subset++)
            for (int limited = 0; limited <= master; limited++)
                for (int stems = 0; stems <= master; stems++) {
                    S2rPostCall call;
                    call.n_buses = 3; call.frames = 64; call.master = master != 0; call.stems = stems != 0; call.limited = limited != 0;
                    for (int k = 0; k < S2R_BUS_STAGES; k++) call.on[k] = (subset >> k & 1) != 0;
                    std::snprintf(what, sizeof what, "%s fill, stages %d%d%d%d%d%d%d%d, limiter %d, stems %d", master ? "master" : "bus", (int)call.on[0],
                                  (int)call.on[1], (int)call.on[2], (int)call.on[3], (int)call.on[4], (int)call.on[5], (int)call.on[6], (int)call.on[7], limited, stems);
                    const S2rPostRoute r = route_of(call);
                    if (!(subset & ~kTabled)) against_table(call, r, what);
                    against_rule(call, r, what);
                    for (int k = 0; k < S2R_BUS_STAGES; k++) if (!call.on[k]) against_one_more(call, r, k, what);
                    calls++;
                }
    std::snprintf(what, sizeof what, "all calls");
    CHECK(calls == 256 * (1 + 2 * 2));
    for (int i = 0; i < 24; i++) CHECK(hits[i] == (kTable[i].master ? 2 : 1));       // (a master row holds for both values of stems)
    std::printf("route ok\n");
    return 0;
}
