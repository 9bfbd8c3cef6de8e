// post_route.cpp — s2r_post_route (csrc/s2r_post_route.h, which includes nothing of HIP) over every call there is, under ASan + UBSan
// (tests/test_rules_native.py): a panned call, bus fills x the 8 subsets of running stem stages, master fills x 8 subsets x limiter
// on or off x stems wanted or not.  Each route is held (a) against the 24 routes written out by hand, one row per call, and (b)
// against the rule, stated without the table.  Prints "route ok".
#include <cstdio>
#include <cstdlib>

#include "s2r_post_route.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "post_route.cpp:%d: %s (%s)\n", __LINE__, #cond, what); std::exit(1); } } while (0)

// the seven buffers of a call, and none
enum Buf { NIL, CH, DL, FX, MS, LI, BO, OH, N_BUF };     // chorus_stage, delay_stage, fx_stage, master_stage, limiter_in, bus_out_dev, out_host_dev
float *cells = nullptr;                                  // main's array: one float per buffer, never touched
float *ptr(int b) { return b == NIL ? nullptr : cells + b; }

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
    float *const stage[S2R_STEM_STAGES] = {ptr(CH), ptr(DL), ptr(FX)};
    return s2r_post_route(call, stage, ptr(MS), ptr(LI), ptr(BO), ptr(OH));
}

// (a) the row of the table that names this call, and no other
void against_table(const S2rPostCall &call, const S2rPostRoute &r, const char *what) {
    int found = -1;
    for (int i = 0; i < 24; i++) {
        const Row &t = kTable[i];
        if (t.master != call.master || t.chorus != call.on[S2R_STEM_CHORUS] || t.delay != call.on[S2R_STEM_DELAY] || t.reverb != call.on[S2R_STEM_REVERB] ||
            t.limiter != call.limited) continue;
        CHECK(found < 0);
        found = i;
    }
    CHECK(found >= 0);
    hits[found]++;
    const Row &t = kTable[found];
    CHECK(r.combine_out == ptr(t.combine_out));
    CHECK(r.stem[S2R_STEM_CHORUS].in == ptr(t.chorus_in) && r.stem[S2R_STEM_CHORUS].out == ptr(t.chorus_out));
    CHECK(r.stem[S2R_STEM_DELAY].in == ptr(t.delay_in) && r.stem[S2R_STEM_DELAY].out == ptr(t.delay_out));
    CHECK(r.stem[S2R_STEM_REVERB].in == ptr(t.fx_in) && r.stem[S2R_STEM_REVERB].out == ptr(t.fx_out));
    CHECK(r.master_in == ptr(t.master_in) && r.master_out == ptr(t.master_out));
    CHECK(r.limiter_in == ptr(t.limiter_in) && r.limiter_out == ptr(t.limiter_out));
    CHECK(r.master_stems == (call.master && call.stems ? ptr(BO) : nullptr));
}

// (b) the rule
void against_rule(const S2rPostCall &call, const S2rPostRoute &r, const char *what) {
    float *const own[S2R_STEM_STAGES] = {ptr(CH), ptr(DL), ptr(FX)};
    float *written = r.combine_out;                      // where the last writer so far has put the stems
    CHECK(written != nullptr);
    for (int k = 0; k < S2R_STEM_STAGES; k++) {
        if (!call.on[k]) { CHECK(r.stem[k].in == nullptr && r.stem[k].out == nullptr); continue; }
        CHECK(r.stem[k].in == own[k]);
        CHECK(r.stem[k].in == written);
        CHECK(r.stem[k].out != nullptr && r.stem[k].out != r.stem[k].in);
        written = r.stem[k].out;
    }
    CHECK(written == (call.master ? ptr(MS) : ptr(BO)));
    CHECK(r.master_in == (call.master ? ptr(MS) : nullptr));
    CHECK(r.master_out == (!call.master ? nullptr : call.limited ? r.limiter_in : ptr(OH)));
    CHECK(r.master_stems == (call.master && call.stems ? ptr(BO) : nullptr));
    if (call.limited) CHECK(r.limiter_in == ptr(LI) && r.limiter_out == ptr(OH));
    else CHECK(r.limiter_in == nullptr && r.limiter_out == nullptr);
}

}  // namespace

int main() {
    float buffers[N_BUF] = {};
    cells = buffers;
    char what[96] = "a panned call";
    {
        S2rPostCall call;                                // (whatever else is set: no buses, no route)
        call.frames = 64; call.on[S2R_STEM_DELAY] = true;
        const S2rPostRoute r = route_of(call);
        CHECK(!r.combine_out && !r.master_in && !r.master_out && !r.master_stems && !r.limiter_in && !r.limiter_out);
        for (int k = 0; k < S2R_STEM_STAGES; k++) CHECK(!r.stem[k].in && !r.stem[k].out);
    }
    int calls = 0;
    for (int master = 0; master < 2; master++)
        for (int subset = 0; subset < 1 << S2R_STEM_STAGES; subset++)
            for (int limited = 0; limited <= master; limited++)
                for (int stems = 0; stems <= master; stems++) {
                    S2rPostCall call;
                    call.n_buses = 3; call.frames = 64; call.master = master != 0; call.stems = stems != 0; call.limited = limited != 0;
                    for (int k = 0; k < S2R_STEM_STAGES; k++) call.on[k] = (subset >> k & 1) != 0;
                    std::snprintf(what, sizeof what, "%s fill, stages %d%d%d, limiter %d, stems %d", master ? "master" : "bus", (int)call.on[0], (int)call.on[1],
                                  (int)call.on[2], limited, stems);
                    const S2rPostRoute r = route_of(call);
                    against_table(call, r, what);
                    against_rule(call, r, what);
                    calls++;
                }
    std::snprintf(what, sizeof what, "all calls");
    CHECK(calls == 8 + 8 * 2 * 2);
    for (int i = 0; i < 24; i++) CHECK(hits[i] == (kTable[i].master ? 2 : 1));       // (a master row holds for both values of stems)
    std::printf("route ok\n");
    return 0;
}
