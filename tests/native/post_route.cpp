// post_route.cpp — s2r_post_route (csrc/s2r_post_route.h, which includes nothing of HIP) over every call there is, under ASan + UBSan
// (tests/test_rules_native.py): a panned call, and the 256 subsets of running bus stages x (a bus fill + master fills x the 64 subsets
// of {multiband, limiter, loudness, spectrum, resampler, PCM} set, the 16 with both resampler and PCM once more with the PCM stage idle
// behind a resampler that makes no frame, x stems wanted or not), 256 x (1 + 80 x 2) calls.  Each route is held (a) against the 24
// routes written out by hand, one row per call, where the EQ, the dynamics, the drive, the flanger, the room and every master stage but
// the limiter are off, and against the 12 rows of the master stages' table where no bus stage runs; (b) against the rule, walked in
// launch order without the tables; and (c) against the route of the same call with one more stage on, for every stage that is off in
// it: a bus stage or a master writer takes exactly one pointer over and nothing else moves, a master reader moves at most the copy
// of the master to the caller and, if it is the only one, the last writer's destination.  Prints "route ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "s2r_post_route.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "post_route.cpp:%d: %s (%s)\n", __LINE__, #cond, what); std::exit(1); } } while (0)

// the sixteen buffers of a call, and none: chorus_stage, delay_stage, fx_stage, master_stage, limiter_in, bus_out_dev, out_host_dev, then
// the stages of the EQ, the dynamics, the drive, the flanger and the room, then the multiband's input, the tail's input (the four
// readers') and the resampler's device output: RD where its buses' frames begin and RDM, kResMasterAt on, where its master's do
enum Buf { NIL, CH, DL, FX, MS, LI, BO, OH, EQ, DY, DR, FL, RM, MB, TL, RD, RDM, N_BUF };
constexpr size_t kResMasterAt = RDM - RD;
float *cells = nullptr;                                  // main's array: one float per buffer, never touched
float *ptr(int b) { return b == NIL ? nullptr : cells + b; }
const int kOwn[S2R_BUS_STAGES] = {EQ, DY, DR, FL, CH, DL, FX, RM};      // each stage's own buffer, by S2rBusStage
const int kTabled = 1 << S2R_BUS_CHORUS | 1 << S2R_BUS_DELAY | 1 << S2R_BUS_REVERB;      // the stages the table knows
const int kOwnMaster[S2R_MASTER_WRITERS] = {MS, MB, LI};                // each master writer's own buffer, by S2rMasterStage
constexpr int R0 = S2R_MASTER_WRITERS;                                  // route.reader[k - R0] is master stage k's

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

// The master stages of a master fill whose bus stages are all off (combine_out = MS, the master kernel reads MS), written out from the
// launches as they stood before the route decided them: the master kernel wrote the multiband's input if that was on, else the
// limiter's if that was, else — as whoever wrote last — the tail's input if any of the four stages behind was set and the pinned
// output if none was; each of the four read the stems' stage and the tail's input, and copied the master out unless the loudness or
// the spectrum kernel in front had; the PCM kernel behind a resampler that made a frame read that one's device output and copied nothing.
struct MasterRow {
    bool mb, limiter, loud, spec, res, pcm, idle;        // idle: the PCM stage is set and does not run
    int mix_out, mb_in, mb_out, limiter_in, limiter_out, loud_in, loud_out, spec_in, spec_out, res_in, res_out, res_dev, pcm_stems, pcm_in, pcm_out;
};
// mb     limiter loud   spec   res    pcm    idle  | mix_out  mb_in -> _out  limiter_in -> _out  loud in, out  spec in, out  res in, out, dev  pcm stems, in, out
const MasterRow kMasterTable[12] = {
    {false, false, false, false, false, false, false, OH, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL},
    {true,  false, false, false, false, false, false, MB, MB,  OH,  NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL},
    {false, true,  false, false, false, false, false, LI, NIL, NIL, LI,  OH,  NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL},
    {false, false, true,  false, false, false, false, TL, NIL, NIL, NIL, NIL, TL,  OH,  NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL},
    {false, false, false, true,  false, false, false, TL, NIL, NIL, NIL, NIL, NIL, NIL, TL,  OH,  NIL, NIL, NIL, NIL, NIL, NIL},
    {false, false, false, false, true,  false, false, TL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, TL,  OH,  NIL, NIL, NIL, NIL},
    {false, false, false, false, false, true,  false, TL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, MS,  TL,  OH},
    {false, true,  true,  false, false, false, false, LI, NIL, NIL, LI,  TL,  TL,  OH,  NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL},
    {true,  true,  false, false, false, true,  false, MB, MB,  LI,  LI,  TL,  NIL, NIL, NIL, NIL, NIL, NIL, NIL, MS,  TL,  OH},
    {false, false, false, false, true,  true,  false, TL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, TL,  OH,  RD,  RD,  RDM, NIL},
    {false, false, false, false, true,  true,  true,  TL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL, TL,  OH,  NIL, NIL, NIL, NIL},
    {true,  true,  true,  true,  true,  true,  false, MB, MB,  LI,  LI,  TL,  TL,  OH,  TL,  NIL, TL,  NIL, RD,  RD,  RDM, NIL},
};
int master_hits[12];

S2rPostRoute route_of(const S2rPostCall &call) {
    float *own[S2R_BUS_STAGES];
    for (int k = 0; k < S2R_BUS_STAGES; k++) own[k] = ptr(kOwn[k]);
    return s2r_post_route(call, own, ptr(MS), ptr(MB), ptr(LI), ptr(TL), ptr(RD), kResMasterAt, ptr(BO), ptr(OH));
}

// the route as its pointers in the order the struct declares them: combine_out, each bus stage's in and out, master_stems, each master
// writer's in and out, each reader's stems, in and out, res_dev
constexpr int kPointers = 1 + 2 * S2R_BUS_STAGES + 1 + 2 * S2R_MASTER_WRITERS + 3 * S2R_MASTER_READERS + 1;
static_assert(sizeof(S2rPostRoute) == kPointers * sizeof(float *), "one route, pointers alone");
struct Flat { float *p[kPointers]; };
Flat flat(const S2rPostRoute &r) { Flat f; std::memcpy(&f, &r, sizeof r); return f; }
constexpr int in_of(int k) { return 1 + 2 * k; }
constexpr int out_of(int k) { return 2 + 2 * k; }
constexpr int kStems = 1 + 2 * S2R_BUS_STAGES, kResDev = kPointers - 1;
constexpr int win_of(int k) { return kStems + 1 + 2 * k; }              // master writer k's
constexpr int wout_of(int k) { return kStems + 2 + 2 * k; }
constexpr int rstems_of(int k) { return kStems + 1 + 2 * S2R_MASTER_WRITERS + 3 * (k - R0); }  // master reader k's, k an S2rMasterStage
constexpr int rin_of(int k) { return rstems_of(k) + 1; }
constexpr int rout_of(int k) { return rstems_of(k) + 2; }
bool tail_of(const S2rPostCall &call) { bool t = false; for (int k = R0; k < S2R_MASTER_STAGES; k++) t = t || call.run[k]; return t; }

// (a) the row of the table that names this call, and no other; for a call whose other five bus stages and five master stages are off
void against_table(const S2rPostCall &call, const S2rPostRoute &r, const char *what) {
    int found = -1;
    for (int i = 0; i < 24; i++) {
        const Row &t = kTable[i];
        if (t.master != call.master || t.chorus != call.on[S2R_BUS_CHORUS] || t.delay != call.on[S2R_BUS_DELAY] || t.reverb != call.on[S2R_BUS_REVERB] ||
            t.limiter != call.run[S2R_MASTER_LIMITER]) continue;
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
    CHECK(r.writer[S2R_MASTER_MIX].in == ptr(t.master_in) && r.writer[S2R_MASTER_MIX].out == ptr(t.master_out));
    CHECK(r.writer[S2R_MASTER_LIMITER].in == ptr(t.limiter_in) && r.writer[S2R_MASTER_LIMITER].out == ptr(t.limiter_out));
    CHECK(r.master_stems == (call.master && call.stems ? ptr(BO) : nullptr));
    CHECK(!r.writer[S2R_MASTER_MULTIBAND].in && !r.writer[S2R_MASTER_MULTIBAND].out && !r.res_dev);
    for (int k = 0; k < S2R_MASTER_READERS; k++) CHECK(!r.reader[k].stems && !r.reader[k].in && !r.reader[k].out);
}

// ... and the row of the master stages' table; for a master fill that runs no bus stage
void against_master_table(const S2rPostCall &call, const S2rPostRoute &r, const char *what) {
    int found = -1;
    for (int i = 0; i < 12; i++) {
        const MasterRow &t = kMasterTable[i];
        if (t.mb != call.run[S2R_MASTER_MULTIBAND] || t.limiter != call.run[S2R_MASTER_LIMITER] || t.loud != call.run[S2R_MASTER_LOUDNESS] ||
            t.spec != call.run[S2R_MASTER_SPECTRUM] || t.res != call.run[S2R_MASTER_RESAMPLER] || t.pcm != (call.run[S2R_MASTER_PCM] || call.pcm_idle) ||
            t.idle != call.pcm_idle) continue;
        CHECK(found < 0);
        found = i;
    }
    if (found < 0) return;                               // (the table names 12 of the 80)
    master_hits[found]++;
    const MasterRow &t = kMasterTable[found];
    const int readers[S2R_MASTER_READERS][3] = {{t.loud ? MS : NIL, t.loud_in, t.loud_out}, {t.spec ? MS : NIL, t.spec_in, t.spec_out}, {t.res ? MS : NIL, t.res_in, t.res_out},
                                                {t.pcm_stems, t.pcm_in, t.pcm_out}};
    CHECK(r.combine_out == ptr(MS) && r.writer[S2R_MASTER_MIX].in == ptr(MS) && r.writer[S2R_MASTER_MIX].out == ptr(t.mix_out));
    CHECK(r.writer[S2R_MASTER_MULTIBAND].in == ptr(t.mb_in) && r.writer[S2R_MASTER_MULTIBAND].out == ptr(t.mb_out));
    CHECK(r.writer[S2R_MASTER_LIMITER].in == ptr(t.limiter_in) && r.writer[S2R_MASTER_LIMITER].out == ptr(t.limiter_out));
    for (int k = 0; k < S2R_MASTER_READERS; k++)
        CHECK(r.reader[k].stems == ptr(readers[k][0]) && r.reader[k].in == ptr(readers[k][1]) && r.reader[k].out == ptr(readers[k][2]));
    CHECK(r.res_dev == ptr(t.res_dev));
    CHECK(r.master_stems == (call.stems ? ptr(BO) : nullptr));
}

// (b) the rule, walked as the chain launches: combine, the bus stages in enum order, the master stages in theirs
void against_rule(const S2rPostCall &call, const S2rPostRoute &r, const char *what) {
    float *const pinned[2] = {ptr(BO), ptr(OH)};
    const bool tail = tail_of(call);
    float *const dest = !call.master ? ptr(BO) : (tail ? ptr(TL) : ptr(OH));
    float *written = nullptr;                            // where the last writer so far has put the stems, or the master
    bool seen[N_BUF] = {};                               // every buffer is written before it is read, and once
    auto copies = [&](float *out) {
        CHECK(out > cells && out < cells + N_BUF && !seen[out - cells]);
        seen[out - cells] = true;
    };
    auto writes = [&](float *out) { copies(out); written = out; };
    auto reads = [&](float *in) {
        CHECK(in != nullptr && seen[in - cells]);
        for (float *p : pinned) CHECK(in != p);          // no kernel reads pinned memory back
    };
    CHECK(r.combine_out != nullptr);                     // the combine writes first
    writes(r.combine_out);
    for (int k = 0; k < S2R_BUS_STAGES; k++) {
        if (!call.on[k]) { CHECK(r.stage[k].in == nullptr && r.stage[k].out == nullptr); continue; }
        CHECK(r.stage[k].in == ptr(kOwn[k]) && r.stage[k].in == written);    // its own buffer, which the writer in front wrote
        reads(r.stage[k].in);
        CHECK(r.stage[k].out != nullptr && r.stage[k].out != r.stage[k].in);
        writes(r.stage[k].out);
    }
    CHECK(call.run[S2R_MASTER_MIX] == call.master);
    for (int k = 0; k < S2R_MASTER_WRITERS; k++) {       // the bus stages' last writer hits the master kernel's buffer, and so on
        if (!call.run[k]) { CHECK(r.writer[k].in == nullptr && r.writer[k].out == nullptr); continue; }
        CHECK(call.master && r.writer[k].in == ptr(kOwnMaster[k]) && r.writer[k].in == written);
        reads(r.writer[k].in);
        CHECK(r.writer[k].out != nullptr && r.writer[k].out != r.writer[k].in);
        writes(r.writer[k].out);
    }
    CHECK(written == dest);                              // the last writer hits the call's destination
    CHECK(r.master_stems == (call.master && call.stems ? ptr(BO) : nullptr));
    if (r.master_stems) copies(r.master_stems);          // the master kernel's copy of the stems is the only writer of the pinned stems
    bool first = true;                                   // no reader so far: the first one copies the master out
    for (int k = R0; k < S2R_MASTER_STAGES; k++) {
        const auto &rd = r.reader[k - R0];
        if (!call.run[k]) { CHECK(rd.stems == nullptr && rd.in == nullptr && rd.out == nullptr); continue; }
        CHECK(call.master && tail && written == ptr(TL));
        if (k == S2R_MASTER_PCM && call.run[S2R_MASTER_RESAMPLER]) {    // behind the resampler: that one's device output, and no copy
            CHECK(!first && r.res_dev == ptr(RD) && rd.stems == ptr(RD) && rd.in == ptr(RDM) && rd.out == nullptr);
        } else {
            CHECK(rd.stems == ptr(MS) && rd.in == written && rd.out == (first ? ptr(OH) : nullptr));    // what the last writer wrote
            if (rd.out) copies(rd.out);
        }
        reads(rd.stems); reads(rd.in);
        if (k == S2R_MASTER_RESAMPLER && r.res_dev) { copies(ptr(RD)); copies(ptr(RDM)); }      // (one buffer, its two parts)
        first = false;
    }
    CHECK(!call.pcm_idle || (call.run[S2R_MASTER_RESAMPLER] && !call.run[S2R_MASTER_PCM]));
    CHECK((r.res_dev != nullptr) == (call.run[S2R_MASTER_RESAMPLER] && call.run[S2R_MASTER_PCM]));
    CHECK(seen[OH] == call.master && seen[BO] == (!call.master || call.stems));     // exactly one stage writes the pinned master (copies refuses a second)
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

// ... master writer k (the multiband, the limiter) of a master fill likewise: the nearest running writer in front — the master kernel
// if no other — now writes k's buffer, and k writes where that one wrote
void against_one_more_writer(const S2rPostCall &call, const S2rPostRoute &r, int k, const char *what) {
    S2rPostCall with = call;
    with.run[k] = true;
    const Flat before = flat(r), after = flat(route_of(with));
    int moved = -1;
    for (int j = 0; j < k; j++) if (call.run[j]) moved = wout_of(j);
    CHECK(moved >= 0);
    float *next = tail_of(call) ? ptr(TL) : ptr(OH);
    for (int j = S2R_MASTER_WRITERS - 1; j > k; j--) if (call.run[j]) next = ptr(kOwnMaster[j]);
    for (int i = 0; i < kPointers; i++) {
        if (i == win_of(k)) CHECK(!before.p[i] && after.p[i] == ptr(kOwnMaster[k]));
        else if (i == wout_of(k)) CHECK(!before.p[i] && after.p[i] == before.p[moved] && after.p[i] == next);
        else if (i == moved) CHECK(after.p[i] == ptr(kOwnMaster[k]) && before.p[i] != after.p[i]);
        else CHECK(after.p[i] == before.p[i]);
    }
}

// ... and master reader k: it reads the stems' stage and the tail's input.  The only reader, it moves the last writer's destination from
// the pinned master to the tail's input; in front of every other, it takes the copy to the pinned master from the one that had it.  The
// PCM stage behind a running resampler reads that one's device output, which the resampler then writes, and moves nothing else — so
// the resampler in front of a running PCM stage moves that one's two inputs as well.
void against_one_more_reader(const S2rPostCall &call, const S2rPostRoute &r, int k, const char *what) {
    S2rPostCall with = call;
    with.run[k] = true;
    const Flat before = flat(r), after = flat(route_of(with));
    int last = -1, had = -1;                             // the last writer's out; the copy-out pointer of the reader that has it in `call`
    for (int j = 0; j < S2R_MASTER_WRITERS; j++) if (call.run[j]) last = wout_of(j);
    for (int j = S2R_MASTER_STAGES - 1; j >= R0; j--) if (call.run[j] && before.p[rout_of(j)]) had = rout_of(j);
    CHECK(last >= 0 && (had >= 0) == tail_of(call));
    const bool behind = k == S2R_MASTER_PCM && call.run[S2R_MASTER_RESAMPLER];
    const bool takes = !behind && (had < 0 || rout_of(k) < had);             // k copies the master out in `with`
    const bool front = k == S2R_MASTER_RESAMPLER && call.run[S2R_MASTER_PCM];
    for (int i = 0; i < kPointers; i++) {
        if (i == rstems_of(k)) CHECK(!before.p[i] && after.p[i] == (behind ? ptr(RD) : ptr(MS)));
        else if (i == rin_of(k)) CHECK(!before.p[i] && after.p[i] == (behind ? ptr(RDM) : ptr(TL)));
        else if (i == rout_of(k)) CHECK(!before.p[i] && after.p[i] == (takes ? ptr(OH) : nullptr));
        else if (i == last && had < 0) CHECK(before.p[i] == ptr(OH) && after.p[i] == ptr(TL));
        else if (i == had && takes) CHECK(before.p[i] == ptr(OH) && after.p[i] == nullptr);
        else if (i == kResDev && (behind || front)) CHECK(!before.p[i] && after.p[i] == ptr(RD));
        else if (i == rstems_of(S2R_MASTER_PCM) && front) CHECK(before.p[i] == ptr(MS) && after.p[i] == ptr(RD));
        else if (i == rin_of(S2R_MASTER_PCM) && front) CHECK(before.p[i] == ptr(TL) && after.p[i] == ptr(RDM));
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
        call.frames = 64; call.master = true; call.stems = true;
        for (int k = 0; k < S2R_BUS_STAGES; k++) call.on[k] = true;
        for (int k = 0; k < S2R_MASTER_STAGES; k++) call.run[k] = true;
        const Flat f = flat(route_of(call));
        for (int i = 0; i < kPointers; i++) CHECK(f.p[i] == nullptr);
    }
    int calls = 0;
    for (int master = 0; master < 2; master++)
        for (int subset = 0; subset < 1 << S2R_BUS_STAGES; subset++)
            for (int set = 0; set < (master ? 1 << (S2R_MASTER_STAGES - 1) : 1); set++)              // bit k - 1: master stage k is set
                for (int idle = 0; idle <= ((set >> (S2R_MASTER_RESAMPLER - 1) & set >> (S2R_MASTER_PCM - 1) & 1)); idle++)
                    for (int stems = 0; stems <= master; stems++) {
                        S2rPostCall call;
                        call.n_buses = 3; call.frames = 64; call.master = master != 0; call.stems = stems != 0;
                        for (int k = 0; k < S2R_BUS_STAGES; k++) call.on[k] = (subset >> k & 1) != 0;
                        call.run[S2R_MASTER_MIX] = call.master;
                        for (int k = 1; k < S2R_MASTER_STAGES; k++) call.run[k] = (set >> (k - 1) & 1) != 0;
                        if (idle) { call.run[S2R_MASTER_PCM] = false; call.pcm_idle = true; }
                        std::snprintf(what, sizeof what, "%s fill, stages %d%d%d%d%d%d%d%d, master stages %d%d%d%d%d%d%d, PCM idle %d, stems %d", master ? "master" : "bus",
                                      (int)call.on[0], (int)call.on[1], (int)call.on[2], (int)call.on[3], (int)call.on[4], (int)call.on[5], (int)call.on[6], (int)call.on[7],
                                      (int)call.run[0], (int)call.run[1], (int)call.run[2], (int)call.run[3], (int)call.run[4], (int)call.run[5], (int)call.run[6], idle, stems);
                        const S2rPostRoute r = route_of(call);
                        if (!(subset & ~kTabled) && !(set & ~(1 << (S2R_MASTER_LIMITER - 1)))) against_table(call, r, what);
                        if (master && !subset) against_master_table(call, r, what);
                        against_rule(call, r, what);
                        for (int k = 0; k < S2R_BUS_STAGES; k++) if (!call.on[k]) against_one_more(call, r, k, what);
                        for (int k = 1; master && k < S2R_MASTER_WRITERS; k++) if (!call.run[k]) against_one_more_writer(call, r, k, what);
                        for (int k = R0; master && k < S2R_MASTER_STAGES; k++)                      // (an idle PCM stage is set: it cannot be turned on)
                            if (!call.run[k] && !(k == S2R_MASTER_PCM && call.pcm_idle)) against_one_more_reader(call, r, k, what);
                        calls++;
                    }
    std::snprintf(what, sizeof what, "all calls");
    CHECK(calls == 256 * (1 + (64 + 16) * 2));
    for (int i = 0; i < 24; i++) CHECK(hits[i] == (kTable[i].master ? 2 : 1));       // (a master row holds for both values of stems)
    for (int i = 0; i < 12; i++) CHECK(master_hits[i] == 2);
    std::printf("route ok\n");
    return 0;
}
