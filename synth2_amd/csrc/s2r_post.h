// s2r_post.h — the chain behind the bus mixdown of s2r_fill_buses and s2r_fill_master: the buses' choruses, their
// feedback delays (4.19), their convolution reverbs (4.16), the master section (4.17) and the master limiter (4.18), in that order.  The chain owns what the five stages own and knows
// nothing of the handle: its functions take a S2rPostCtx and return the HIP error.  Per call: prepare, launch, — the caller's synchronise —
// commit, read_timers.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>

#include "s2r.h"
#include "s2r_device.h"

// what the chain is told of its handle: `timing` is s2r_set_timing, the two pointers the device's views of the pinned outputs
struct S2rPostCtx { hipStream_t stream; uint32_t max_frames; bool timing; float *bus_out_dev, *out_host_dev; };

// a pair of events around a stage's kernels, created by the first call that needs them, and the time between them
struct S2rPostTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    float ms = -1.0f;
    hipError_t begin(hipStream_t stream);
    hipError_t end(hipStream_t stream) { return hipEventRecord(ev[1], stream); }
    hipError_t read() { return hipEventElapsedTime(&ms, ev[0], ev[1]); }
    void destroy() { for (hipEvent_t &e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; } }
};

// every pointer of one call (s2r_post_route): the bus combine's, the chorus kernel's, the delay kernel's, the reverbs' kernels', the master kernel's and the limiter's
struct S2rPostRoute { float *combine_out, *chorus_in, *chorus_out, *delay_in, *delay_out, *fx_in, *fx_out, *master_in, *master_out, *master_stems, *limiter_in, *limiter_out; };
struct S2rPostCall {                                // one fill, as prepare leaves it
    uint32_t n_buses = 0, frames = 0;            // n_buses 0: a panned fill, which runs no stage
    bool master = false, stems = false;          // s2r_fill_master; the caller wants the stems too
    bool chorus_on = false;                      // a chorus sits on one of the call's buses
    bool delay_on = false;                       // a delay sits on one of the call's buses
    bool fx_on = false, limited = false;         // a reverb sits on one of the call's buses; a master fill with the limiter set
    S2rPostRoute route{};
};

// Who reads and writes what, the only place that decides it.  The combine writes into the first stem stage that runs, each running
// stage into the next running stage's input, and whichever stage writes the stems LAST writes them where the call wants them: the
// pinned output in a bus fill; the master's device stage in a master fill, whose kernel must not read pinned memory back and copies
// them out itself when the caller wants them.  The master kernel's two channels go to the pinned output unless the limiter follows
// and writes there in its place.  A stage that does not run has null pointers.
//   call         chorus delay reverb limiter | combine_out   chorus_in -> chorus_out       delay_in -> delay_out          fx_in -> fx_out             master_in     master_out    limiter_in -> _out
//   bus fill     no     no    no     -       | bus_out_dev   -                             -                              -                           -             -             -
//   bus fill     no     no    yes    -       | fx_stage      -                             -                              fx_stage -> bus_out_dev     -             -             -
//   bus fill     no     yes   no     -       | delay_stage   -                             delay_stage -> bus_out_dev     -                           -             -             -
//   bus fill     no     yes   yes    -       | delay_stage   -                             delay_stage -> fx_stage        fx_stage -> bus_out_dev     -             -             -
//   master fill  no     no    no     no      | master_stage  -                             -                              -                           master_stage  out_host_dev  -
//   master fill  no     no    yes    no      | fx_stage      -                             -                              fx_stage -> master_stage    master_stage  out_host_dev  -
//   master fill  no     yes   no     no      | delay_stage   -                             delay_stage -> master_stage    -                           master_stage  out_host_dev  -
//   master fill  no     yes   yes    no      | delay_stage   -                             delay_stage -> fx_stage        fx_stage -> master_stage    master_stage  out_host_dev  -
//   master fill  no     no    no     yes     | master_stage  -                             -                              -                           master_stage  limiter_in    limiter_in -> out_host_dev
//   master fill  no     no    yes    yes     | fx_stage      -                             -                              fx_stage -> master_stage    master_stage  limiter_in    limiter_in -> out_host_dev
//   master fill  no     yes   no     yes     | delay_stage   -                             delay_stage -> master_stage    -                           master_stage  limiter_in    limiter_in -> out_host_dev
//   master fill  no     yes   yes    yes     | delay_stage   -                             delay_stage -> fx_stage        fx_stage -> master_stage    master_stage  limiter_in    limiter_in -> out_host_dev
//   bus fill     yes    no    no     -       | chorus_stage  chorus_stage -> bus_out_dev   -                              -                           -             -             -
//   bus fill     yes    no    yes    -       | chorus_stage  chorus_stage -> fx_stage      -                              fx_stage -> bus_out_dev     -             -             -
//   bus fill     yes    yes   no     -       | chorus_stage  chorus_stage -> delay_stage   delay_stage -> bus_out_dev     -                           -             -             -
//   bus fill     yes    yes   yes    -       | chorus_stage  chorus_stage -> delay_stage   delay_stage -> fx_stage        fx_stage -> bus_out_dev     -             -             -
//   master fill  yes    no    no     no      | chorus_stage  chorus_stage -> master_stage  -                              -                           master_stage  out_host_dev  -
//   master fill  yes    no    yes    no      | chorus_stage  chorus_stage -> fx_stage      -                              fx_stage -> master_stage    master_stage  out_host_dev  -
//   master fill  yes    yes   no     no      | chorus_stage  chorus_stage -> delay_stage   delay_stage -> master_stage    -                           master_stage  out_host_dev  -
//   master fill  yes    yes   yes    no      | chorus_stage  chorus_stage -> delay_stage   delay_stage -> fx_stage        fx_stage -> master_stage    master_stage  out_host_dev  -
//   master fill  yes    no    no     yes     | chorus_stage  chorus_stage -> master_stage  -                              -                           master_stage  limiter_in    limiter_in -> out_host_dev
//   master fill  yes    no    yes    yes     | chorus_stage  chorus_stage -> fx_stage      -                              fx_stage -> master_stage    master_stage  limiter_in    limiter_in -> out_host_dev
//   master fill  yes    yes   no     yes     | chorus_stage  chorus_stage -> delay_stage   delay_stage -> master_stage    -                           master_stage  limiter_in    limiter_in -> out_host_dev
//   master fill  yes    yes   yes    yes     | chorus_stage  chorus_stage -> delay_stage   delay_stage -> fx_stage        fx_stage -> master_stage    master_stage  limiter_in    limiter_in -> out_host_dev
//   master_stems = bus_out_dev in a master fill with stems, else null.  A limiter that is set is idle in a bus fill, a chorus, a
//   delay or a reverb on a bus past the call's in any; a panned fill (no buses) has no route.
S2rPostRoute s2r_post_route(const S2rPostCall &call, float *chorus_stage, float *delay_stage, float *fx_stage, float *master_stage, float *limiter_in, float *bus_out_dev,
                            float *out_host_dev);

struct S2rPostChain {
    // The choruses (s2r_set_bus_chorus).  Everything of theirs is allocated when a chorus is set, never in a fill.
    struct BusChorus {
        uint32_t voices = 0;                     // V; 0: the bus has no chorus
        uint32_t history = 0;                    // H = floor(fl(base + depth)) + 1
        float base = 0.0f, depth = 0.0f, dry = 0.0f, wet = 0.0f;
        uint32_t phase_inc = 0, spread = 0;
        uint32_t phase = 0;                      // the LFO's phase at frame 0 of the next call: moved on by the commit
        float *line[2] = {nullptr, nullptr};     // [H][2] each, oldest frame first, L then R: line[cur] holds the history of the input, the kernel writes the other
        int cur = 0;
        void release() { for (float *p : line) if (p) (void)hipFree(p); *this = BusChorus{}; }
    } chorus[S2R_MAX_BUSES];
    float *chorus_stage = nullptr;               // [S2R_MAX_BUSES][2 * max_frames]: where the bus combine writes in a call that runs a chorus
    S2rPostTimer chorus_timer;                   // around the chorus kernel of the last bus or master fill: 0 when it ran none (tools/chorus_time.py)
    // The delays (s2r_set_bus_delay).  Everything of theirs is allocated when a delay is set, never in a fill.
    struct BusDelay {
        uint32_t delay = 0;                      // D; 0: the bus has no delay
        float feedback = 0.0f, cross = 0.0f, dry = 0.0f, wet = 0.0f;
        float *line[2] = {nullptr, nullptr};     // [D][2] each, oldest frame first, L then R: line[cur] holds the history, the kernel writes the other
        int cur = 0;
        void release() { for (float *p : line) if (p) (void)hipFree(p); *this = BusDelay{}; }
    } delay[S2R_MAX_BUSES];
    float *delay_stage = nullptr;                // [S2R_MAX_BUSES][2 * max_frames]: where the bus combine writes in a call that runs a delay
    S2rPostTimer delay_timer;                    // around the delay kernel of the last bus or master fill: 0 when it ran none (tools/delay_time.py)
    // The reverbs (s2r_set_bus_reverb).  Everything of theirs is allocated when a reverb is set, never in a fill.
    struct BusFx {
        uint32_t n_taps = 0;                     // K; 0: the bus has no reverb
        float dry = 0.0f, wet = 0.0f;
        float *taps = nullptr;                   // [2][tstride]: ir_L, ir_R, padded with +0.0 up to whole segments
        float *line[2] = {nullptr, nullptr};     // [2][lstride] each: K - 1 frames of history per channel in front of a call's dry frames; line[cur] holds the history
        float *partials = nullptr;               // [2][n_seg][pstride]
        uint32_t tstride = 0, lstride = 0;
        int cur = 0;
        void release() { for (float *p : {taps, line[0], line[1], partials}) if (p) (void)hipFree(p); *this = BusFx{}; }
    } fx[S2R_MAX_BUSES];
    float *fx_stage = nullptr;                   // [S2R_MAX_BUSES][2 * max_frames]: where the bus combine writes in a call that runs a reverb
    S2rPostTimer fx_timer;                          // around the reverbs' kernels of the last bus or master fill: 0 when it ran none (tools/reverb_time.py)
    // The master section.  Nothing is allocated before the first master fill.
    struct Master {
        float ret[S2R_MAX_BUSES], ret_app[S2R_MAX_BUSES];        // what the caller last set — the target — and what the last master fill left — the applied
        float fader = 1.0f, fader_app = 1.0f;
        float *stage = nullptr;                  // [S2R_MAX_BUSES][2 * max_frames] in device memory: where the last stem writer of a master fill writes
        float *partials = nullptr, *partials_dev = nullptr;      // pinned and device-mapped: [ceil(max_frames / S2R_METER_BLOCK)][S2R_MASTER_ROW]
        bool metered = false;                    // a master fill has succeeded: the meters below are its
        uint32_t meter_buses = 0;
        float peak[S2R_MASTER_CH], energy[S2R_MASTER_CH];
        S2rPostTimer timer;                         // around the master kernel of the last master fill (tools/master_time.py)
        Master() { for (uint32_t b = 0; b < S2R_MAX_BUSES; b++) ret[b] = ret_app[b] = 1.0f; }
    } master;
    // The master limiter.  Nothing is allocated before the first master fill that finds it set.
    struct Limiter {
        float ceiling = 0.0f;
        uint32_t lookahead = 0, hold = 0;        // lookahead 0: off
        // The state — xh [lookahead][2], then gh [2 * lookahead + hold] — lives in `host` while host_valid (set, reset or restored since
        // the last fill) and in state[cur] otherwise: a fill uploads a valid host copy, the kernel writes state[cur ^ 1], the commit flips.
        std::vector<float> host;
        bool host_valid = false;
        float *state[2] = {nullptr, nullptr};    // device memory, each 2 * S2R_LIMITER_MAX_LOOKAHEAD + (2 * S2R_LIMITER_MAX_LOOKAHEAD + S2R_LIMITER_MAX_HOLD) floats
        int cur = 0;
        float *in = nullptr;                     // [2 * max_frames] in device memory: where the master kernel writes when the limiter is on
        float *partials = nullptr, *partials_dev = nullptr;      // pinned and device-mapped: [ceil(max_frames / S2R_LIMITER_BLOCK)][2]
        bool metered = false;                    // a master fill has run the limiter: the meters below are its
        float min_gain = 1.0f, out_peak = 0.0f;
        S2rPostTimer timer;                         // around the limiter kernel of the last master fill: 0 when it ran none (tools/limiter_time.py)
        size_t n_x() const { return 2u * (size_t)lookahead; }
        size_t n_g() const { return 2u * (size_t)lookahead + hold; }
    } limiter;
    // one fill: what it runs, its once-only allocations and its route; the launches in order, each between its timer's marks; after
    // the synchronise that succeeded, and only then, histories, applied values and state move on and the meters fold
    hipError_t prepare(const S2rPostCtx &c, uint32_t n_buses, uint32_t frames, bool master_fill, bool stems, S2rPostCall &call);
    hipError_t launch(const S2rPostCtx &c, const S2rPostCall &call);
    void commit(const S2rPostCall &call);
    hipError_t read_timers(const S2rPostCall &call);
    void release();
    // what the entry points of s2r_host.cpp do behind their checks, on a quiet stream
    hipError_t set_chorus(const S2rPostCtx &c, uint32_t bus, uint32_t voices, float base, float depth, uint32_t phase_inc, uint32_t spread, float dry, float wet);
    hipError_t chorus_state(const S2rPostCtx &c, uint32_t bus, float *get, const float *set);       // the history: frames, oldest first, L then R
    hipError_t set_delay(const S2rPostCtx &c, uint32_t bus, uint32_t delay_frames, float feedback, float cross, float dry, float wet);
    hipError_t delay_history(const S2rPostCtx &c, uint32_t bus, float *get, const float *set);      // frames, oldest first, L then R
    hipError_t set_reverb(const S2rPostCtx &c, uint32_t bus, const float *ir_l, const float *ir_r, uint32_t n_taps, float dry, float wet);
    hipError_t reverb_history(const S2rPostCtx &c, uint32_t bus, float *get, const float *set);     // frames, oldest first, L then R
    void snap_master() { for (uint32_t b = 0; b < S2R_MAX_BUSES; b++) master.ret_app[b] = master.ret[b]; master.fader_app = master.fader; }
    void set_limiter(float ceiling, uint32_t lookahead, uint32_t hold);      // (0, 0, 0): off
    void set_limiter_state(const float *xh, const float *gh);
    hipError_t fetch_limiter_state(const S2rPostCtx &c);            // the device's copy into `host`, kept until the next fill
};
