// s2r_mixer.h — the device side of the voice mixer: the gains' staging buffers and their device copies, the
// rows buffer the render kernel fills slice by slice, the mixdowns' partial rows, the bus fill's pinned output and the timers around
// the mixdown kernels.  S2rVoiceMixer owns these and knows nothing of the handle: s2r_host_mix.cpp tells it what it needs (S2rMixCtx)
// and renders the rows itself.  What the gains are made from is S2rMixerKeep's (s2r_mixer_keep.h).  Compiled with hipcc.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>

#include "s2r.h"
#include "s2r_device.h"
#include "s2r_mixer_keep.h"

// what the mixer is told of its handle: `timing` is s2r_set_timing, out_host_dev the device's view of the panned fill's pinned output
struct S2rMixCtx {
    hipStream_t stream;
    uint32_t shard_voices, padded_voices, block_voices, n_blocks, mix_groups, max_frames;
    bool timing;
    float *out_host_dev;
};

class S2rVoiceMixer {
public:
    // The once-only allocations of a panned (n_buses == 0) or bus fill: the rows buffer, the partial rows of the mixdown asked for
    // and, for a bus fill whose caller wants the stems, their pinned output.  Starts the fill's timers over.
    hipError_t prepare(const S2rMixCtx &c, uint32_t n_buses, bool stems);
    // the gains of the voices' pans, from pinned memory to the device on the handle's stream (when a pan changed) ...
    hipError_t send_pan_gains(const S2rMixCtx &c, S2rMixerKeep &keep);
    // ... and what the bus mixdown reads per voice (when a pan, a mix, a send or a fader changed, or the last fill was ramped and
    // this one is not, or the reverse); `ramp`, `total`: S2rMixerKeep::stage_bus
    hipError_t send_bus_gains(const S2rMixCtx &c, S2rMixerKeep &keep, bool ramp, uint32_t total);
    // sends come into use while the staging buffer exists: it is laid out anew (S2rBusLayout), so nothing stale stays in it
    hipError_t sends_begin(const S2rMixCtx &c);
    // One slice's mixdown between its timer marks: `len` frames of rows() that begin at frame `at` of the call, into the mapped
    // output (panned) or into `bus_dst` (a bus fill of `total` frames; `ramp`: told where in the call the slice begins).
    hipError_t mix_slice(const S2rMixCtx &c, bool sends, uint32_t at, uint32_t len, uint32_t n_buses, uint32_t total, bool ramp, float *bus_dst);
    // the timers' read-out behind the fill: the sum over its slices
    hipError_t read_timers(uint32_t n_buses);
    void release();

    float *rows() const { return pan_rows; }                 // [shard_voices][slice()]: what the render kernel writes
    uint32_t slice() const { return pan_slice; }             // frames per slice, a multiple of 16 (0: not allocated yet)
    float *stems_dev() const { return bus_out_dev; }         // the bus fill's pinned output, as the device and as the host see it
    const float *stems() const { return bus_out; }
    float mix_ms(bool buses) const { return buses ? bus_mix_ms : pan_mix_ms; }       // device time of the last panned / bus fill's mixdowns

private:
    float *gains_host = nullptr, *gains_dev = nullptr;   // the panned fill's [2][padded_voices]: gL then gR (pinned / device); entries past the shard hold 0
    hipEvent_t gains_sent = nullptr;             // behind the last copy out of gains_host
    float *pan_rows = nullptr;                   // [shard_voices][pan_slice]: the voices' rows of one slice (allocated by the first panned or bus fill)
    uint32_t pan_slice = 0;                      // frames per slice, a multiple of 16
    float *pan_partials = nullptr;               // [n_blocks][2][pan_slice]
    std::vector<hipEvent_t> pan_ev;              // s2r_set_timing: a pair of events around every slice's mixdown of the last panned or bus fill
    size_t pan_ev_used = 0;
    float pan_mix_ms = -1.0f;                    // ... and their sum (tools/pan_time.py reads it through s2r_debug_pan_mix_ms)
    char *bus_gains_host = nullptr, *bus_gains_dev = nullptr;    // the bus fill's staging buffer (S2rBusLayout)
    hipEvent_t bus_gains_sent = nullptr;
    float *bus_partials = nullptr;               // [n_blocks][S2R_MAX_BUSES][2][pan_slice], allocated by the first bus fill
    float *bus_out = nullptr, *bus_out_dev = nullptr;            // pinned and device-mapped: S2R_MAX_BUSES * 2 * max_frames floats
    float bus_mix_ms = -1.0f;                    // pan_mix_ms of the last s2r_fill_buses (tools/bus_time.py)
    bool bus_dev_ramped = false;                 // what bus_gains_dev holds was sent for a ramped fill: (G0, step), not the static gains
};
