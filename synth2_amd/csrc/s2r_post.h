// s2r_post.h — the chain behind the bus mixdown of s2r_fill_buses and s2r_fill_master: the eight bus stages in the order of
// S2rBusStage (s2r_post_route.h) — the buses' equalisers, their dynamics (4.22), drives (4.24), flangers (4.25),
// choruses (4.20), feedback delays (4.19), convolution reverbs (4.16) and rooms (4.23) —, then the master section (4.17), the master's multiband compressor (4.31) and the master
// limiter (4.18), and behind it the loudness and true-peak meters (4.26), the spectrum meters (4.27), the sample-rate converter (4.29) and the PCM stage (4.28) — the seven master
// stages, in the order of S2rMasterStage.  The bus stages keep their histories in a S2rBusLine each; the stages behind the master
// fader keep their state in a S2rMirror each, and the two meters their rows in a S2rRowStore each (s2r_post_keep.h); what else a
// master stage holds on the device is a S2rDevBuf or a S2rDevTable, what it shares with the host a S2rPinned.  The chain owns what
// these stages own and knows nothing of the handle: its functions take a S2rPostCtx and return the HIP error.  Per call: prepare —
// which alone decides what runs (call.on, call.run) and, through s2r_post_route, who reads and writes what —, launch — a walk over
// the two stage lists —, the caller's synchronise, commit, read_timers.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>

#include "s2r.h"
#include "s2r_device.h"
#include "s2r_post_keep.h"
#include "s2r_post_route.h"

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

// A bus effect's history on the device, double-buffered: line[cur] holds it, the call's kernel writes the other and the commit flips,
// so that a call that fails leaves the history where it was.  Allocated when the effect is set, never in a fill; an effect that is
// set has its lines, and no other has.
struct S2rBusLine {
    float *line[2] = {nullptr, nullptr};         // `floats` each
    int cur = 0;
    size_t floats = 0;
    uint32_t history = 0;                        // the frames of history the effect carries from call to call (s2r_get_bus_*_history)
    bool present() const { return line[0] != nullptr; }
    float *now() const { return line[cur]; }
    float *next() const { return line[cur ^ 1]; }
    void flip() { cur ^= 1; }
    hipError_t alloc(size_t n);
    hipError_t zero(int which, hipStream_t stream) { return hipMemsetAsync(line[which], 0, floats * sizeof(float), stream); }  // +0.0 everywhere
    // `n` floats at `at` of the current line to `get`, or from `set`; the caller synchronises
    hipError_t copy(float *get, const float *set, size_t at, size_t n, hipStream_t stream) const;
    // (not virtual: an effect with more device memory than its lines frees it in a free() of its own, and is dropped by its type)
    void free() { for (float *&p : line) if (p) { (void)hipFree(p); p = nullptr; } }
};

// The device side of a master stage's state (S2rMirrorHost, s2r_post_keep.h): the two copies, allocated by the first master fill that
// finds the stage set.  A fill reads now() — behind upload(), which sends a valid host copy there — and writes next(); committed() flips.
struct S2rMirror : S2rMirrorHost {
    float *dev[2] = {nullptr, nullptr};          // device memory, `floats` each
    size_t floats = 0;
    float *now() const { return dev[cur]; }
    float *next() const { return dev[cur ^ 1]; }
    hipError_t reserve(size_t n);                // at least n floats each: allocates what is missing, and regrows only while the host copy is valid
    hipError_t upload(hipStream_t stream) const; // nothing unless the host copy is valid; it stays so until the commit
    hipError_t fetch(hipStream_t stream);        // the device's copy into `host`, kept until the next fill; synchronises; a failure leaves `host` as it was
    void free() { for (float *&p : dev) if (p) { (void)hipFree(p); p = nullptr; } floats = 0; }
};

// Device memory that a fill reserves: at least n floats, allocated by the first that asks and regrown — what it held is gone then —
// by one that asks for more.
struct S2rDevBuf {
    float *dev = nullptr;
    size_t floats = 0;
    hipError_t reserve(size_t n);
    void free() { if (dev) (void)hipFree(dev); dev = nullptr; floats = 0; }
};
// ... that holds a table of the host's, good while `valid`: never after a regrowth or a set, from the commit of a fill that sent it on
struct S2rDevTable : S2rDevBuf {
    bool valid = false;
    hipError_t reserve(size_t n) { if (n > floats) valid = false; return S2rDevBuf::reserve(n); }
    hipError_t send(const std::vector<float> &host, size_t at, hipStream_t stream) const;       // to dev + at; nothing while valid
    void committed() { valid = true; }
};
// Pinned memory that the device sees at `dev` and the host reads behind a synchronise: at least n of T, grown as a S2rDevBuf is.
// `host` survives a failed hipHostGetDevicePointer, and the next call goes on from there.
template <class T> struct S2rPinned {
    T *host = nullptr, *dev = nullptr;
    size_t count = 0;
    bool grows(size_t n) const { return n > count; }             // reserve(n) would drop what it holds
    hipError_t reserve(size_t n);
    void free() { if (host) (void)hipHostFree(host); host = dev = nullptr; count = 0; }
};

struct S2rPostChain {
    // what a bus stage keeps beside its buses' effects
    struct Stem {
        float *buffer = nullptr;                 // [S2R_MAX_BUSES][2 * max_frames]: the stage's input in a call that runs it, allocated when its effect is first set
        S2rPostTimer timer;                      // around the stage's kernels of the last bus or master fill: 0 when it ran none (tools/*_time.py)
    } stage[S2R_BUS_STAGES];
    // The effects, in chain order.
    // The EQs (s2r_set_bus_eq): lines of [n_bands][s1_L, s1_R, s2_L, s2_R], 4 * n_bands floats (history = 2 * n_bands "frames" of two)
    struct BusEq : S2rBusLine {
        uint32_t n_bands = 0;
        float c[S2R_EQ_MAX_BANDS][5] = {};       // (b0, b1, b2, a1, a2) per band
    } eq[S2R_MAX_BUSES];
    // The dynamics (s2r_set_bus_dynamics): lines of one float, the gain y; beside them the curves' tables on the device and a pinned row
    // for the calls' meters
    struct BusDyn : S2rBusLine {
        uint32_t key = 0;
        float a_att = 0.0f, a_rel = 0.0f;
        float min_gain = 1.0f;                   // the meter of the last successful call that ran these dynamics
        std::vector<float> curve;                // the host's copy of the table: S2R_DYN_CURVE_POINTS entries
    } dyn[S2R_MAX_BUSES];
    S2rDevBuf dyn_curves;                        // [S2R_MAX_BUSES][S2R_DYN_CURVE_POINTS], allocated when dynamics are first set
    S2rPinned<float> dyn_meter;                  // [S2R_MAX_BUSES]
    // The drives (s2r_set_bus_drive): lines of [S2R_DRIVE_HISTORY][2], the bus's last input frames, oldest first, L then R; beside them
    // the tables on the device
    struct BusDrive : S2rBusLine {
        float pre = 0.0f, dry = 0.0f, wet = 0.0f;
        std::vector<float> curve;                // the host's copy of the table: S2R_DRIVE_CURVE_POINTS entries
    } drive[S2R_MAX_BUSES];
    S2rDevBuf drive_curves;                      // [S2R_MAX_BUSES][S2R_DRIVE_CURVE_POINTS], allocated when a drive is first set
    // The flangers (s2r_set_bus_flanger): lines of [H][2], the last frames of the stage's line signal w, oldest first, L then R, H =
    // history = floor(fl(base + depth)) + 1
    struct BusFlanger : S2rBusLine {
        float base = 0.0f, depth = 0.0f, feedback = 0.0f, cross = 0.0f, dry = 0.0f, wet = 0.0f;
        uint32_t phase_inc = 0, spread = 0;
        uint32_t phase = 0;                      // the LFO's phase at frame 0 of the next call: moved on by the commit
    } flanger[S2R_MAX_BUSES];
    // The choruses (s2r_set_bus_chorus): lines of [H][2], oldest frame first, L then R, H = history = floor(fl(base + depth)) + 1
    struct BusChorus : S2rBusLine {
        uint32_t voices = 0;                     // V
        float base = 0.0f, depth = 0.0f, dry = 0.0f, wet = 0.0f;
        uint32_t phase_inc = 0, spread = 0;
        uint32_t phase = 0;                      // the LFO's phase at frame 0 of the next call: moved on by the commit
    } chorus[S2R_MAX_BUSES];
    // The delays (s2r_set_bus_delay): lines of [D][2], oldest frame first, L then R, D = history
    struct BusDelay : S2rBusLine {
        float feedback = 0.0f, cross = 0.0f, dry = 0.0f, wet = 0.0f;
    } delay[S2R_MAX_BUSES];
    // The reverbs (s2r_set_bus_reverb): lines of [2][lstride], history = K - 1 frames per channel in front of a call's dry frames
    struct BusFx : S2rBusLine {
        uint32_t n_taps = 0;                     // K
        float dry = 0.0f, wet = 0.0f;
        float *taps = nullptr;                   // [2][tstride]: ir_L, ir_R, padded with +0.0 up to whole segments
        float *partials = nullptr;               // [2][n_seg][pstride]
        uint32_t tstride = 0, lstride = 0;
        void free() { for (float *p : {taps, partials}) if (p) (void)hipFree(p); S2rBusLine::free(); }
    } fx[S2R_MAX_BUSES];
    // The rooms (s2r_set_bus_room): lines in the checkpoint's layout (s2r.h): per channel each comb's line and its f, then each allpass's
    // line; a room also owns the work area its kernel keeps a call's frames of the 24 lines in
    struct BusRoom : S2rBusLine {
        uint32_t cd[S2R_ROOM_COMBS] = {}, ad[S2R_ROOM_ALLPASSES] = {}, spread = 0;
        float feedback = 0.0f, damp = 0.0f, d1 = 0.0f, g = 0.0f, gain = 0.0f, dry = 0.0f, wet = 0.0f, cross = 0.0f;
        float *work = nullptr;                   // [S2R_ROOM_LINES][max_frames]
        void free() { if (work) (void)hipFree(work); work = nullptr; S2rBusLine::free(); }
    } room[S2R_MAX_BUSES];
    // stage k's effect on a bus, as far as the stages are alike
    template <class Line, class Chain> static Line &bus_of(Chain &c, int k, uint32_t b) {
        Line *const of[S2R_BUS_STAGES] = {&c.eq[b], &c.dyn[b], &c.drive[b], &c.flanger[b], &c.chorus[b], &c.delay[b], &c.fx[b], &c.room[b]};
        return *of[k];
    }
    S2rBusLine &bus(int k, uint32_t b) { return bus_of<S2rBusLine>(*this, k, b); }
    const S2rBusLine &bus(int k, uint32_t b) const { return bus_of<const S2rBusLine>(*this, k, b); }
    // the bus's effect of stage k runs in a call of n_buses buses: the bus is among them (an effect on a bus past the call's is idle in
    // it), and for the dynamics their key bus too
    bool runs(int k, uint32_t b, uint32_t n_buses) const { return b < n_buses && bus(k, b).present() && (k != S2R_BUS_DYN || dyn[b].key < n_buses); }
    // The master stages.  Each one's timer, by S2rMasterStage: around its kernel in the last master fill, 0 when that ran none
    // (tools/master_time.py, limiter_time.py, loudness_time.py, spectrum_time.py, pcm_time.py, resampler_time.py, multiband_time.py)
    S2rPostTimer master_timer[S2R_MASTER_STAGES];
    // The master section.  Nothing is allocated before the first master fill.
    struct Master {
        float ret[S2R_MAX_BUSES], ret_app[S2R_MAX_BUSES];        // what the caller last set — the target — and what the last master fill left — the applied
        float fader = 1.0f, fader_app = 1.0f;
        S2rDevBuf stage;                         // [S2R_MAX_BUSES][2 * max_frames]: where the last stem writer of a master fill writes
        S2rPinned<float> partials;               // [ceil(max_frames / S2R_METER_BLOCK)][S2R_MASTER_ROW]
        bool metered = false;                    // a master fill has succeeded: the meters below are its
        uint32_t meter_buses = 0;
        float peak[S2R_MASTER_CH], energy[S2R_MASTER_CH];
        Master() { for (uint32_t b = 0; b < S2R_MAX_BUSES; b++) ret[b] = ret_app[b] = 1.0f; }
    } master;
    // The master limiter.  Nothing is allocated before the first master fill that finds it set.
    struct Limiter {
        float ceiling = 0.0f;
        uint32_t lookahead = 0, hold = 0;        // lookahead 0: off
        uint32_t detector = 0;                   // S2R_LIMITER_SAMPLE_PEAK, or S2R_LIMITER_TRUE_PEAK: its own kernel, 16 frames more of xh
        // xh [lookahead][2] ([lookahead + 16][2] with the true-peak detector), then gh [2 * lookahead + hold], on the host and on the
        // device alike: n_x() + n_g() floats, in copies sized for the largest lookahead and hold
        S2rMirror state;
        S2rDevBuf in;                            // [2 * max_frames]: where the writer in front writes when the limiter is on
        S2rPinned<float> partials;               // [ceil(max_frames / S2R_LIMITER_BLOCK)][2]
        bool metered = false;                    // a master fill has run the limiter: the meters below are its
        float min_gain = 1.0f, out_peak = 0.0f;
        size_t n_x() const { return 2u * ((size_t)lookahead + (detector == S2R_LIMITER_TRUE_PEAK ? S2R_LIMITER_TP_HISTORY : 0u)); }
        size_t n_g() const { return 2u * (size_t)lookahead + hold; }
    } limiter;
    // The loudness and true-peak meters (s2r_set_master_loudness).  Nothing is allocated before the first master fill
    // that finds the meter set, and a handle on which it never was passes the pointers and makes the launches it always did.
    struct Loudness {
        float c[10] = {};
        uint32_t hop = 0;                        // 0: off
        S2rMirror state;                         // S2R_LOUDNESS_STATE floats
        uint32_t pos = 0;                        // the frames of the hop under way: the host's alone, and a kernel argument
        S2rDevBuf in;                            // [2 * max_frames]: the tail's input, where the master's last writer writes when any of the four readers is on
        S2rPinned<float> rows;                   // [max_frames / 16 + 1][S2R_LOUDNESS_CHANNELS]
        S2rPinned<float> peaks;                  // [ceil(max_frames / S2R_LOUDNESS_BLOCK)][2]
        S2rRowStore kept;                        // the hop rows kept: S2R_LOUDNESS_CHANNELS floats each, at most max_hops of them
        float tp_last[2] = {0.0f, 0.0f}, tp_held[2] = {0.0f, 0.0f};
    } loud;
    // The spectrum meters (s2r_set_master_spectrum), behind the loudness meters.  As theirs: nothing is allocated before
    // the first master fill that finds the meter set — and what is allocated then is sized by n_fft and hop, and grown by a later fill
    // that finds them larger —, and a handle on which it never was set makes the launches it always did.
    struct Spectrum {
        uint32_t n_fft = 0, hop = 0;             // both 0: off
        std::vector<float> window, twiddles;     // [n_fft] and [n_fft / 2][2], the host's
        S2rMirror state;                         // S2R_SPECTRUM_STATE(n_fft) floats
        uint32_t pos = 0;                        // the frames of the hop under way: the host's alone, and a kernel argument
        S2rDevTable tables;                      // window [n_fft], then twiddles [n_fft / 2][2]
        S2rPinned<float> rows;                   // [max_frames / hop + 1][9][n_fft / 2 + 1]
        S2rRowStore kept;                        // the rows kept: S2R_SPECTRUM_ROW(n_fft) floats each, at most max_rows of them
    } spec;
    // The PCM stage (s2r_set_master_pcm), behind the spectrum meters, the last of a master fill.  As theirs: nothing is
    // allocated before the first master fill that finds the stage set, and a handle on which it never was set makes the launches it
    // always did.
    struct Pcm {
        uint32_t bits = 0, dither = 0, n_taps = 0, seed = 0;     // bits 0: off
        float h[S2R_PCM_MAX_TAPS] = {};          // +0.0 past n_taps
        S2rMirror state;                         // S2R_PCM_STATE floats
        uint32_t t = 0;                          // the frames converted since the set or reset, mod 2^32: the host's alone, and a kernel argument
        S2rPinned<int32_t> samples;              // [9][cap()][2]
        // max_frames, or the resampler's S2R_RESAMPLER_MAX_OUT when a fill found that set: grown, never shrunk
        uint32_t cap() const { return (uint32_t)(samples.count / (2u * S2R_PCM_PROGRAMMES)); }
        bool have = false;                       // a master fill has run the stage since the set or reset: `frames` (0 with the resampler in front) is its
        S2rPinned<uint32_t> counts;              // [S2R_PCM_CHANNELS], the call's clips
        uint32_t frames = 0;                     // the frames of the last successful fill that ran the stage
        uint32_t clips_last[S2R_PCM_CHANNELS] = {}, clips_held[S2R_PCM_CHANNELS] = {};
    } pcm;
    // The sample-rate converter (s2r_set_master_resampler), behind the spectrum meters and in front of the PCM stage.  As
    // theirs: nothing is allocated before the first master fill that finds the stage set — and what is allocated then is sized by L, M
    // and T, and grown by a later fill that finds them larger —, and a handle on which it never was set makes the launches it always did.
    struct Resampler {
        uint32_t L = 0, M = 0, T = 0;            // L 0: off
        std::vector<float> table;                // [L][T], the host's
        S2rDevTable table_dev;
        S2rMirror state;                         // S2R_RESAMPLER_STATE(T) floats
        uint32_t ph = 0;                         // the next output's position in 1 / L input frames: the host's alone, and a kernel argument
        S2rPinned<float> res;                    // [9][cap()][2], the call's outputs
        S2rDevBuf res_dev;                       // as much: the PCM kernel's input, allocated when a fill finds both stages set
        uint32_t cap() const { return (uint32_t)(res.count / (2u * S2R_RESAMPLER_PROGRAMMES)); }        // S2R_RESAMPLER_MAX_OUT(max_frames, L, M) when it was allocated
        uint32_t call_count = 0;                 // the output frames of the call under way (prepare)
        bool have = false;                       // a master fill has run the stage since the set or reset: `count` is its
        uint32_t count = 0;
    } res;
    // The master's multiband compressor (s2r_set_master_multiband), behind the master kernel and in front of the limiter.
    // As the stages above: nothing is allocated before the first master fill that finds the stage set, and a handle on which it never was
    // set makes the launches it always did.  A writer of the route (s2r_post_route.h) as the limiter is: in a call that runs it the
    // master kernel writes `in`, and the stage's kernel writes where that would have.
    struct Multiband {
        uint32_t n_bands = 0;                    // B; 0: off
        float lp[S2R_MULTIBAND_MAX_BANDS - 1u][5] = {}, hp[S2R_MULTIBAND_MAX_BANDS - 1u][5] = {}, ap[S2R_MULTIBAND_MAX_BANDS - 2u][5] = {};
        float a_att[S2R_MULTIBAND_MAX_BANDS] = {}, a_rel[S2R_MULTIBAND_MAX_BANDS] = {};
        std::vector<float> curves;               // the host's copy of the tables: [B][S2R_DYN_CURVE_POINTS]
        S2rDevTable curves_dev;                  // [S2R_MULTIBAND_MAX_BANDS][S2R_DYN_CURVE_POINTS]
        S2rMirror state;                         // S2R_MULTIBAND_STATE(B) floats, in copies sized for four bands
        S2rDevBuf in;                            // [2 * max_frames]: where the master kernel writes when the stage is on
        S2rPinned<float> meter;                  // [S2R_MULTIBAND_MAX_BANDS], the call's minima
        bool metered = false;                    // a master fill has run the stage since the set or reset: the minima below are its
        float min_gain[S2R_MULTIBAND_MAX_BANDS] = {1.0f, 1.0f, 1.0f, 1.0f};
    } mb;
    // one fill: what it runs, its once-only allocations and its route; the launches in order, each between its timer's marks; after
    // the synchronise that succeeded, and only then, histories, applied values and state move on and the meters fold
    hipError_t prepare(const S2rPostCtx &c, uint32_t n_buses, uint32_t frames, bool master_fill, bool stems, S2rPostCall &call);
    hipError_t launch(const S2rPostCtx &c, const S2rPostCall &call);
    // a bus stage's part of launch: its kernels' arguments from the buses' effects and route.stage[k], and the launch
    hipError_t launch_eq(const S2rPostCtx &c, const S2rPostCall &call) const;
    hipError_t launch_dyn(const S2rPostCtx &c, const S2rPostCall &call) const;
    hipError_t launch_drive(const S2rPostCtx &c, const S2rPostCall &call) const;
    hipError_t launch_flanger(const S2rPostCtx &c, const S2rPostCall &call) const;
    hipError_t launch_chorus(const S2rPostCtx &c, const S2rPostCall &call) const;
    hipError_t launch_delay(const S2rPostCtx &c, const S2rPostCall &call) const;
    hipError_t launch_reverb(const S2rPostCtx &c, const S2rPostCall &call) const;
    hipError_t launch_room(const S2rPostCtx &c, const S2rPostCall &call) const;
    // a master stage's part: what is still to be sent to the device — tables, a state set on the host —, the kernel's arguments from
    // route.writer or route.reader, and the launch
    hipError_t launch_master(const S2rPostCtx &c, const S2rPostCall &call) const;
    hipError_t launch_multiband(const S2rPostCtx &c, const S2rPostCall &call) const;
    hipError_t launch_limiter(const S2rPostCtx &c, const S2rPostCall &call) const;
    hipError_t launch_loudness(const S2rPostCtx &c, const S2rPostCall &call) const;
    hipError_t launch_spectrum(const S2rPostCtx &c, const S2rPostCall &call) const;
    hipError_t launch_resampler(const S2rPostCtx &c, const S2rPostCall &call) const;
    hipError_t launch_pcm(const S2rPostCtx &c, const S2rPostCall &call) const;
    void commit(const S2rPostCall &call);
    hipError_t read_timers(const S2rPostCall &call);
    void release();
    // what the entry points of s2r_host_post.cpp do behind their checks, on a quiet stream; in chain order
    hipError_t set_eq(const S2rPostCtx &c, uint32_t bus, uint32_t n_bands, const float *coeffs);
    // curve null: removes the bus's dynamics; keep_state: the parameters alone, on a bus that has them
    hipError_t set_dyn(const S2rPostCtx &c, uint32_t bus, uint32_t key, const float *curve, float a_att, float a_rel, bool keep_state);
    // pre < 0: removes the bus's drive; keep_state: the levels, and the table unless curve is null, on a bus that has one
    hipError_t set_drive(const S2rPostCtx &c, uint32_t bus, const float *curve, float pre, float dry, float wet, bool keep_state);
    // base < 0: removes the bus's flanger
    hipError_t set_flanger(const S2rPostCtx &c, uint32_t bus, float base, float depth, uint32_t phase_inc, uint32_t spread, float feedback, float cross, float dry,
                           float wet);
    hipError_t set_chorus(const S2rPostCtx &c, uint32_t bus, uint32_t voices, float base, float depth, uint32_t phase_inc, uint32_t spread, float dry, float wet);
    hipError_t set_delay(const S2rPostCtx &c, uint32_t bus, uint32_t delay_frames, float feedback, float cross, float dry, float wet);
    hipError_t set_reverb(const S2rPostCtx &c, uint32_t bus, const float *ir_l, const float *ir_r, uint32_t n_taps, float dry, float wet);
    // cd null: removes the bus's room; the levels alone on a bus that has one: set_room_params
    hipError_t set_room(const S2rPostCtx &c, uint32_t bus, const uint32_t *cd, const uint32_t *ad, uint32_t spread, const float levels[7]);
    void set_room_params(uint32_t bus, const float levels[7]);
    // the whole state of stage k's effect on a bus — all the floats of its line —, out or in (the EQ's, the dynamics', the room's)
    hipError_t state(const S2rPostCtx &c, int k, uint32_t bus, float *get, const float *set);
    // the history of stage k's effect on a bus, out or in: `history` frames, oldest first, L then R
    hipError_t history(const S2rPostCtx &c, int k, uint32_t bus, float *get, const float *set);
    void snap_master() { for (uint32_t b = 0; b < S2R_MAX_BUSES; b++) master.ret_app[b] = master.ret[b]; master.fader_app = master.fader; }
    void set_limiter(float ceiling, uint32_t lookahead, uint32_t hold, uint32_t detector);      // (0, 0, 0, 0): off
    void set_limiter_state(const float *xh, const float *gh);
    // n_bands 0: off; keep_state: the parameters alone, with the n_bands that is set; else on, from the initial state
    void set_multiband(uint32_t n_bands, const float *lp, const float *hp, const float *ap, const float *curves, const float *a_att, const float *a_rel,
                       bool keep_state);
    void reset_multiband();                                         // state and meters; the parameters stay
    void set_loudness(const float *coeffs, uint32_t hop, uint32_t max_hops);  // coeffs null: off; else on, from the initial state
    void reset_loudness();                                          // state, rows and held true peak; the parameters stay
    void set_spectrum(uint32_t n_fft, uint32_t hop, const float *window, uint32_t max_rows);   // window null: off; else on, from the initial state
    void reset_spectrum();                                          // state and rows; the parameters stay
    void set_pcm(uint32_t bits, uint32_t dither, const float *taps, uint32_t n_taps, uint32_t seed);     // bits 0: off; else on, from the initial state
    void reset_pcm();                                               // state, t, counts and the last samples; the parameters stay
    void set_pcm_state(const float *state, uint32_t t);             // the first n_taps errors of every row, +0.0 past them
    void set_resampler(uint32_t L, uint32_t M, uint32_t T, const float *table);        // table null: off; else on, from the initial state
    void reset_resampler();                                         // state, ph and the last outputs; the parameters stay
    void set_resampler_state(const float *state, uint32_t ph);
};
