// s2r_post.cpp — the post-mix chain (s2r_post.h): the eight bus stages (EQs, dynamics, drives, flangers, choruses, delays, reverbs, rooms), master section, master multiband compressor, master limiter, loudness meters, spectrum meters, sample-rate converter, PCM stage —
// the last five on the device side of s2r_post_keep.h (S2rMirror).  Compiled with hipcc, -ffp-contract=off.
#include "s2r_post.h"
#include "s2r_rules.h"

#include <cstring>

namespace {

// mapped host memory the host reads behind a synchronise: coherent and portable, as every pinned buffer of s2r_host.cpp
constexpr unsigned kHostPolled = hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable;
constexpr size_t kLimState = 2u * (S2R_LIMITER_MAX_LOOKAHEAD + S2R_LIMITER_TP_HISTORY) + 2u * S2R_LIMITER_MAX_LOOKAHEAD + S2R_LIMITER_MAX_HOLD;     // the largest xh (the true-peak detector's), then the largest gh

#define POST_HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)
// a stage's launch between its timer's marks
#define POST_TIMED(c, t, call) do { if ((c).timing) POST_HIP((t).begin((c).stream)); POST_HIP(call); if ((c).timing) POST_HIP((t).end((c).stream)); } while (0)

inline uint32_t fx_pstride(const S2rPostCtx &c) { return (c.max_frames + 7u) & ~7u; }

template <class F> void drop(F &f) { f.free(); f = F{}; }
template <class... Owner> void free_all(Owner &...o) { (o.free(), ...); }

// The setters' shared sequence.  The new effect `f` is built aside — the stage's staging buffer if this is its first effect, the two
// lines, the current one +0.0 everywhere (the other is written whole by the first call), then `own(f)`: what else the effect allocates
// and sends on the stream — and waited for on the handle's stream, which waits for no other handle's kernels.  On any error it is
// freed and the bus keeps the effect it had; on success it replaces that one.
template <class F, class Own>
hipError_t replace(const S2rPostCtx &c, float *&stage, F &slot, F f, size_t line_floats, Own own) {
    hipError_t e = hipSuccess;
    if (!stage) e = hipMalloc((void **)&stage, (size_t)2 * S2R_MAX_BUSES * c.max_frames * sizeof(float));
    if (e == hipSuccess) e = f.alloc(line_floats);
    if (e == hipSuccess) e = f.zero(0, c.stream);
    if (e == hipSuccess) e = own(f);
    { const hipError_t e2 = hipStreamSynchronize(c.stream); if (e == hipSuccess) e = e2; }
    if (e != hipSuccess) { drop(f); return e; }
    drop(slot);
    slot = f;
    return hipSuccess;
}
hipError_t nothing_more(S2rBusLine &) { return hipSuccess; }

// each bus stage's part of launch, by S2rBusStage
using StageLaunch = hipError_t (S2rPostChain::*)(const S2rPostCtx &, const S2rPostCall &) const;
const StageLaunch kStageLaunch[S2R_BUS_STAGES] = {&S2rPostChain::launch_eq,     &S2rPostChain::launch_dyn,   &S2rPostChain::launch_drive,  &S2rPostChain::launch_flanger,
                                                  &S2rPostChain::launch_chorus, &S2rPostChain::launch_delay, &S2rPostChain::launch_reverb, &S2rPostChain::launch_room};
// ... and each master stage's, by S2rMasterStage
const StageLaunch kMasterLaunch[S2R_MASTER_STAGES] = {&S2rPostChain::launch_master,   &S2rPostChain::launch_multiband, &S2rPostChain::launch_limiter, &S2rPostChain::launch_loudness,
                                                      &S2rPostChain::launch_spectrum, &S2rPostChain::launch_resampler, &S2rPostChain::launch_pcm};

}  // namespace

hipError_t S2rDevBuf::reserve(size_t n) {
    if (n <= floats) return hipSuccess;
    free();
    POST_HIP(hipMalloc((void **)&dev, n * sizeof(float)));
    floats = n;
    return hipSuccess;
}

hipError_t S2rDevTable::send(const std::vector<float> &host, size_t at, hipStream_t stream) const {
    if (valid) return hipSuccess;
    return hipMemcpyAsync(dev + at, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, stream);
}

template <class T> hipError_t S2rPinned<T>::reserve(size_t n) {
    if (n > count) free();
    if (!host) { POST_HIP(hipHostMalloc((void **)&host, n * sizeof(T), kHostPolled)); count = n; }
    if (!dev) POST_HIP(hipHostGetDevicePointer((void **)&dev, host, 0));
    return hipSuccess;
}

hipError_t S2rBusLine::alloc(size_t n) {
    floats = n;
    for (float *&p : line) POST_HIP(hipMalloc((void **)&p, n * sizeof(float)));
    return hipSuccess;
}

hipError_t S2rBusLine::copy(float *get, const float *set, size_t at, size_t n, hipStream_t stream) const {
    if (get) return hipMemcpyAsync(get, now() + at, n * sizeof(float), hipMemcpyDeviceToHost, stream);
    return hipMemcpyAsync(now() + at, set, n * sizeof(float), hipMemcpyHostToDevice, stream);
}

hipError_t S2rMirror::reserve(size_t n) {
    if (n > floats) { free(); floats = n; }                      // (only behind a set: the state is the host's then, and the device's copies hold nothing)
    for (float *&p : dev) if (!p) POST_HIP(hipMalloc((void **)&p, floats * sizeof(float)));
    return hipSuccess;
}

hipError_t S2rMirror::upload(hipStream_t stream) const {
    if (!host_valid) return hipSuccess;
    return hipMemcpyAsync(now(), host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, stream);
}

hipError_t S2rMirror::fetch(hipStream_t stream) {
    std::vector<float> st(host.size());
    POST_HIP(hipMemcpyAsync(st.data(), now(), st.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
    POST_HIP(hipStreamSynchronize(stream));
    host.swap(st);
    host_valid = true;
    return hipSuccess;
}

hipError_t S2rPostTimer::begin(hipStream_t stream) {
    for (hipEvent_t &e : ev) if (!e) POST_HIP(hipEventCreate(&e));
    return hipEventRecord(ev[0], stream);
}

hipError_t S2rPostChain::prepare(const S2rPostCtx &c, uint32_t n_buses, uint32_t frames, bool master_fill, bool stems, S2rPostCall &call) {
    call = S2rPostCall{};
    call.n_buses = n_buses; call.frames = frames; call.master = master_fill; call.stems = stems;
    for (int k = 0; k < S2R_BUS_STAGES; k++)
        for (uint32_t b = 0; b < n_buses; b++) if (runs(k, b, n_buses)) call.on[k] = true;
    const uint32_t set[S2R_MASTER_STAGES] = {1u, mb.n_bands, limiter.lookahead, loud.hop, spec.n_fft, res.L, pcm.bits};      // 0: the stage is off
    bool *const run = call.run;
    for (int k = 0; k < S2R_MASTER_STAGES; k++) run[k] = master_fill && set[k] != 0;
    if (run[S2R_MASTER_RESAMPLER]) res.call_count = (uint32_t)resampler_count(res.L, res.M, res.ph, frames);
    call.pcm_idle = run[S2R_MASTER_PCM] && run[S2R_MASTER_RESAMPLER] && res.call_count == 0;    // the PCM kernel runs behind the resampler only when that makes a frame
    run[S2R_MASTER_PCM] = run[S2R_MASTER_PCM] && !call.pcm_idle;
    const size_t lr = (size_t)2 * c.max_frames;                  // the master's two channels, or one bus's
    const auto blocks = [&](uint32_t block) { return (size_t)((c.max_frames + block - 1u) / block); };
    if (run[S2R_MASTER_MIX]) {                                   // the device copy of the stems and the pinned rows of block partials
        POST_HIP(master.stage.reserve(S2R_MAX_BUSES * lr));
        POST_HIP(master.partials.reserve(blocks(S2R_METER_BLOCK) * S2R_MASTER_ROW));
    }
    if (run[S2R_MASTER_LIMITER]) {                               // the limiter's input, the two copies of its state, its pinned rows of meter partials
        POST_HIP(limiter.in.reserve(lr));
        POST_HIP(limiter.state.reserve(kLimState));
        POST_HIP(limiter.partials.reserve(blocks(S2R_LIMITER_BLOCK) * 2u));
    }
    if (run[S2R_MASTER_MULTIBAND]) {                             // its input, the tables, the two copies of its state, its pinned meter row
        POST_HIP(mb.in.reserve(lr));
        POST_HIP(mb.curves_dev.reserve((size_t)S2R_MULTIBAND_MAX_BANDS * S2R_DYN_CURVE_POINTS));
        POST_HIP(mb.state.reserve(S2R_MULTIBAND_STATE(S2R_MULTIBAND_MAX_BANDS)));
        POST_HIP(mb.meter.reserve(S2R_MULTIBAND_MAX_BANDS));
    }
    const bool pcm_set = run[S2R_MASTER_PCM] || call.pcm_idle;
    if (run[S2R_MASTER_LOUDNESS] || run[S2R_MASTER_SPECTRUM] || run[S2R_MASTER_RESAMPLER] || pcm_set) POST_HIP(loud.in.reserve(lr));       // the tail's input
    if (run[S2R_MASTER_SPECTRUM]) {                              // the two copies of the state, the tables and the pinned rows, by n_fft and hop
        POST_HIP(spec.state.reserve(S2R_SPECTRUM_STATE(spec.n_fft)));
        POST_HIP(spec.tables.reserve(2u * (size_t)spec.n_fft));
        POST_HIP(spec.rows.reserve((size_t)(c.max_frames / spec.hop + 1u) * spec.kept.width));
    }
    if (run[S2R_MASTER_LOUDNESS]) {                              // the two copies of its state, its pinned hop rows and peaks
        POST_HIP(loud.state.reserve(S2R_LOUDNESS_STATE));
        POST_HIP(loud.rows.reserve((size_t)(c.max_frames / S2R_LOUDNESS_MIN_HOP + 1u) * S2R_LOUDNESS_CHANNELS));
        POST_HIP(loud.peaks.reserve(blocks(S2R_LOUDNESS_BLOCK) * 2u));
    }
    const size_t res_cap = res.L ? (size_t)S2R_RESAMPLER_MAX_OUT(c.max_frames, res.L, res.M) : 0u;
    if (run[S2R_MASTER_RESAMPLER]) {                             // the two copies of its state, the table and the outputs, by L, M and T
        const size_t need = (size_t)S2R_RESAMPLER_PROGRAMMES * 2u * res_cap;
        POST_HIP(res.state.reserve(S2R_RESAMPLER_STATE(res.T)));
        POST_HIP(res.table_dev.reserve((size_t)res.L * res.T));
        if (res.res.grows(need)) { res.have = false; res.count = 0; }      // (a regrowth drops the last fill's outputs)
        POST_HIP(res.res.reserve(need));
        if (pcm_set) POST_HIP(res.res_dev.reserve(need));        // what the PCM kernel reads behind it
    }
    if (pcm_set) {                                               // the two copies of its state, its pinned samples and counts
        const size_t need = (size_t)S2R_PCM_PROGRAMMES * 2u * (run[S2R_MASTER_RESAMPLER] ? res_cap : c.max_frames);
        POST_HIP(pcm.state.reserve(S2R_PCM_STATE));
        if (pcm.samples.grows(need)) { pcm.have = false; pcm.frames = 0; }   // (a regrowth drops the last fill's samples)
        POST_HIP(pcm.samples.reserve(need));
        POST_HIP(pcm.counts.reserve(S2R_PCM_CHANNELS));
    }
    float *own[S2R_BUS_STAGES];
    for (int k = 0; k < S2R_BUS_STAGES; k++) own[k] = stage[k].buffer;
    call.route = s2r_post_route(call, own, master.stage.dev, mb.in.dev, limiter.in.dev, loud.in.dev, res.res_dev.dev, (size_t)2 * S2R_MAX_BUSES * res.call_count,
                                c.bus_out_dev, c.out_host_dev);
    return hipSuccess;
}

hipError_t S2rPostChain::launch(const S2rPostCtx &c, const S2rPostCall &call) {
    for (int k = 0; k < S2R_BUS_STAGES; k++)                     // each once per call, over all of its frames, every bus as the stages in front left it
        if (call.on[k]) POST_TIMED(c, stage[k].timer, (this->*kStageLaunch[k])(c, call));
    for (int k = 0; k < S2R_MASTER_STAGES; k++)                  // ... and the master stages behind them, each on what route.writer or route.reader names
        if (call.run[k]) POST_TIMED(c, master_timer[k], (this->*kMasterLaunch[k])(c, call));
    return hipSuccess;
}

hipError_t S2rPostChain::launch_master(const S2rPostCtx &c, const S2rPostCall &call) const {    // returns, master fader and the meters' block partials
    const float fn = (float)call.frames;
    S2rMaster m{};
    m.stage = call.route.writer[S2R_MASTER_MIX].in; m.out = call.route.writer[S2R_MASTER_MIX].out; m.stems = call.route.master_stems; m.partials = master.partials.dev;
    m.n_buses = call.n_buses; m.frames = call.frames;
    for (uint32_t b = 0; b < call.n_buses; b++) {
        const float d = master.ret[b] - master.ret_app[b];       // (+0.0 for a pair that did not move, and so is its step)
        m.r0[b] = master.ret_app[b]; m.dr[b] = d / fn;
    }
    const float d = master.fader - master.fader_app;
    m.m0 = master.fader_app; m.dm = d / fn;
    return s2r_launch_master(m, c.stream);
}

hipError_t S2rPostChain::launch_multiband(const S2rPostCtx &c, const S2rPostCall &call) const {
    const Multiband &f = mb;
    POST_HIP(f.curves_dev.send(f.curves, 0, c.stream));          // (not valid until the commit)
    POST_HIP(f.state.upload(c.stream));
    const S2rMultibandGraph g = multiband_graph(f.n_bands);
    S2rMultiband a{};
    a.in = call.route.writer[S2R_MASTER_MULTIBAND].in; a.out = call.route.writer[S2R_MASTER_MULTIBAND].out;
    a.state = f.state.now(); a.next = f.state.next(); a.curves = f.curves_dev.dev; a.meter = f.meter.dev;
    for (uint32_t i = 0; i < g.n; i++) {
        const float *q = g.kind[i] == 0u ? f.lp[g.row[i]] : (g.kind[i] == 1u ? f.hp[g.row[i]] : f.ap[g.row[i]]);
        std::memcpy(a.c[i], q, sizeof a.c[i]);
        a.src[i] = g.src[i]; a.depth[i] = g.depth[i];
    }
    for (uint32_t j = 0; j < f.n_bands; j++) { a.leaf[j] = g.leaf[j]; a.a_att[j] = f.a_att[j]; a.a_rel[j] = f.a_rel[j]; }
    a.n_bands = f.n_bands; a.n_sections = g.n; a.frames = call.frames;
    return s2r_launch_multiband(a, c.stream);
}

hipError_t S2rPostChain::launch_limiter(const S2rPostCtx &c, const S2rPostCall &call) const {   // the next state goes into the copy that is not the current one
    const Limiter &lm = limiter;
    float *cur = lm.state.now(), *next = lm.state.next();
    POST_HIP(lm.state.upload(c.stream));                         // (a host copy stays valid until the commit: a failed call leaves the state where it was)
    S2rLimiter a{};
    a.x = call.route.writer[S2R_MASTER_LIMITER].in; a.out = call.route.writer[S2R_MASTER_LIMITER].out;
    a.xh = cur; a.gh = cur + lm.n_x(); a.xh_next = next; a.gh_next = next + lm.n_x();
    a.partials = lm.partials.dev; a.frames = call.frames; a.lookahead = lm.lookahead; a.hold = lm.hold; a.ceiling = lm.ceiling;
    if (lm.detector != S2R_LIMITER_TRUE_PEAK) return s2r_launch_limiter(a, c.stream);
    S2rLimiterTp t{};                                            // the same block, the interpolator's taps beside it, its own kernel
    t.l = a; std::memcpy(t.g, drive_taps().g, sizeof t.g);
    return s2r_launch_limiter_tp(t, c.stream);
}

hipError_t S2rPostChain::launch_loudness(const S2rPostCtx &c, const S2rPostCall &call) const {  // behind whoever wrote the master last
    const Loudness &ld = loud; const auto &r = call.route.reader[S2R_MASTER_LOUDNESS - S2R_MASTER_WRITERS];
    POST_HIP(ld.state.upload(c.stream));
    S2rLoudness a{};
    a.stems = r.stems; a.master = r.in; a.out = r.out; a.state = ld.state.now(); a.next = ld.state.next();
    a.rows = ld.rows.dev; a.peaks = ld.peaks.dev; a.n_buses = call.n_buses; a.frames = call.frames; a.hop = ld.hop; a.pos = ld.pos;
    std::memcpy(a.c, ld.c, sizeof a.c); std::memcpy(a.g, drive_taps().g, sizeof a.g);
    return s2r_launch_loudness(a, c.stream);
}

hipError_t S2rPostChain::launch_spectrum(const S2rPostCtx &c, const S2rPostCall &call) const {
    const Spectrum &sp = spec; const auto &r = call.route.reader[S2R_MASTER_SPECTRUM - S2R_MASTER_WRITERS];
    POST_HIP(sp.tables.send(sp.window, 0, c.stream));            // (not valid until the commit)
    POST_HIP(sp.tables.send(sp.twiddles, sp.n_fft, c.stream));
    POST_HIP(sp.state.upload(c.stream));
    S2rSpectrum a{};
    a.stems = r.stems; a.master = r.in; a.out = r.out;
    a.state = sp.state.now(); a.next = sp.state.next(); a.window = sp.tables.dev; a.twiddles = sp.tables.dev + sp.n_fft; a.rows = sp.rows.dev;
    a.n_buses = call.n_buses; a.frames = call.frames; a.n_fft = sp.n_fft; a.hop = sp.hop; a.pos = sp.pos;
    return s2r_launch_spectrum(a, c.stream);
}

hipError_t S2rPostChain::launch_resampler(const S2rPostCtx &c, const S2rPostCall &call) const {
    const Resampler &rs = res; const auto &r = call.route.reader[S2R_MASTER_RESAMPLER - S2R_MASTER_WRITERS];
    POST_HIP(rs.table_dev.send(rs.table, 0, c.stream));          // (not valid until the commit)
    POST_HIP(rs.state.upload(c.stream));
    S2rResampler a{};
    a.stems = r.stems; a.master = r.in; a.out = r.out;
    a.state = rs.state.now(); a.next = rs.state.next(); a.table = rs.table_dev.dev; a.res = rs.res.dev; a.res_dev = call.route.res_dev;
    a.n_buses = call.n_buses; a.frames = call.frames; a.L = rs.L; a.M = rs.M; a.T = rs.T; a.ph = rs.ph; a.count = rs.call_count; a.out_cap = rs.cap();
    return s2r_launch_resampler(a, c.stream);
}

hipError_t S2rPostChain::launch_pcm(const S2rPostCtx &c, const S2rPostCall &call) const {       // last of all
    const Pcm &pm = pcm; const auto &r = call.route.reader[S2R_MASTER_PCM - S2R_MASTER_WRITERS];
    POST_HIP(pm.state.upload(c.stream));
    S2rPcm a{};
    a.stems = r.stems; a.master = r.in; a.out = r.out;
    a.state = pm.state.now(); a.next = pm.state.next(); a.pcm = pm.samples.dev; a.clips = pm.counts.dev;
    std::memcpy(a.h, pm.h, sizeof a.h);
    a.n_buses = call.n_buses; a.frames = call.frames; a.pstride = pm.cap(); a.bits = pm.bits; a.dither = pm.dither; a.n_taps = pm.n_taps;
    a.seed = pm.seed; a.t = pm.t;
    if (call.run[S2R_MASTER_RESAMPLER]) { a.n_buses = S2R_MAX_BUSES; a.frames = res.call_count; }        // the resampler's output: all eight buses, then the master, `count` frames each
    return s2r_launch_pcm(a, c.stream);
}

hipError_t S2rPostChain::launch_eq(const S2rPostCtx &c, const S2rPostCall &call) const {
    S2rEq a{};
    for (uint32_t b = 0; b < call.n_buses; b++) {
        const BusEq &f = eq[b];
        if (!f.present()) continue;
        S2rEqBus &d = a.bus[b];
        d.line = f.now(); d.next = f.next(); d.n_bands = f.n_bands;
        std::memcpy(d.c, f.c, sizeof d.c);
    }
    a.in = call.route.stage[S2R_BUS_EQ].in; a.out = call.route.stage[S2R_BUS_EQ].out; a.n_buses = call.n_buses; a.frames = call.frames;
    return s2r_launch_bus_eq(a, c.stream);
}

hipError_t S2rPostChain::launch_dyn(const S2rPostCtx &c, const S2rPostCall &call) const {       // every bus and every key as the EQs left them
    S2rDyn a{};
    for (uint32_t b = 0; b < call.n_buses; b++) {
        if (!runs(S2R_BUS_DYN, b, call.n_buses)) continue;
        const BusDyn &f = dyn[b];
        S2rDynBus &d = a.bus[b];
        d.line = f.now(); d.next = f.next(); d.curve = dyn_curves.dev + (size_t)b * S2R_DYN_CURVE_POINTS;
        d.key = f.key; d.a_att = f.a_att; d.a_rel = f.a_rel;
    }
    a.in = call.route.stage[S2R_BUS_DYN].in; a.out = call.route.stage[S2R_BUS_DYN].out; a.meter = dyn_meter.dev; a.n_buses = call.n_buses; a.frames = call.frames;
    return s2r_launch_bus_dyn(a, c.stream);
}

hipError_t S2rPostChain::launch_drive(const S2rPostCtx &c, const S2rPostCall &call) const {     // tiles x buses workgroups, none waiting for another
    S2rDrive a{};
    for (uint32_t b = 0; b < call.n_buses; b++) {
        const BusDrive &f = drive[b];
        if (!f.present()) continue;
        S2rDriveBus &d = a.bus[b];
        d.curve = drive_curves.dev + (size_t)b * S2R_DRIVE_CURVE_POINTS; d.line = f.now(); d.next = f.next();
        d.pre = f.pre; d.dry = f.dry; d.wet = f.wet;
    }
    const S2rDriveTaps &taps = drive_taps();
    std::memcpy(a.h, taps.h, sizeof a.h); std::memcpy(a.g, taps.g, sizeof a.g);
    a.in = call.route.stage[S2R_BUS_DRIVE].in; a.out = call.route.stage[S2R_BUS_DRIVE].out; a.n_buses = call.n_buses; a.frames = call.frames;
    return s2r_launch_bus_drive(a, c.stream);
}

hipError_t S2rPostChain::launch_flanger(const S2rPostCtx &c, const S2rPostCall &call) const {   // a wavefront per bus, tile by tile
    S2rFlanger a{};
    for (uint32_t b = 0; b < call.n_buses; b++) {
        const BusFlanger &f = flanger[b];
        if (!f.present()) continue;
        S2rFlangerBus &d = a.bus[b];
        d.line = f.now(); d.next = f.next(); d.history = f.history;
        d.phase = f.phase; d.phase_inc = f.phase_inc; d.spread = f.spread;
        d.base = f.base; d.depth = f.depth; d.feedback = f.feedback; d.cross = f.cross; d.dry = f.dry; d.wet = f.wet;
    }
    a.in = call.route.stage[S2R_BUS_FLANGER].in; a.out = call.route.stage[S2R_BUS_FLANGER].out; a.n_buses = call.n_buses; a.frames = call.frames;
    return s2r_launch_bus_flanger(a, c.stream);
}

hipError_t S2rPostChain::launch_chorus(const S2rPostCtx &c, const S2rPostCall &call) const {
    S2rChorus a{};
    for (uint32_t b = 0; b < call.n_buses; b++) {
        const BusChorus &f = chorus[b];
        if (!f.present()) continue;
        S2rChorusBus &d = a.bus[b];
        d.line = f.now(); d.next = f.next(); d.voices = f.voices; d.history = f.history;
        d.phase = f.phase; d.phase_inc = f.phase_inc; d.spread = f.spread;
        d.base = f.base; d.depth = f.depth; d.dry = f.dry; d.wet = f.wet;
        for (uint32_t v = 0; v < f.voices; v++) d.off[v] = chorus_voice_offset(v, f.voices);
    }
    a.in = call.route.stage[S2R_BUS_CHORUS].in; a.out = call.route.stage[S2R_BUS_CHORUS].out; a.n_buses = call.n_buses; a.frames = call.frames;
    return s2r_launch_bus_chorus(a, c.stream);
}

hipError_t S2rPostChain::launch_delay(const S2rPostCtx &c, const S2rPostCall &call) const {
    S2rDelay a{};
    for (uint32_t b = 0; b < call.n_buses; b++) {
        const BusDelay &f = delay[b];
        if (!f.present()) continue;
        S2rDelayBus &d = a.bus[b];
        d.line = f.now(); d.next = f.next(); d.delay = f.history;
        d.feedback = f.feedback; d.cross = f.cross; d.dry = f.dry; d.wet = f.wet;
    }
    a.in = call.route.stage[S2R_BUS_DELAY].in; a.out = call.route.stage[S2R_BUS_DELAY].out; a.n_buses = call.n_buses; a.frames = call.frames;
    return s2r_launch_bus_delay(a, c.stream);
}

hipError_t S2rPostChain::launch_reverb(const S2rPostCtx &c, const S2rPostCall &call) const {
    S2rFx a{};
    for (uint32_t b = 0; b < call.n_buses; b++) {
        const BusFx &f = fx[b];
        if (!f.present()) continue;
        S2rFxBus &d = a.bus[b];
        d.taps = f.taps; d.line = f.now(); d.next = f.next(); d.partials = f.partials;
        d.n_taps = f.n_taps; d.n_seg = (f.n_taps + S2R_IR_SEGMENT - 1u) / S2R_IR_SEGMENT;
        d.tstride = f.tstride; d.lstride = f.lstride; d.dry = f.dry; d.wet = f.wet;
    }
    a.stage = call.route.stage[S2R_BUS_REVERB].in; a.out = call.route.stage[S2R_BUS_REVERB].out; a.n_buses = call.n_buses; a.frames = call.frames; a.pstride = fx_pstride(c);
    return s2r_launch_bus_fx(a, c.stream);
}

hipError_t S2rPostChain::launch_room(const S2rPostCtx &c, const S2rPostCall &call) const {      // the last of the bus stages
    S2rRoom a{};
    for (uint32_t b = 0; b < call.n_buses; b++) {
        const BusRoom &f = room[b];
        if (!f.present()) continue;
        S2rRoomBus &d = a.bus[b];
        d.line = f.now(); d.next = f.next(); d.work = f.work; d.floats = (uint32_t)f.floats;
        room_layout(f.cd, f.ad, f.spread, d.len, d.off);
        d.feedback = f.feedback; d.damp = f.damp; d.d1 = f.d1; d.g = f.g; d.gain = f.gain; d.dry = f.dry; d.wet = f.wet; d.cross = f.cross;
    }
    a.in = call.route.stage[S2R_BUS_ROOM].in; a.out = call.route.stage[S2R_BUS_ROOM].out; a.n_buses = call.n_buses; a.frames = call.frames; a.wstride = c.max_frames;
    return s2r_launch_bus_room(a, c.stream);
}

void S2rPostChain::commit(const S2rPostCall &call) {
    for (int k = 0; k < S2R_BUS_STAGES; k++)                     // the histories and states have moved on
        for (uint32_t b = 0; b < call.n_buses; b++) if (runs(k, b, call.n_buses)) bus(k, b).flip();
    for (uint32_t b = 0; b < call.n_buses; b++) {                // ... and what is no flip: the LFOs' phases, and the dynamics kernel's minima are the call's meters
        if (chorus[b].present()) chorus[b].phase += chorus[b].phase_inc * call.frames;
        if (flanger[b].present()) flanger[b].phase += flanger[b].phase_inc * call.frames;
        if (runs(S2R_BUS_DYN, b, call.n_buses)) dyn[b].min_gain = dyn_meter.host[b];
    }
    if (call.run[S2R_MASTER_MIX]) {                                   // the block partials in block order, and applied = target
        Master &ms = master;
        const uint32_t n_ch = (call.n_buses + 1u) * 2u, n_blocks = (call.frames + S2R_METER_BLOCK - 1u) / S2R_METER_BLOCK;
        for (uint32_t ch = 0; ch < n_ch; ch++) {
            float peak = 0.0f, energy = 0.0f;
            for (uint32_t k = 0; k < n_blocks; k++) {
                const float *row = ms.partials.host + (size_t)k * S2R_MASTER_ROW;
                peak = row[ch] > peak ? row[ch] : peak;
                energy = energy + row[S2R_MASTER_CH + ch];
            }
            ms.peak[ch] = peak; ms.energy[ch] = energy;
        }
        ms.metered = true; ms.meter_buses = call.n_buses; snap_master();
    }
    if (call.run[S2R_MASTER_MULTIBAND]) {                             // the state has moved on, and the walkers' minima are the call's meters
        Multiband &f = mb;
        f.state.committed(); f.curves_dev.committed(); f.metered = true;
        for (uint32_t j = 0; j < f.n_bands; j++) f.min_gain[j] = f.meter.host[j];
    }
    if (call.run[S2R_MASTER_LIMITER]) {                               // the state has moved on, and the workgroups' rows give the call's meters
        Limiter &lm = limiter;
        lm.state.committed();
        const uint32_t n_blocks = (call.frames + S2R_LIMITER_BLOCK - 1u) / S2R_LIMITER_BLOCK;
        float mn = lm.partials.host[0], pk = lm.partials.host[1];
        for (uint32_t k = 1; k < n_blocks; k++) {
            const float *row = lm.partials.host + (size_t)k * 2u;
            mn = row[0] < mn ? row[0] : mn;
            pk = row[1] > pk ? row[1] : pk;
        }
        lm.min_gain = mn; lm.out_peak = pk; lm.metered = true;
    }
    if (call.run[S2R_MASTER_SPECTRUM]) {                              // the state has moved on, and the call's rows join the rows kept
        Spectrum &sp = spec;
        sp.state.committed(); sp.tables.committed();
        sp.kept.take(sp.rows.host, sp.pos, call.frames, sp.hop);
    }
    if (call.run[S2R_MASTER_PCM]) {                                   // the state and t have moved on; the call's clips join the held ones
        Pcm &pm = pcm;
        const uint32_t made = call.run[S2R_MASTER_RESAMPLER] ? res.call_count : call.frames;
        pm.state.committed(); pm.t += made; pm.frames = made; pm.have = true;
        for (uint32_t q = 0; q < S2R_PCM_CHANNELS; q++) {
            pm.clips_last[q] = pm.counts.host[q];
            pm.clips_held[q] = pm.clips_held[q] + pm.counts.host[q] < pm.clips_held[q] ? UINT32_MAX : pm.clips_held[q] + pm.counts.host[q];
        }
    } else if (call.pcm_idle) {                                  // the resampler made no frame: no kernel ran, state, t and the held clips stay
        Pcm &pm = pcm;
        pm.frames = 0; pm.have = true;
        for (uint32_t q = 0; q < S2R_PCM_CHANNELS; q++) pm.clips_last[q] = 0u;
    }
    if (call.run[S2R_MASTER_RESAMPLER]) {                             // the state and ph have moved on
        Resampler &rs = res;
        rs.state.committed(); rs.table_dev.committed();
        rs.ph = (uint32_t)((uint64_t)rs.ph + (uint64_t)rs.call_count * rs.M - (uint64_t)call.frames * rs.L);
        rs.count = rs.call_count; rs.have = true;
    }
    if (call.run[S2R_MASTER_LOUDNESS]) {                              // the state has moved on; the call's hops join the rows, its peaks the held ones
        Loudness &ld = loud;
        ld.state.committed();
        ld.kept.take(ld.rows.host, ld.pos, call.frames, ld.hop);
        const uint32_t n_blocks = (call.frames + S2R_LOUDNESS_BLOCK - 1u) / S2R_LOUDNESS_BLOCK;
        for (uint32_t ch = 0; ch < 2u; ch++) {
            float pk = ld.peaks.host[ch];
            for (uint32_t k = 1; k < n_blocks; k++) pk = ld.peaks.host[(size_t)k * 2u + ch] > pk ? ld.peaks.host[(size_t)k * 2u + ch] : pk;
            ld.tp_last[ch] = pk;
            ld.tp_held[ch] = pk > ld.tp_held[ch] ? pk : ld.tp_held[ch];
        }
    }
}

// a stage that the fill could have run and did not reads 0; a panned fill leaves all fifteen values alone, a bus fill the master stages' seven
hipError_t S2rPostChain::read_timers(const S2rPostCall &call) {
    if (call.n_buses) for (int k = 0; k < S2R_BUS_STAGES; k++) { stage[k].timer.ms = 0.0f; if (call.on[k]) POST_HIP(stage[k].timer.read()); }
    if (call.master) for (int k = 0; k < S2R_MASTER_STAGES; k++) { master_timer[k].ms = 0.0f; if (call.run[k]) POST_HIP(master_timer[k].read()); }
    return hipSuccess;
}

void S2rPostChain::release() {
    for (uint32_t b = 0; b < S2R_MAX_BUSES; b++) { drop(eq[b]); drop(dyn[b]); drop(drive[b]); drop(flanger[b]); drop(chorus[b]); drop(delay[b]); drop(fx[b]); drop(room[b]); }
    for (Stem &st : stage) { if (st.buffer) (void)hipFree(st.buffer); st.timer.destroy(); }
    free_all(dyn_curves, dyn_meter, drive_curves);               // ... and what is neither a line nor a stage's buffer, stage by stage
    free_all(master.stage, master.partials);
    free_all(mb.state, mb.in, mb.curves_dev, mb.meter);
    free_all(limiter.state, limiter.in, limiter.partials);
    free_all(loud.state, loud.in, loud.rows, loud.peaks);
    free_all(spec.state, spec.tables, spec.rows);
    free_all(res.state, res.table_dev, res.res, res.res_dev);
    free_all(pcm.state, pcm.samples, pcm.counts);
    for (S2rPostTimer &t : master_timer) t.destroy();
}



hipError_t S2rPostChain::set_eq(const S2rPostCtx &c, uint32_t bus, uint32_t n_bands, const float *coeffs) {
    if (n_bands == 0) { drop(eq[bus]); return hipSuccess; }
    BusEq f;
    f.n_bands = n_bands; f.history = 2u * n_bands;
    std::memcpy(f.c, coeffs, (size_t)n_bands * 5u * sizeof(float));
    return replace(c, stage[S2R_BUS_EQ].buffer, eq[bus], f, 4u * (size_t)n_bands, nothing_more);
}

// The tables and the pinned meter row come first and once; the bus's row of the tables is written last, by a copy queued behind
// everything that can fail for want of memory, so that a refused set leaves the earlier dynamics whole.
hipError_t S2rPostChain::set_dyn(const S2rPostCtx &c, uint32_t bus, uint32_t key, const float *curve, float a_att, float a_rel, bool keep_state) {
    if (!curve) { drop(dyn[bus]); return hipSuccess; }
    if (keep_state) {
        BusDyn &d = dyn[bus];
        POST_HIP(hipMemcpyAsync(dyn_curves.dev + (size_t)bus * S2R_DYN_CURVE_POINTS, curve, S2R_DYN_CURVE_POINTS * sizeof(float), hipMemcpyHostToDevice, c.stream));
        POST_HIP(hipStreamSynchronize(c.stream));
        d.key = key; d.a_att = a_att; d.a_rel = a_rel;
        d.curve.assign(curve, curve + S2R_DYN_CURVE_POINTS);
        return hipSuccess;
    }
    POST_HIP(dyn_curves.reserve((size_t)S2R_MAX_BUSES * S2R_DYN_CURVE_POINTS));
    POST_HIP(dyn_meter.reserve(S2R_MAX_BUSES));
    BusDyn f;
    f.key = key; f.a_att = a_att; f.a_rel = a_rel; f.history = 1u;
    f.curve.assign(curve, curve + S2R_DYN_CURVE_POINTS);
    float *const to = dyn_curves.dev + (size_t)bus * S2R_DYN_CURVE_POINTS;
    return replace(c, stage[S2R_BUS_DYN].buffer, dyn[bus], f, 1u, [&](BusDyn &n) {          // y = curve[0], the gain at silence
        POST_HIP(hipMemcpyAsync(n.line[0], n.curve.data(), sizeof(float), hipMemcpyHostToDevice, c.stream));
        return hipMemcpyAsync(to, n.curve.data(), S2R_DYN_CURVE_POINTS * sizeof(float), hipMemcpyHostToDevice, c.stream);
    });
}

// As set_dyn: the tables come first and once, the bus's row of them is written last, behind everything that can fail for want of
// memory, so that a refused set leaves the earlier drive whole.  The history starts as +0.0 (replace).
hipError_t S2rPostChain::set_drive(const S2rPostCtx &c, uint32_t bus, const float *curve, float pre, float dry, float wet, bool keep_state) {
    if (pre < 0.0f) { drop(drive[bus]); return hipSuccess; }
    constexpr size_t kRow = S2R_DRIVE_CURVE_POINTS;
    if (keep_state) {
        BusDrive &d = drive[bus];
        if (curve) {
            POST_HIP(hipMemcpyAsync(drive_curves.dev + bus * kRow, curve, kRow * sizeof(float), hipMemcpyHostToDevice, c.stream));
            POST_HIP(hipStreamSynchronize(c.stream));
            d.curve.assign(curve, curve + kRow);
        }
        d.pre = pre; d.dry = dry; d.wet = wet;
        return hipSuccess;
    }
    POST_HIP(drive_curves.reserve((size_t)S2R_MAX_BUSES * kRow));
    BusDrive f;
    f.pre = pre; f.dry = dry; f.wet = wet; f.history = S2R_DRIVE_HISTORY;
    f.curve.assign(curve, curve + kRow);
    float *const to = drive_curves.dev + bus * kRow;
    return replace(c, stage[S2R_BUS_DRIVE].buffer, drive[bus], f, 2u * (size_t)S2R_DRIVE_HISTORY, [&](BusDrive &n) {
        return hipMemcpyAsync(to, n.curve.data(), kRow * sizeof(float), hipMemcpyHostToDevice, c.stream);
    });
}

// the line starts as +0.0 and the phase as 0 (replace); the other copy is written whole by the first call
hipError_t S2rPostChain::set_flanger(const S2rPostCtx &c, uint32_t bus, float base, float depth, uint32_t phase_inc, uint32_t spread, float feedback, float cross,
                                     float dry, float wet) {
    if (base < 0.0f) { drop(flanger[bus]); return hipSuccess; }
    BusFlanger f;
    f.history = flanger_history(base, depth); f.base = base; f.depth = depth; f.feedback = feedback; f.cross = cross; f.dry = dry; f.wet = wet;
    f.phase_inc = phase_inc; f.spread = spread;
    return replace(c, stage[S2R_BUS_FLANGER].buffer, flanger[bus], f, 2u * (size_t)f.history, nothing_more);
}

hipError_t S2rPostChain::set_chorus(const S2rPostCtx &c, uint32_t bus, uint32_t voices, float base, float depth, uint32_t phase_inc, uint32_t spread, float dry,
                                    float wet) {
    if (voices == 0) { drop(chorus[bus]); return hipSuccess; }
    BusChorus f;
    f.voices = voices; f.history = chorus_history(base, depth); f.base = base; f.depth = depth; f.dry = dry; f.wet = wet;
    f.phase_inc = phase_inc; f.spread = spread;
    return replace(c, stage[S2R_BUS_CHORUS].buffer, chorus[bus], f, 2u * (size_t)f.history, nothing_more);
}

hipError_t S2rPostChain::set_delay(const S2rPostCtx &c, uint32_t bus, uint32_t delay_frames, float feedback, float cross, float dry, float wet) {
    if (delay_frames == 0) { drop(delay[bus]); return hipSuccess; }
    BusDelay f;
    f.history = delay_frames; f.feedback = feedback; f.cross = cross; f.dry = dry; f.wet = wet;
    return replace(c, stage[S2R_BUS_DELAY].buffer, delay[bus], f, 2u * (size_t)delay_frames, nothing_more);
}

hipError_t S2rPostChain::set_reverb(const S2rPostCtx &c, uint32_t bus, const float *ir_l, const float *ir_r, uint32_t n_taps, float dry, float wet) {
    if (n_taps == 0) { drop(fx[bus]); return hipSuccess; }
    BusFx f;
    const uint32_t n_seg = (n_taps + S2R_IR_SEGMENT - 1u) / S2R_IR_SEGMENT;
    f.n_taps = n_taps; f.history = n_taps - 1u; f.dry = dry; f.wet = wet;
    f.tstride = n_seg * S2R_IR_SEGMENT;
    f.lstride = (n_taps - 1u + c.max_frames + 3u) & ~3u;
    std::vector<float> padded(2u * (size_t)f.tstride, 0.0f);
    std::memcpy(padded.data(), ir_l, (size_t)n_taps * sizeof(float));
    std::memcpy(padded.data() + f.tstride, ir_r, (size_t)n_taps * sizeof(float));
    return replace(c, stage[S2R_BUS_REVERB].buffer, fx[bus], f, 2u * (size_t)f.lstride, [&](BusFx &n) {      // the padded taps, the partials, and both lines +0.0
        POST_HIP(hipMalloc((void **)&n.taps, padded.size() * sizeof(float)));
        POST_HIP(hipMalloc((void **)&n.partials, (size_t)2 * n_seg * fx_pstride(c) * sizeof(float)));
        POST_HIP(hipMemcpyAsync(n.taps, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice, c.stream));
        return n.zero(1, c.stream);
    });
}

// The work area is the room's own: allocated with its lines, so that a refused set leaves the earlier room whole.  The kernel writes a
// work row before it reads it, and writes the state's other copy whole: only the current copy needs its +0.0.
hipError_t S2rPostChain::set_room(const S2rPostCtx &c, uint32_t bus, const uint32_t *cd, const uint32_t *ad, uint32_t spread, const float levels[7]) {
    if (!cd) { drop(room[bus]); return hipSuccess; }
    BusRoom f;
    std::memcpy(f.cd, cd, sizeof f.cd); std::memcpy(f.ad, ad, sizeof f.ad); f.spread = spread;
    f.history = 0;
    const size_t floats = room_state_count(cd, ad, spread);
    const hipError_t e = replace(c, stage[S2R_BUS_ROOM].buffer, room[bus], f, floats, [&](BusRoom &n) {
        return hipMalloc((void **)&n.work, (size_t)S2R_ROOM_LINES * c.max_frames * sizeof(float));
    });
    if (e == hipSuccess) set_room_params(bus, levels);
    return e;
}

void S2rPostChain::set_room_params(uint32_t bus, const float levels[7]) {
    BusRoom &f = room[bus];
    f.feedback = levels[0]; f.damp = levels[1]; f.g = levels[2]; f.gain = levels[3]; f.dry = levels[4]; f.wet = levels[5]; f.cross = levels[6];
    volatile float d1 = 1.0f - f.damp;                           // rounded to binary32, once
    f.d1 = d1;
}

hipError_t S2rPostChain::state(const S2rPostCtx &c, int k, uint32_t bus, float *get, const float *set) {
    const S2rBusLine &f = this->bus(k, bus);
    POST_HIP(f.copy(get, set, 0, f.floats, c.stream));
    return hipStreamSynchronize(c.stream);
}

// the history crosses the boundary as frames; every stage keeps it so but the reverb, which keeps it planar
hipError_t S2rPostChain::history(const S2rPostCtx &c, int k, uint32_t bus, float *get, const float *set) {
    const S2rBusLine &f = this->bus(k, bus);
    const size_t h = f.history;
    if (k != S2R_BUS_REVERB) {
        POST_HIP(f.copy(get, set, 0, 2 * h, c.stream));
        return hipStreamSynchronize(c.stream);
    }
    std::vector<float> planar(2 * h);
    if (set) for (size_t i = 0; i < h; i++) { planar[i] = set[2 * i]; planar[h + i] = set[2 * i + 1]; }
    for (int ch = 0; ch < 2; ch++) {
        float *host = planar.data() + ch * h;
        POST_HIP(f.copy(get ? host : nullptr, host, (size_t)ch * fx[bus].lstride, h, c.stream));
    }
    POST_HIP(hipStreamSynchronize(c.stream));
    if (get) for (size_t i = 0; i < h; i++) { get[2 * i] = planar[i]; get[2 * i + 1] = planar[h + i]; }
    return hipSuccess;
}

// another lookahead, hold or detector (off is a lookahead of 0: it differs) resets the state — xh +0.0, gh 1.0 —, another ceiling keeps it
void S2rPostChain::set_limiter(float ceiling, uint32_t lookahead, uint32_t hold, uint32_t detector) {
    Limiter &lm = limiter;
    const bool reset = lm.lookahead != lookahead || lm.hold != hold || lm.detector != detector;
    lm.ceiling = ceiling; lm.lookahead = lookahead; lm.hold = hold; lm.detector = detector;
    if (!lookahead) lm.state.off();
    else if (reset) {
        std::vector<float> st(lm.n_x(), 0.0f);
        st.resize(lm.n_x() + lm.n_g(), 1.0f);
        lm.state.set(st.data(), st.size());
    }
}

void S2rPostChain::set_limiter_state(const float *xh, const float *gh) {
    std::vector<float> st(xh, xh + limiter.n_x());
    st.insert(st.end(), gh, gh + limiter.n_g());
    limiter.state.set(st.data(), st.size());
}

// a set starts from the rule's initial state — the filters +0.0, y_j = curves[j][0] —; the parameters alone keep the state
void S2rPostChain::set_multiband(uint32_t n_bands, const float *lp, const float *hp, const float *ap, const float *curves, const float *a_att, const float *a_rel,
                                 bool keep_state) {
    Multiband &f = mb;
    f.curves_dev.valid = false;
    if (!n_bands) { f.n_bands = 0; f.curves.clear(); f.state.off(); f.metered = false; return; }
    f.n_bands = n_bands;
    if (n_bands >= 2u) { std::memcpy(f.lp, lp, (size_t)(n_bands - 1u) * 5u * sizeof(float)); std::memcpy(f.hp, hp, (size_t)(n_bands - 1u) * 5u * sizeof(float)); }
    if (n_bands >= 3u) std::memcpy(f.ap, ap, (size_t)(n_bands - 2u) * 5u * sizeof(float));
    std::memcpy(f.a_att, a_att, n_bands * sizeof(float)); std::memcpy(f.a_rel, a_rel, n_bands * sizeof(float));
    f.curves.assign(curves, curves + (size_t)n_bands * S2R_DYN_CURVE_POINTS);
    if (!keep_state) reset_multiband();
}

void S2rPostChain::reset_multiband() {
    Multiband &f = mb;
    const uint32_t S = S2R_MULTIBAND_SECTIONS(f.n_bands);
    std::vector<float> st(4u * (size_t)S + f.n_bands, 0.0f);
    for (uint32_t j = 0; j < f.n_bands; j++) st[4u * (size_t)S + j] = f.curves[(size_t)j * S2R_DYN_CURVE_POINTS];
    f.state.set(st.data(), st.size());
    f.metered = false;
    for (float &g : f.min_gain) g = 1.0f;
}

void S2rPostChain::set_loudness(const float *coeffs, uint32_t hop, uint32_t max_hops) {
    Loudness &ld = loud;
    if (!coeffs) { ld.hop = 0; std::memset(ld.c, 0, sizeof ld.c); }
    else { std::memcpy(ld.c, coeffs, sizeof ld.c); ld.hop = hop; }
    ld.kept.shape(S2R_LOUDNESS_CHANNELS, coeffs ? max_hops : 0u);
    reset_loudness();
    if (!coeffs) ld.state.off();
}

void S2rPostChain::reset_loudness() {
    Loudness &ld = loud;
    ld.state.zero(S2R_LOUDNESS_STATE); ld.pos = 0;
    ld.kept.clear();
    for (int ch = 0; ch < 2; ch++) ld.tp_last[ch] = ld.tp_held[ch] = 0.0f;
}

void S2rPostChain::set_spectrum(uint32_t n_fft, uint32_t hop, const float *window, uint32_t max_rows) {
    Spectrum &sp = spec;
    sp.tables.valid = false;
    if (!window) { sp.n_fft = sp.hop = 0; sp.window.clear(); sp.twiddles.clear(); }
    else {
        sp.n_fft = n_fft; sp.hop = hop;
        sp.window.assign(window, window + n_fft);
        sp.twiddles.assign(n_fft, 0.0f);
        (void)s2r_spectrum_twiddles(n_fft, sp.twiddles.data());
    }
    sp.kept.shape(window ? S2R_SPECTRUM_ROW(n_fft) : 0u, window ? max_rows : 0u);
    reset_spectrum();
    if (!window) sp.state.off();
}

void S2rPostChain::reset_spectrum() {
    Spectrum &sp = spec;
    sp.state.zero(S2R_SPECTRUM_STATE(sp.n_fft)); sp.pos = 0;
    sp.kept.clear();
}

void S2rPostChain::set_pcm(uint32_t bits, uint32_t dither, const float *taps, uint32_t n_taps, uint32_t seed) {
    Pcm &pm = pcm;
    pm.bits = bits; pm.dither = dither; pm.n_taps = bits ? n_taps : 0u; pm.seed = seed;
    for (uint32_t k = 0; k < S2R_PCM_MAX_TAPS; k++) pm.h[k] = k < pm.n_taps ? taps[k] : 0.0f;
    reset_pcm();
    if (!bits) pm.state.off();
}

void S2rPostChain::reset_pcm() {
    Pcm &pm = pcm;
    pm.state.zero(S2R_PCM_STATE); pm.t = 0; pm.frames = 0; pm.have = false;
    for (uint32_t q = 0; q < S2R_PCM_CHANNELS; q++) pm.clips_last[q] = pm.clips_held[q] = 0u;
}

void S2rPostChain::set_pcm_state(const float *state, uint32_t t) {
    Pcm &pm = pcm;
    float st[S2R_PCM_STATE];
    for (uint32_t i = 0; i < S2R_PCM_STATE; i++) st[i] = i % S2R_PCM_MAX_TAPS < pm.n_taps ? state[i] : 0.0f;
    pm.state.set(st, S2R_PCM_STATE);
    pm.t = t;
}

void S2rPostChain::set_resampler(uint32_t L, uint32_t M, uint32_t T, const float *table) {
    Resampler &rs = res;
    rs.L = table ? L : 0u; rs.M = table ? M : 0u; rs.T = table ? T : 0u;
    if (table) rs.table.assign(table, table + (size_t)L * T);
    else rs.table.clear();
    rs.table_dev.valid = false;
    if (table) reset_resampler();
    else { rs.state.off(); rs.ph = 0; rs.have = false; rs.count = 0; }
}

void S2rPostChain::reset_resampler() {
    Resampler &rs = res;
    rs.state.zero(S2R_RESAMPLER_STATE(rs.T)); rs.ph = 0; rs.have = false; rs.count = 0;
}

void S2rPostChain::set_resampler_state(const float *state, uint32_t ph) {
    res.state.set(state, S2R_RESAMPLER_STATE(res.T));
    res.ph = ph;
}
