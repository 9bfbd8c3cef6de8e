// s2r_post.cpp — the post-mix chain (s2r_post.h): choruses, delays, reverbs, master section, master limiter.  Compiled with hipcc, -ffp-contract=off.
#include "s2r_post.h"
#include "s2r_rules.h"

#include <cstring>

namespace {

// mapped host memory the host reads behind a synchronise: coherent and portable, as every pinned buffer of s2r_host.cpp
constexpr unsigned kHostPolled = hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable;
constexpr size_t kLimXh = 2u * S2R_LIMITER_MAX_LOOKAHEAD, kLimState = kLimXh + 2u * S2R_LIMITER_MAX_LOOKAHEAD + S2R_LIMITER_MAX_HOLD;

#define POST_HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)
// a stage's launch between its timer's marks
#define POST_TIMED(c, t, call) do { if ((c).timing) POST_HIP((t).begin((c).stream)); POST_HIP(call); if ((c).timing) POST_HIP((t).end((c).stream)); } while (0)

inline uint32_t fx_pstride(const S2rPostCtx &c) { return (c.max_frames + 7u) & ~7u; }

// pinned rows of partials, once; `host` survives a failed hipHostGetDevicePointer, and the next call goes on from there
hipError_t pinned_rows(float *&host, float *&dev, size_t floats) {
    if (dev) return hipSuccess;
    if (!host) POST_HIP(hipHostMalloc((void **)&host, floats * sizeof(float), kHostPolled));
    return hipHostGetDevicePointer((void **)&dev, host, 0);
}

}  // namespace

hipError_t S2rPostTimer::begin(hipStream_t stream) {
    for (hipEvent_t &e : ev) if (!e) POST_HIP(hipEventCreate(&e));
    return hipEventRecord(ev[0], stream);
}

S2rPostRoute s2r_post_route(const S2rPostCall &call, float *chorus_stage, float *delay_stage, float *fx_stage, float *master_stage, float *limiter_in, float *bus_out_dev,
                            float *out_host_dev) {
    S2rPostRoute r{};
    if (!call.n_buses) return r;
    float *last_stems = call.master ? master_stage : bus_out_dev;
    float *behind_delay = call.fx_on ? fx_stage : last_stems;    // where the stems go when no delay stands in front
    float *behind_chorus = call.delay_on ? delay_stage : behind_delay;   // ... and when no chorus does
    r.combine_out = call.chorus_on ? chorus_stage : behind_chorus;
    if (call.chorus_on) { r.chorus_in = chorus_stage; r.chorus_out = behind_chorus; }
    if (call.delay_on) { r.delay_in = delay_stage; r.delay_out = behind_delay; }
    if (call.fx_on) { r.fx_in = fx_stage; r.fx_out = last_stems; }
    if (call.master) { r.master_in = master_stage; r.master_out = call.limited ? limiter_in : out_host_dev; r.master_stems = call.stems ? bus_out_dev : nullptr; }
    if (call.limited) { r.limiter_in = limiter_in; r.limiter_out = out_host_dev; }
    return r;
}

hipError_t S2rPostChain::prepare(const S2rPostCtx &c, uint32_t n_buses, uint32_t frames, bool master_fill, bool stems, S2rPostCall &call) {
    call = S2rPostCall{};
    call.n_buses = n_buses; call.frames = frames; call.master = master_fill; call.stems = stems;
    for (uint32_t b = 0; b < n_buses; b++) if (chorus[b].voices) call.chorus_on = true;      // (a chorus on a bus past the call's is idle in it)
    for (uint32_t b = 0; b < n_buses; b++) if (delay[b].delay) call.delay_on = true; // (and so is a delay)
    for (uint32_t b = 0; b < n_buses; b++) if (fx[b].n_taps) call.fx_on = true;      // (and so is a reverb)
    call.limited = master_fill && limiter.lookahead != 0;
    if (call.master) {                                           // the device copy of the stems and the pinned rows of block partials
        if (!master.stage) POST_HIP(hipMalloc((void **)&master.stage, (size_t)2 * S2R_MAX_BUSES * c.max_frames * sizeof(float)));
        POST_HIP(pinned_rows(master.partials, master.partials_dev, (size_t)((c.max_frames + S2R_METER_BLOCK - 1u) / S2R_METER_BLOCK) * S2R_MASTER_ROW));
    }
    if (call.limited) {                                          // the limiter's input, the two copies of its state, its pinned rows of meter partials
        if (!limiter.in) POST_HIP(hipMalloc((void **)&limiter.in, (size_t)2 * c.max_frames * sizeof(float)));
        for (float *&p : limiter.state) if (!p) POST_HIP(hipMalloc((void **)&p, kLimState * sizeof(float)));
        POST_HIP(pinned_rows(limiter.partials, limiter.partials_dev, (size_t)((c.max_frames + S2R_LIMITER_BLOCK - 1u) / S2R_LIMITER_BLOCK) * 2u));
    }
    call.route = s2r_post_route(call, chorus_stage, delay_stage, fx_stage, master.stage, limiter.in, c.bus_out_dev, c.out_host_dev);
    return hipSuccess;
}

hipError_t S2rPostChain::launch(const S2rPostCtx &c, const S2rPostCall &call) {
    const S2rPostRoute &r = call.route; const float fn = (float)call.frames;
    if (call.chorus_on) {                                        // once per call, over all of its frames, in front of the delays
        S2rChorus a{};
        for (uint32_t b = 0; b < call.n_buses; b++) {
            const BusChorus &f = chorus[b];
            if (!f.voices) continue;
            S2rChorusBus &d = a.bus[b];
            d.line = f.line[f.cur]; d.next = f.line[f.cur ^ 1]; d.voices = f.voices; d.history = f.history;
            d.phase = f.phase; d.phase_inc = f.phase_inc; d.spread = f.spread;
            d.base = f.base; d.depth = f.depth; d.dry = f.dry; d.wet = f.wet;
            for (uint32_t v = 0; v < f.voices; v++) d.off[v] = chorus_voice_offset(v, f.voices);
        }
        a.in = r.chorus_in; a.out = r.chorus_out; a.n_buses = call.n_buses; a.frames = call.frames;
        POST_TIMED(c, chorus_timer, s2r_launch_bus_chorus(a, c.stream));
    }
    if (call.delay_on) {                                         // likewise, in front of the reverbs
        S2rDelay a{};
        for (uint32_t b = 0; b < call.n_buses; b++) {
            const BusDelay &f = delay[b];
            if (!f.delay) continue;
            S2rDelayBus &d = a.bus[b];
            d.line = f.line[f.cur]; d.next = f.line[f.cur ^ 1]; d.delay = f.delay;
            d.feedback = f.feedback; d.cross = f.cross; d.dry = f.dry; d.wet = f.wet;
        }
        a.in = r.delay_in; a.out = r.delay_out; a.n_buses = call.n_buses; a.frames = call.frames;
        POST_TIMED(c, delay_timer, s2r_launch_bus_delay(a, c.stream));
    }
    if (call.fx_on) {                                            // likewise
        S2rFx a{};
        for (uint32_t b = 0; b < call.n_buses; b++) {
            const BusFx &f = fx[b];
            if (!f.n_taps) continue;
            S2rFxBus &d = a.bus[b];
            d.taps = f.taps; d.line = f.line[f.cur]; d.next = f.line[f.cur ^ 1]; d.partials = f.partials;
            d.n_taps = f.n_taps; d.n_seg = (f.n_taps + S2R_IR_SEGMENT - 1u) / S2R_IR_SEGMENT;
            d.tstride = f.tstride; d.lstride = f.lstride; d.dry = f.dry; d.wet = f.wet;
        }
        a.stage = r.fx_in; a.out = r.fx_out; a.n_buses = call.n_buses; a.frames = call.frames; a.pstride = fx_pstride(c);
        POST_TIMED(c, fx_timer, s2r_launch_bus_fx(a, c.stream));
    }
    if (call.master) {                                           // returns, master fader and the meters' block partials
        S2rMaster m{};
        m.stage = r.master_in; m.out = r.master_out; m.stems = r.master_stems; m.partials = master.partials_dev;
        m.n_buses = call.n_buses; m.frames = call.frames;
        for (uint32_t b = 0; b < call.n_buses; b++) {
            const float d = master.ret[b] - master.ret_app[b];   // (+0.0 for a pair that did not move, and so is its step)
            m.r0[b] = master.ret_app[b]; m.dr[b] = d / fn;
        }
        const float d = master.fader - master.fader_app;
        m.m0 = master.fader_app; m.dm = d / fn;
        POST_TIMED(c, master.timer, s2r_launch_master(m, c.stream));
    }
    if (call.limited) {                                          // the next state goes into the copy that is not the current one
        Limiter &lm = limiter;
        float *cur = lm.state[lm.cur], *next = lm.state[lm.cur ^ 1];
        if (lm.host_valid) {                                     // (stays valid until the commit: a failed call leaves the state where it was)
            POST_HIP(hipMemcpyAsync(cur, lm.host.data(), lm.n_x() * sizeof(float), hipMemcpyHostToDevice, c.stream));
            POST_HIP(hipMemcpyAsync(cur + kLimXh, lm.host.data() + lm.n_x(), lm.n_g() * sizeof(float), hipMemcpyHostToDevice, c.stream));
        }
        S2rLimiter a{};
        a.x = r.limiter_in; a.out = r.limiter_out; a.xh = cur; a.gh = cur + kLimXh; a.xh_next = next; a.gh_next = next + kLimXh;
        a.partials = lm.partials_dev; a.frames = call.frames; a.lookahead = lm.lookahead; a.hold = lm.hold; a.ceiling = lm.ceiling;
        POST_TIMED(c, lm.timer, s2r_launch_limiter(a, c.stream));
    }
    return hipSuccess;
}

void S2rPostChain::commit(const S2rPostCall &call) {
    if (call.chorus_on) for (uint32_t b = 0; b < call.n_buses; b++) if (chorus[b].voices) {                   // the histories have moved on, and the phases
        chorus[b].cur ^= 1; chorus[b].phase += chorus[b].phase_inc * call.frames;
    }
    if (call.delay_on) for (uint32_t b = 0; b < call.n_buses; b++) if (delay[b].delay) delay[b].cur ^= 1;
    if (call.fx_on) for (uint32_t b = 0; b < call.n_buses; b++) if (fx[b].n_taps) fx[b].cur ^= 1;
    if (call.master) {                                           // the block partials in block order, and applied = target
        Master &ms = master;
        const uint32_t n_ch = (call.n_buses + 1u) * 2u, n_blocks = (call.frames + S2R_METER_BLOCK - 1u) / S2R_METER_BLOCK;
        for (uint32_t ch = 0; ch < n_ch; ch++) {
            float peak = 0.0f, energy = 0.0f;
            for (uint32_t k = 0; k < n_blocks; k++) {
                const float *row = ms.partials + (size_t)k * S2R_MASTER_ROW;
                peak = row[ch] > peak ? row[ch] : peak;
                energy = energy + row[S2R_MASTER_CH + ch];
            }
            ms.peak[ch] = peak; ms.energy[ch] = energy;
        }
        ms.metered = true; ms.meter_buses = call.n_buses; snap_master();
    }
    if (call.limited) {                                          // the state has moved on, and the workgroups' rows give the call's meters
        Limiter &lm = limiter;
        lm.cur ^= 1; lm.host_valid = false;
        const uint32_t n_blocks = (call.frames + S2R_LIMITER_BLOCK - 1u) / S2R_LIMITER_BLOCK;
        float mn = lm.partials[0], pk = lm.partials[1];
        for (uint32_t k = 1; k < n_blocks; k++) {
            const float *row = lm.partials + (size_t)k * 2u;
            mn = row[0] < mn ? row[0] : mn;
            pk = row[1] > pk ? row[1] : pk;
        }
        lm.min_gain = mn; lm.out_peak = pk; lm.metered = true;
    }
}

// a stage that the fill could have run and did not reads 0; a panned fill leaves all five values alone, a bus fill the master's two
hipError_t S2rPostChain::read_timers(const S2rPostCall &call) {
    if (call.n_buses) { chorus_timer.ms = 0.0f; if (call.chorus_on) POST_HIP(chorus_timer.read()); }
    if (call.n_buses) { delay_timer.ms = 0.0f; if (call.delay_on) POST_HIP(delay_timer.read()); }
    if (call.n_buses) { fx_timer.ms = 0.0f; if (call.fx_on) POST_HIP(fx_timer.read()); }
    if (call.master) {
        POST_HIP(master.timer.read());
        limiter.timer.ms = 0.0f;
        if (call.limited) POST_HIP(limiter.timer.read());
    }
    return hipSuccess;
}

void S2rPostChain::release() {
    for (BusChorus &f : chorus) f.release();
    for (BusDelay &f : delay) f.release();
    for (BusFx &f : fx) f.release();
    for (float *p : {chorus_stage, delay_stage, fx_stage, master.stage, limiter.state[0], limiter.state[1], limiter.in}) if (p) (void)hipFree(p);
    for (float *p : {master.partials, limiter.partials}) if (p) (void)hipHostFree(p);
    for (S2rPostTimer *t : {&chorus_timer, &delay_timer, &fx_timer, &master.timer, &limiter.timer}) t->destroy();
}

hipError_t S2rPostChain::set_chorus(const S2rPostCtx &c, uint32_t bus, uint32_t voices, float base, float depth, uint32_t phase_inc, uint32_t spread, float dry,
                                    float wet) {
    if (voices == 0) { chorus[bus].release(); return hipSuccess; }
    BusChorus f;
    f.voices = voices; f.history = chorus_history(base, depth); f.base = base; f.depth = depth; f.dry = dry; f.wet = wet;
    f.phase_inc = phase_inc; f.spread = spread;
    const size_t line_bytes = 2u * (size_t)f.history * sizeof(float);
    hipError_t e = hipSuccess;
    if (!chorus_stage) e = hipMalloc((void **)&chorus_stage, (size_t)2 * S2R_MAX_BUSES * c.max_frames * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&f.line[0], line_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&f.line[1], line_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(f.line[0], 0, line_bytes, c.stream);     // the history: +0.0 everywhere (the other line is written whole by the first call)
    { const hipError_t e2 = hipStreamSynchronize(c.stream); if (e == hipSuccess) e = e2; }
    if (e != hipSuccess) { f.release(); return e; }              // (the earlier chorus of the bus is kept)
    chorus[bus].release();                                       // replaces any earlier chorus of the bus
    chorus[bus] = f;
    return hipSuccess;
}

hipError_t S2rPostChain::chorus_state(const S2rPostCtx &c, uint32_t bus, float *get, const float *set) {
    const BusChorus &f = chorus[bus];
    const size_t bytes = 2u * (size_t)f.history * sizeof(float);
    if (get) POST_HIP(hipMemcpyAsync(get, f.line[f.cur], bytes, hipMemcpyDeviceToHost, c.stream));
    else POST_HIP(hipMemcpyAsync(f.line[f.cur], set, bytes, hipMemcpyHostToDevice, c.stream));
    return hipStreamSynchronize(c.stream);
}

hipError_t S2rPostChain::set_delay(const S2rPostCtx &c, uint32_t bus, uint32_t delay_frames, float feedback, float cross, float dry, float wet) {
    if (delay_frames == 0) { delay[bus].release(); return hipSuccess; }
    BusDelay f;
    f.delay = delay_frames; f.feedback = feedback; f.cross = cross; f.dry = dry; f.wet = wet;
    const size_t line_bytes = 2u * (size_t)delay_frames * sizeof(float);
    hipError_t e = hipSuccess;
    if (!delay_stage) e = hipMalloc((void **)&delay_stage, (size_t)2 * S2R_MAX_BUSES * c.max_frames * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&f.line[0], line_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&f.line[1], line_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(f.line[0], 0, line_bytes, c.stream);     // the history: +0.0 everywhere (the other line is written whole by the first call)
    { const hipError_t e2 = hipStreamSynchronize(c.stream); if (e == hipSuccess) e = e2; }
    if (e != hipSuccess) { f.release(); return e; }              // (the earlier delay of the bus is kept)
    delay[bus].release();                                        // replaces any earlier delay of the bus
    delay[bus] = f;
    return hipSuccess;
}

hipError_t S2rPostChain::delay_history(const S2rPostCtx &c, uint32_t bus, float *get, const float *set) {
    const BusDelay &f = delay[bus];
    const size_t bytes = 2u * (size_t)f.delay * sizeof(float);
    if (get) POST_HIP(hipMemcpyAsync(get, f.line[f.cur], bytes, hipMemcpyDeviceToHost, c.stream));
    else POST_HIP(hipMemcpyAsync(f.line[f.cur], set, bytes, hipMemcpyHostToDevice, c.stream));
    return hipStreamSynchronize(c.stream);
}

hipError_t S2rPostChain::set_reverb(const S2rPostCtx &c, uint32_t bus, const float *ir_l, const float *ir_r, uint32_t n_taps, float dry, float wet) {
    if (n_taps == 0) { fx[bus].release(); return hipSuccess; }
    BusFx f;
    const uint32_t n_seg = (n_taps + S2R_IR_SEGMENT - 1u) / S2R_IR_SEGMENT;
    f.n_taps = n_taps; f.dry = dry; f.wet = wet;
    f.tstride = n_seg * S2R_IR_SEGMENT;
    f.lstride = (n_taps - 1u + c.max_frames + 3u) & ~3u;
    std::vector<float> padded(2u * (size_t)f.tstride, 0.0f);
    std::memcpy(padded.data(), ir_l, (size_t)n_taps * sizeof(float));
    std::memcpy(padded.data() + f.tstride, ir_r, (size_t)n_taps * sizeof(float));
    const size_t line_bytes = 2u * (size_t)f.lstride * sizeof(float);
    hipError_t e = hipSuccess;
    if (!fx_stage) e = hipMalloc((void **)&fx_stage, (size_t)2 * S2R_MAX_BUSES * c.max_frames * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&f.taps, padded.size() * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&f.line[0], line_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&f.line[1], line_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&f.partials, (size_t)2 * n_seg * fx_pstride(c) * sizeof(float));
    // (on the handle's stream, and waited for there: nothing here waits for another handle's kernels)
    if (e == hipSuccess) e = hipMemcpyAsync(f.taps, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice, c.stream);
    if (e == hipSuccess) e = hipMemsetAsync(f.line[0], 0, line_bytes, c.stream);     // the history: +0.0 everywhere
    if (e == hipSuccess) e = hipMemsetAsync(f.line[1], 0, line_bytes, c.stream);
    { const hipError_t e2 = hipStreamSynchronize(c.stream); if (e == hipSuccess) e = e2; }
    if (e != hipSuccess) { f.release(); return e; }
    fx[bus].release();                                           // replaces any earlier reverb of the bus
    fx[bus] = f;
    return hipSuccess;
}

// the history crosses the boundary as frames; the device keeps it planar
hipError_t S2rPostChain::reverb_history(const S2rPostCtx &c, uint32_t bus, float *get, const float *set) {
    const BusFx &f = fx[bus];
    const size_t h = f.n_taps - 1u;
    std::vector<float> planar(2 * h);
    float *line = f.line[f.cur];
    if (set) for (size_t i = 0; i < h; i++) { planar[i] = set[2 * i]; planar[h + i] = set[2 * i + 1]; }
    for (int ch = 0; ch < 2; ch++) {
        float *host = planar.data() + ch * h, *dev = line + (size_t)ch * f.lstride;
        POST_HIP(hipMemcpyAsync(get ? host : dev, get ? dev : host, h * sizeof(float), get ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice, c.stream));
    }
    POST_HIP(hipStreamSynchronize(c.stream));
    if (get) for (size_t i = 0; i < h; i++) { get[2 * i] = planar[i]; get[2 * i + 1] = planar[h + i]; }
    return hipSuccess;
}

// another lookahead or hold (off is a lookahead of 0: it differs) resets the state — xh +0.0, gh 1.0 —, another ceiling keeps it
void S2rPostChain::set_limiter(float ceiling, uint32_t lookahead, uint32_t hold) {
    Limiter &lm = limiter;
    const bool reset = lm.lookahead != lookahead || lm.hold != hold;
    lm.ceiling = ceiling; lm.lookahead = lookahead; lm.hold = hold;
    if (!lookahead) { lm.host.clear(); lm.host_valid = false; }
    else if (reset) {
        lm.host.assign(lm.n_x(), 0.0f);
        lm.host.resize(lm.n_x() + lm.n_g(), 1.0f);
        lm.host_valid = true;
    }
}

void S2rPostChain::set_limiter_state(const float *xh, const float *gh) {
    limiter.host.assign(xh, xh + limiter.n_x());
    limiter.host.insert(limiter.host.end(), gh, gh + limiter.n_g());
    limiter.host_valid = true;
}

hipError_t S2rPostChain::fetch_limiter_state(const S2rPostCtx &c) {
    Limiter &lm = limiter;
    std::vector<float> st(lm.n_x() + lm.n_g());
    const float *cur = lm.state[lm.cur];
    POST_HIP(hipMemcpyAsync(st.data(), cur, lm.n_x() * sizeof(float), hipMemcpyDeviceToHost, c.stream));
    POST_HIP(hipMemcpyAsync(st.data() + lm.n_x(), cur + kLimXh, lm.n_g() * sizeof(float), hipMemcpyDeviceToHost, c.stream));
    POST_HIP(hipStreamSynchronize(c.stream));
    lm.host.swap(st);
    lm.host_valid = true;
    return hipSuccess;
}
