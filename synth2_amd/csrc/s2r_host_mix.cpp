// s2r_host_mix.cpp — the panned, bus and master fills of libs2r (s2r_fill_panned, s2r_fill_buses, s2r_fill_master) and the entries of
// the voice mixer in front of them: program pan, mix, send and fader, the per-voice get / set pairs.  The bookkeeping is S2rMixerKeep's
// (s2r_mixer_keep.h), the device side S2rVoiceMixer's (s2r_mixer.h); what is left here touches the handle (s2r_handle.h): the split of
// a fill at its event frames, and the device read that seeds the voices' programs.  Compiled with hipcc, -ffp-contract=off.
#include "s2r_handle.h"

#include <cstring>
#include <utility>
#include <vector>

#include "s2r_rules.h"

using namespace s2r_host;

namespace {

// Frames [at, at + n) of a panned fill (n_buses == 0) or of a bus fill of `total` frames, the events of frame `at` already folded
// into `pending`: slice after slice the MODE 1 launch into the rows buffer and the mixdown into the mapped output.  `last_event`:
// the frame the pool's clock has already been moved to by the fill's events (fill_time at entry) — the slices from there on move
// it further.
// `ramp`: a bus fill under moving faders — the ramped mixdown, told where in the CALL each slice begins.  `bus_dst`: the route's combine_out.
int pan_segment(s2r_synth *s, uint32_t at, uint32_t n, uint32_t last_event, uint32_t sample_rate, uint32_t n_buses, uint32_t total, bool ramp,
                float *bus_dst) {
    const S2rMixCtx mc = mix_ctx(s);
    S2rVoiceMixer &dev = s->mixer_dev;
    S2R_HIP(s, n_buses ? dev.send_bus_gains(mc, s->mixer, ramp, total) : dev.send_pan_gains(mc, s->mixer));
    for (uint32_t done = 0; done < n;) {
        const uint32_t len = n - done < dev.slice() ? n - done : dev.slice();
        s->fill_time = at + done >= last_event ? 0u : len;       // enqueue_fill moves the clock by len - fill_time
        S2R_TRY(render_rows(s, len, sample_rate, dev.rows()));
        S2R_HIP(s, dev.mix_slice(mc, (s->mixer.used & kMixSend) != 0, at + done, len, n_buses, total, ramp, bus_dst));
        done += len;
    }
    return S2R_OK;
}

// The first call that takes attribute `bit` off its default: its arrays, and from here on the note_on paths record it.
int mixer_begin(s2r_synth *s, uint32_t bit) {
    S2rMixerKeep &m = s->mixer;
    if (m.used & bit) return S2R_OK;
    if (bit == kMixSend) S2R_HIP(s, s->mixer_dev.sends_begin(mix_ctx(s)));
    if (bit != kMixFader) { m.begin(bit); return S2R_OK; }
    // The host mirrors every shard voice's program from now on.  What the voices hold NOW is on the device (the render
    // kernels keep it); on top of it come the events the host still holds for the next fill, in their order — the timed
    // ones as records of their own (S2rMixerKeep::begin_faders).
    S2R_QUIESCE(s);
    S2R_HIP(s, hipSetDevice(s->device));
    std::vector<uint32_t> h(s->padded_voices);
    S2R_HIP(s, hipMemcpyAsync(h.data(), s->v.program, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    S2R_HIP(s, hipStreamSynchronize(s->stream));
    std::vector<uint8_t> program(s->shard_voices);
    std::vector<S2rMixerKeep::Record> waiting;
    for (uint32_t i = 0; i < s->shard_voices; i++) program[i] = (uint8_t)h[i];
    for (const S2rVoiceEvent &e : s->pending) if (e.flags & S2R_EV_RESTART) program[e.voice] = (uint8_t)(e.flags >> S2R_EV_PROGRAM_SHIFT);
    for (const S2rTimedEvent &te : s->tpending) {
        if (!(te.flags & S2R_EV_RESTART)) continue;
        if (te.frame == 0) program[te.voice] = (uint8_t)te.program;
        else waiting.push_back(S2rMixerKeep::Record{te.voice, te.frame, kMixFader, 0.0f, 0.0f, 0.0f, 0u, 0u, (uint8_t)te.program});
    }
    m.begin_faders(std::move(program), waiting);
    return S2R_OK;
}

// s2r_fill_panned (n_buses == 0: two channels into `out`), s2r_fill_buses (n_buses stereo buses, bus-major, `capacity` floats) and
// s2r_fill_master (`master`: the master section behind the buses, its two channels into `master_lr`; `out` — the stems — may be null)
int fill_rows_mixed(s2r_synth *s, float *out, size_t capacity, uint32_t n_buses, size_t frames, uint32_t sample_rate_hz, const char *who,
                    bool master = false, float *master_lr = nullptr) {
    if (!s) return S2R_ERR_INVALID;
    if (!s->kids.empty() || s->parent) return set_err(s, S2R_ERR_INVALID, "%s takes a single-device handle, not a device list", who);
    if (s->xg_on) return set_err(s, S2R_ERR_INVALID, "%s takes a handle without an exchange attached", who);
    S2R_TRY(check_fill(s, frames, sample_rate_hz));
    if (frames == 0) return S2R_OK;
    if (master ? !master_lr : !out) return set_err(s, S2R_ERR_INVALID, "null output buffer");
    if (n_buses && out && capacity < 2 * frames * n_buses)
        return set_err(s, S2R_ERR_INVALID, "%s: %u buses of %zu frames take %zu floats, the buffer holds %zu", who, n_buses, frames, 2 * frames * n_buses, capacity);
    if (s->ring_count) return set_err(s, S2R_ERR_INVALID, "%s with fills of s2r_fill_begin in flight: s2r_fill_end first", who);
    S2R_QUIESCE(s);
    S2R_HIP(s, hipSetDevice(s->device));
    const S2rMixCtx mc = mix_ctx(s);
    S2R_HIP(s, s->mixer_dev.prepare(mc, n_buses, out != nullptr));
    // what runs behind the mixdown in this call, its once-only allocations and who writes where (s2r_post.h)
    const S2rPostCtx pc = post_ctx(s); S2rPostCall call;
    S2R_HIP(s, s->post.prepare(pc, n_buses, (uint32_t)frames, master, out != nullptr, call));
    fold_frame0_records(s);
    s->mixer.settle(s->fill_time);
    const uint32_t last_event = s->fill_time;
    // a bus fill with a program fader away from where the last one left it ramps; whatever the device holds from
    // an earlier ramp is stale, and what this one sends is no static gain either (S2rVoiceMixer::send_bus_gains keeps which it sent)
    const bool ramp = n_buses && s->mixer.faders_moving();
    if (ramp) s->mixer.mark_bus();
    if (s->tpending.empty()) S2R_TRY(pan_segment(s, 0u, (uint32_t)frames, last_event, sample_rate_hz, n_buses, (uint32_t)frames, ramp, call.route.combine_out));
    else {
        // Events inside the fill: the per-voice rows and the event chains exclude each other in the render kernels, and an
        // event at frame f acts "exactly as if the caller had split the fill there" (s2r.h) — so the fill IS split there: the
        // records of one frame are folded like untimed ones (fold_frame0_records), what their note_ons give becomes the voices', and
        // the segment up to the next event frame is rendered.  (Records arrive in non-decreasing frame order.)
        std::vector<S2rTimedEvent> recs;
        recs.swap(s->tpending);
        for (const S2rTimedEvent &te : recs) s->tlast[te.voice] = -1;
        const std::vector<S2rMixerKeep::Record> mrecs = s->mixer.take_queued();
        size_t k = 0, km = 0;
        uint32_t at = 0;
        while (at < frames) {
            for (; k < recs.size() && recs[k].frame <= at; k++) fold_event(s, recs[k].voice, recs[k].flags, recs[k].pitch, recs[k].seed, recs[k].program);
            s->mixer.apply_through(mrecs, km, at);
            const uint32_t next = k < recs.size() && recs[k].frame < frames ? recs[k].frame : (uint32_t)frames;
            const int rc = pan_segment(s, at, next - at, last_event, sample_rate_hz, n_buses, (uint32_t)frames, ramp, call.route.combine_out);
            if (rc != S2R_OK) { s->fill_time = 0; return rc; }
            at = next;
        }
    }
    S2R_HIP(s, s->post.launch(pc, call));
    S2R_HIP(s, hipStreamSynchronize(s->stream));
    if (n_buses && (s->mixer.used & kMixFader)) s->mixer.snap_faders();      // the faders have arrived
    s->post.commit(call);                                        // ... and so has everything behind the mixdown
    if (n_buses && out) std::memcpy(out, s->mixer_dev.stems(), 2 * frames * n_buses * sizeof(float));
    if (master) std::memcpy(master_lr, s->out_host, 2 * frames * sizeof(float));
    else if (!n_buses) std::memcpy(out, s->out_host, 2 * frames * sizeof(float));
    if (s->timing) {
        S2R_HIP(s, s->mixer_dev.read_timers(n_buses));
        S2R_HIP(s, s->post.read_timers(call));
    }
    return S2R_OK;
}

// The three per-voice get / set pairs (pans; gains and buses; sends and send buses) behind their own checks of the values.  The
// handle: a single-device one (`shards_too`: nor a shard of a device list), and no null buffer (`args`).
int voices_handle(s2r_synth *s, bool args, bool shards_too, const char *what) {
    if (!s || !args) return S2R_ERR_INVALID;
    if (!s->kids.empty() || (shards_too && s->parent)) return set_err(s, S2R_ERR_INVALID, "voice %s are kept by single-device handles, not by a device list", what);
    return S2R_OK;
}
// ... out: an attribute never used answers with its default and settles nothing (values of note_ons inside a fill not rendered yet
// are not the voices' yet)
int voices_get(s2r_synth *s, uint32_t bit, float *values, uint8_t *bytes) {
    if (s->mixer.used & bit) s->mixer.settle(s->fill_time);
    s->mixer.get_voices(bit, values, bytes);
    return S2R_OK;
}
// ... and in
int voices_set(s2r_synth *s, uint32_t bit, const float *values, const uint8_t *bytes) {
    S2R_TRY(mixer_begin(s, bit));
    s->mixer.settle(s->fill_time);
    s->mixer.set_voices(bit, values, bytes);
    return S2R_OK;
}

}  // namespace

extern "C" {

// ---- true stereo ----
int s2r_set_program_pan(s2r_synth *s, uint32_t program, float pan, float key_spread) {
    // (the values first: they are wrong whatever the handle holds — and a front-end can ask without a device)
    if (!pan_in_range(pan) || !pan_in_range(key_spread))
        return set_err(s, S2R_ERR_PATCH_RANGE, "program %u: pan %g, key_spread %g: both lie in [-1, 1]", program, (double)pan, (double)key_spread);
    if (!s) return S2R_ERR_INVALID;
    if (program >= s->bank.size()) return set_err(s, S2R_ERR_INVALID, "program %u: the bank holds %zu patches", program, s->bank.size());
    if (pan != 0.0f || key_spread != 0.0f) { (void)mixer_begin(s, kMixPan); s->mixer.settle(s->fill_time); }
    s->mixer.prog[program].pan = pan; s->mixer.prog[program].spread = key_spread;
    return S2R_OK;
}

int s2r_get_program_pan(const s2r_synth *s, uint32_t program, float *pan, float *key_spread) {
    if (!s) return S2R_ERR_INVALID;
    if (program >= s->bank.size()) return S2R_ERR_INVALID;
    if (pan) *pan = s->mixer.prog[program].pan;
    if (key_spread) *key_spread = s->mixer.prog[program].spread;
    return S2R_OK;
}

int s2r_get_voice_pans(s2r_synth *s, float *pans) {
    S2R_TRY(voices_handle(s, pans != nullptr, false, "pans"));
    return voices_get(s, kMixPan, pans, nullptr);
}

int s2r_set_voice_pans(s2r_synth *s, const float *pans) {
    S2R_TRY(voices_handle(s, pans != nullptr, false, "pans"));
    for (uint32_t i = 0; i < s->shard_voices; i++)
        if (!pan_in_range(pans[i])) return set_err(s, S2R_ERR_PATCH_RANGE, "voice %u: pan %g does not lie in [-1, 1]", i, (double)pans[i]);
    return voices_set(s, kMixPan, pans, nullptr);
}

int s2r_fill_panned(s2r_synth *s, float *interleaved_lr_out, size_t frames, uint32_t sample_rate_hz) {
    return fill_rows_mixed(s, interleaved_lr_out, 0, 0u, frames, sample_rate_hz, "s2r_fill_panned");
}

// ---- the voice mixer ----
int s2r_set_program_mix(s2r_synth *s, uint32_t program, float level, float velocity_sens, uint32_t bus) {
    // (the values first, like s2r_set_program_pan)
    if (!unit_in_range(level) || !unit_in_range(velocity_sens) || bus >= S2R_MAX_BUSES)
        return set_err(s, S2R_ERR_PATCH_RANGE, "program %u: level %g, velocity_sens %g, bus %u: both values lie in [0, 1], the bus below %u", program,
                       (double)level, (double)velocity_sens, bus, S2R_MAX_BUSES);
    if (!s) return S2R_ERR_INVALID;
    if (program >= s->bank.size()) return set_err(s, S2R_ERR_INVALID, "program %u: the bank holds %zu patches", program, s->bank.size());
    if (level != 1.0f || velocity_sens != 0.0f || bus != 0u) { (void)mixer_begin(s, kMixLevel); s->mixer.settle(s->fill_time); }
    S2rProgramMix &p = s->mixer.prog[program];
    p.level = level; p.sens = velocity_sens; p.bus = (uint8_t)bus;
    return S2R_OK;
}

int s2r_get_program_mix(const s2r_synth *s, uint32_t program, float *level, float *velocity_sens, uint32_t *bus) {
    if (!s) return S2R_ERR_INVALID;
    if (program >= s->bank.size()) return S2R_ERR_INVALID;
    const S2rProgramMix &p = s->mixer.prog[program];
    if (level) *level = p.level;
    if (velocity_sens) *velocity_sens = p.sens;
    if (bus) *bus = p.bus;
    return S2R_OK;
}

int s2r_get_voice_mix(s2r_synth *s, float *gains, uint8_t *buses) {
    S2R_TRY(voices_handle(s, gains && buses, false, "mixes"));
    return voices_get(s, kMixLevel, gains, buses);
}

int s2r_set_voice_mix(s2r_synth *s, const float *gains, const uint8_t *buses) {
    S2R_TRY(voices_handle(s, gains && buses, false, "mixes"));
    for (uint32_t i = 0; i < s->shard_voices; i++)
        if (!unit_in_range(gains[i]) || buses[i] >= S2R_MAX_BUSES)
            return set_err(s, S2R_ERR_PATCH_RANGE, "voice %u: gain %g, bus %u: the gain lies in [0, 1], the bus below %u", i, (double)gains[i], (unsigned)buses[i], S2R_MAX_BUSES);
    return voices_set(s, kMixLevel, gains, buses);
}

// ---- aux sends ----
int s2r_set_program_send(s2r_synth *s, uint32_t program, float send, uint32_t send_bus) {
    // (the values first, like s2r_set_program_mix)
    if (!unit_in_range(send) || send_bus >= S2R_MAX_BUSES)
        return set_err(s, S2R_ERR_PATCH_RANGE, "program %u: send %g, send bus %u: the send lies in [0, 1], the bus below %u", program, (double)send, send_bus, S2R_MAX_BUSES);
    if (!s) return S2R_ERR_INVALID;
    if (!s->kids.empty() || s->parent) return set_err(s, S2R_ERR_INVALID, "program sends are kept by single-device handles, not by a device list");
    if (program >= s->bank.size()) return set_err(s, S2R_ERR_INVALID, "program %u: the bank holds %zu patches", program, s->bank.size());
    if (send != 0.0f || send_bus != 0u) {
        S2R_TRY(mixer_begin(s, kMixSend));
        s->mixer.settle(s->fill_time);
    }
    s->mixer.prog[program].send = send; s->mixer.prog[program].send_bus = (uint8_t)send_bus;
    return S2R_OK;
}

int s2r_get_program_send(const s2r_synth *s, uint32_t program, float *send, uint32_t *send_bus) {
    if (!s) return S2R_ERR_INVALID;
    if (!s->kids.empty() || s->parent || program >= s->bank.size()) return S2R_ERR_INVALID;
    if (send) *send = s->mixer.prog[program].send;
    if (send_bus) *send_bus = s->mixer.prog[program].send_bus;
    return S2R_OK;
}

int s2r_get_voice_sends(s2r_synth *s, float *sends, uint8_t *send_buses) {
    S2R_TRY(voices_handle(s, sends && send_buses, true, "sends"));
    return voices_get(s, kMixSend, sends, send_buses);
}

int s2r_set_voice_sends(s2r_synth *s, const float *sends, const uint8_t *send_buses) {
    S2R_TRY(voices_handle(s, sends && send_buses, true, "sends"));
    for (uint32_t i = 0; i < s->shard_voices; i++)
        if (!unit_in_range(sends[i]) || send_buses[i] >= S2R_MAX_BUSES)
            return set_err(s, S2R_ERR_PATCH_RANGE, "voice %u: send %g, send bus %u: the send lies in [0, 1], the bus below %u", i, (double)sends[i], (unsigned)send_buses[i], S2R_MAX_BUSES);
    return voices_set(s, kMixSend, sends, send_buses);
}

// ---- program faders ----
int s2r_set_program_fader(s2r_synth *s, uint32_t program, float fader, float pan_shift) {
    // (the values first, like s2r_set_program_pan)
    if (!fader_in_range(fader, pan_shift))
        return set_err(s, S2R_ERR_PATCH_RANGE, "program %u: fader %g, pan_shift %g: the fader lies in [0, 1], the shift in [-2, 2]", program, (double)fader, (double)pan_shift);
    if (!s) return S2R_ERR_INVALID;
    if (!s->kids.empty() || s->parent) return set_err(s, S2R_ERR_INVALID, "program faders are kept by single-device handles, not by a device list");
    if (program >= s->bank.size()) return set_err(s, S2R_ERR_INVALID, "program %u: the bank holds %zu patches", program, s->bank.size());
    if (fader != 1.0f || pan_shift != 0.0f) {
        S2R_REFUSE_BROKEN(s);
        S2R_TRY(mixer_begin(s, kMixFader));
    }
    s->mixer.prog[program].fader = fader; s->mixer.prog[program].shift = pan_shift;
    return S2R_OK;
}

int s2r_get_program_fader(const s2r_synth *s, uint32_t program, float *fader, float *pan_shift, float *applied_fader, float *applied_pan_shift) {
    if (!s) return S2R_ERR_INVALID;
    if (!s->kids.empty() || s->parent || program >= s->bank.size()) return S2R_ERR_INVALID;
    const S2rProgramMix &p = s->mixer.prog[program];
    if (fader) *fader = p.fader;
    if (pan_shift) *pan_shift = p.shift;
    if (applied_fader) *applied_fader = p.fader_app;
    if (applied_pan_shift) *applied_pan_shift = p.shift_app;
    return S2R_OK;
}

int s2r_snap_program_faders(s2r_synth *s) {
    if (!s) return S2R_ERR_INVALID;
    if (!s->kids.empty() || s->parent) return set_err(s, S2R_ERR_INVALID, "program faders are kept by single-device handles, not by a device list");
    s->mixer.snap_faders();
    s->mixer.mark_bus();
    return S2R_OK;
}

int s2r_fill_buses(s2r_synth *s, float *out, size_t capacity, uint32_t n_buses, size_t frames, uint32_t sample_rate_hz) {
    if (!s) return S2R_ERR_INVALID;
    if (n_buses == 0 || n_buses > S2R_MAX_BUSES) return set_err(s, S2R_ERR_INVALID, "s2r_fill_buses: %u buses (1 .. %u)", n_buses, S2R_MAX_BUSES);
    return fill_rows_mixed(s, out, capacity, n_buses, frames, sample_rate_hz, "s2r_fill_buses");
}

int s2r_fill_master(s2r_synth *s, float *master_lr, float *stems, size_t stems_capacity, uint32_t n_buses, size_t frames, uint32_t sample_rate_hz) {
    if (!s) return S2R_ERR_INVALID;
    if (n_buses == 0 || n_buses > S2R_MAX_BUSES) return set_err(s, S2R_ERR_INVALID, "s2r_fill_master: %u buses (1 .. %u)", n_buses, S2R_MAX_BUSES);
    return fill_rows_mixed(s, stems, stems_capacity, n_buses, frames, sample_rate_hz, "s2r_fill_master", true, master_lr);
}

// measurement (tools/pan_time.py): device time of the panned mixdown's kernels in the last s2r_fill_panned, summed over its
// slices, in milliseconds (s2r_set_timing on; < 0 otherwise); and the frames per slice of the rows buffer (0: not allocated yet)
float s2r_debug_pan_mix_ms(const s2r_synth *s) { return s && s->timing ? s->mixer_dev.mix_ms(false) : -1.0f; }
uint32_t s2r_debug_pan_slice(const s2r_synth *s) { return s ? s->mixer_dev.slice() : 0u; }
// ... and of the bus mixdown's kernels in the last s2r_fill_buses (tools/bus_time.py)
float s2r_debug_bus_mix_ms(const s2r_synth *s) { return s && s->timing ? s->mixer_dev.mix_ms(true) : -1.0f; }

}  // extern "C"
