// mixer_keep.cpp — S2rMixerKeep (csrc/s2r_mixer_keep.h, which includes nothing of HIP) under ASan + UBSan (tests/test_rules_native.py),
// held to a naive model over seeded random walks: plain per-voice arrays that exist from the start and are updated in place — a
// note_on inside a fill when that fill is rendered — and gains recomputed voice by voice with the rule_* functions.  The walk plays
// the handle's part the way s2r_host.cpp and s2r_host_mix.cpp do: it settles where they settle, begins an attribute where they
// begin it, hands begin_faders the programs "the device" holds with the events still waiting on top, and refuses what they refuse
// (an untimed note_on behind timed ones, a checkpoint with timed events pending).  After every step it may stage both buffers, as a
// panned or bus fill would, into allocations of exactly 2 * padded_voices floats and padded_voices * kBusGainBytes bytes and compares
// BITS: every byte the layout defines, zeros past the shard in every array, the per-voice getters, and the dirty bits against the
// model's prediction — exactly kGainsAll or |= kGainsBus where the handle's code marked that before the type existed.
// Shapes: 1, 63, 64 and 65 shard voices padded to the next multiple of 64; one program and eight; walks that never use sends and
// walks that do (which moves dL, dR); ramps over 1 and 48 frames.  One scenario is written out: the first fader call behind timed
// note_ons at two frames.  Prints "mixer ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "s2r.h"
#include "s2r_mixer_keep.h"

namespace {

char what[160] = "";
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "mixer_keep.cpp:%d: %s (%s)\n", __LINE__, #cond, what); std::exit(1); } } while (0)

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return next() % n; }
    bool coin() { return next() & 1u; }
    float unit() { const uint32_t k = below(9); return k == 0 ? 0.0f : k == 8 ? 1.0f : (float)below(1025) / 1024.0f; }        // [0, 1], ends included
    float pan() { return unit() * 2.0f - 1.0f; }
};

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// what a note_on leaves for its frame: the attributes in use when it came (`mask`: the record the type made of it, 0 when it never
// heard of this note_on; `extra`: begin_faders handed it a second, program-only record later), and always its program, as the
// device keeps it
struct Waiting { uint32_t local, frame, mask; bool extra; float pan, gain, send; uint8_t bus, send_bus, program; };

struct Model {
    uint32_t n = 0, used = 0;
    std::vector<S2rProgramMix> prog;
    std::vector<float> pan, gain, send;
    std::vector<uint8_t> bus, send_bus, program;
    std::vector<Waiting> waiting;                            // note_ons inside a fill not rendered yet, in event order
    unsigned dirty = kGainsAll;
    Model(uint32_t voices, uint32_t programs) : n(voices), prog(programs), pan(voices, 0.0f), gain(voices, 1.0f), send(voices, 0.0f), bus(voices, 0), send_bus(voices, 0), program(voices, 0) {}
    void land(const Waiting &w) {
        if (w.mask & kMixPan) pan[w.local] = w.pan;
        if (w.mask & kMixLevel) { gain[w.local] = w.gain; bus[w.local] = w.bus; }
        if (w.mask & kMixSend) { send[w.local] = w.send; send_bus[w.local] = w.send_bus; }
        program[w.local] = w.program;
    }
    const S2rProgramMix &fader_of(uint32_t i) const { return prog[program[i] < prog.size() ? program[i] : 0u]; }
};

struct Walk {
    uint32_t n, pv;
    Rng rng;
    bool allow_sends;
    S2rMixerKeep keep;
    Model model;
    uint32_t fill_time = 0, current = 0;
    bool timed_pending = false;                              // a note_on at a frame > 0 waits for the next fill (the handle's tpending)
    std::vector<uint32_t> unsettled;                         // masks the type still queues from a fill ALREADY rendered (it settles lazily)
    struct Event { uint32_t local, frame; uint8_t program; };                    // the handle's pending / tpending: note_ons since the last fill rendered
    std::vector<Event> events;
    std::unique_ptr<float[]> pan_buf;                        // the device side's staging buffers, exactly as large as it makes them
    std::unique_ptr<char[]> bus_buf;
    std::vector<uint8_t> dev_program;                        // every voice's program as of the last fill rendered

    Walk(uint32_t voices, uint32_t programs, uint64_t seed) : n(voices), pv((voices + 63u) & ~63u), rng{(seed * 16u + programs) * 2654435761ull + voices}, allow_sends((seed & 1u) != 0),
                                                              model(voices, programs), pan_buf(new float[2 * (size_t)pv]), bus_buf(new char[(size_t)pv * kBusGainBytes]), dev_program(voices, 0) {
        keep.prog.resize(programs);
        keep.shape(n, pv);
        std::memset(pan_buf.get(), 0, 2 * (size_t)pv * sizeof(float));
        std::memset(bus_buf.get(), 0, (size_t)pv * kBusGainBytes);
        CHECK(keep.dirty() == kGainsAll && keep.used == 0 && keep.voices() == n && keep.padded() == pv);
    }

    // ---- the handle's part ----
    void settle() {                                          // mixer_settle: s->mixer.settle(s->fill_time)
        keep.settle(fill_time);
        if (fill_time == 0 && !unsettled.empty()) { unsettled.clear(); model.dirty = kGainsAll; }
    }
    void begin(uint32_t bit) {                               // mixer_begin
        if (keep.used & bit) return;
        if (bit == kMixSend) std::memset(bus_buf.get(), 0, (size_t)pv * kBusGainBytes);         // (S2rVoiceMixer::sends_begin)
        if (bit != kMixFader) keep.begin(bit);
        else {
            // the device holds the programs as of the last fill rendered; on top, in event order, what waits: the model's frame-0
            // note_ons have landed in model.program already, so the device's array is rebuilt here from the model's BEFORE them
            std::vector<uint8_t> programs(dev_program);
            std::vector<S2rMixerKeep::Record> records;
            for (const Event &e : events) {
                if (e.frame == 0) programs[e.local] = e.program;
                else records.push_back(S2rMixerKeep::Record{e.local, e.frame, kMixFader, 0.0f, 0.0f, 0.0f, 0u, 0u, e.program});
            }
            keep.begin_faders(std::move(programs), records);
            for (Waiting &w : model.waiting) w.extra = true;
        }
        model.used |= bit; model.dirty = kGainsAll;
    }

    void note_on(uint32_t frame, int64_t voice = -1) {
        const uint32_t local = voice < 0 ? rng.below(n) : (uint32_t)voice;
        const uint8_t note = (uint8_t)rng.below(128);
        const float velocity = rng.unit();
        if (keep.used) { settle(); keep.note_on(local, current, note, velocity, frame); }
        const S2rProgramMix &p = model.prog[current];
        Waiting w{local, frame, model.used, false, 0.0f, 0.0f, p.send, p.bus, p.send_bus, (uint8_t)current};
        if (model.used & kMixPan) w.pan = rule_voice_pan(p.pan, p.spread, note);
        if (model.used & kMixLevel) w.gain = rule_voice_gain(p.level, p.sens, velocity);
        events.push_back(Event{local, frame, (uint8_t)current});
        if (frame == 0) { model.land(w); if (model.used) model.dirty = kGainsAll; }
        else { model.waiting.push_back(w); fill_time = frame; timed_pending = true; }
    }
    // a fill has rendered everything that waited: the model's voices have it now, the type's when it next settles
    void rendered() {
        for (const Waiting &w : model.waiting) { model.land(w); if (w.mask) unsettled.push_back(w.mask); if (w.extra) unsettled.push_back(kMixFader); }
        model.waiting.clear(); events.clear();
        dev_program = model.program;
        fill_time = 0; timed_pending = false;
    }

    // ---- the comparisons ----
    void compare_voices() {
        std::vector<float> f(n); std::vector<uint8_t> b(n);
        const uint32_t bits[3] = {kMixPan, kMixLevel, kMixSend};
        for (uint32_t bit : bits) {
            if (keep.used & bit) settle();                   // (voices_get)
            keep.get_voices(bit, f.data(), bit == kMixPan ? nullptr : b.data());
            const bool on = (model.used & bit) != 0;
            for (uint32_t i = 0; i < n; i++) {
                // (with timed note_ons waiting, the model's arrays are what the type's are: neither has them yet)
                const float want = !on ? (bit == kMixLevel ? 1.0f : 0.0f) : bit == kMixPan ? model.pan[i] : bit == kMixLevel ? model.gain[i] : model.send[i];
                CHECK(same_bits(f[i], want));
                if (bit != kMixPan) CHECK(b[i] == (!on ? 0 : bit == kMixLevel ? model.bus[i] : model.send_bus[i]));
            }
        }
    }
    void compare_pan() {
        keep.stage_pan(pan_buf.get());
        for (uint32_t i = 0; i < pv; i++) {
            float l = 0.0f, r = 0.0f;
            if (i < n) rule_pan_gains((model.used & kMixPan) ? model.pan[i] : 0.0f, &l, &r);
            CHECK(same_bits(pan_buf[i], l) && same_bits(pan_buf[pv + i], r));
        }
        keep.sent(kGainsPan); model.dirty &= ~kGainsPan;
    }
    void compare_bus(bool ramp, uint32_t total) {
        char *host = bus_buf.get();
        keep.stage_bus(host, ramp, total);
        const bool sends = (model.used & kMixSend) != 0;
        const S2rBusLayout o = keep.bus_layout();
        const size_t f = (size_t)pv * sizeof(float);
        CHECK(o.gl == 0 && o.gr == f && o.bus == 2 * f && o.dl == (sends ? 2 * f + pv + f + pv : 2 * f + pv) && o.dr == o.dl + f && o.end == o.dr + f);
        CHECK(o.end <= (size_t)pv * kBusGainBytes);
        auto fl = [&](size_t off, uint32_t i) { float v; std::memcpy(&v, host + off + (size_t)i * sizeof(float), sizeof v); return v; };
        for (uint32_t i = 0; i < n; i++) {
            const float pan = (model.used & kMixPan) ? model.pan[i] : 0.0f, w = (model.used & kMixLevel) ? model.gain[i] : 1.0f;
            float g0l, g0r, g1l, g1r;
            if (!(model.used & kMixFader)) { rule_pan_gains(pan, &g0l, &g0r); g0l = g0l * w; g0r = g0r * w; g1l = g0l; g1r = g0r; }
            else {
                const S2rProgramMix &p = model.fader_of(i);
                rule_fader_gains(pan, w, p.fader_app, p.shift_app, &g0l, &g0r);
                g1l = g0l; g1r = g0r;
                if (p.moving()) rule_fader_gains(pan, w, p.fader, p.shift, &g1l, &g1r);
            }
            CHECK(same_bits(fl(o.gl, i), g0l) && same_bits(fl(o.gr, i), g0r));
            CHECK((uint8_t)host[o.bus + i] == ((model.used & kMixLevel) ? model.bus[i] : 0));
            if (sends) CHECK(same_bits(fl(o.send, i), model.send[i]) && (uint8_t)host[o.send_bus + i] == model.send_bus[i]);
            if (ramp) {
                const bool moving = (model.used & kMixFader) && model.fader_of(i).moving();
                const float dl = moving ? (g1l - g0l) / (float)total : 0.0f, dr = moving ? (g1r - g0r) / (float)total : 0.0f;
                CHECK(same_bits(fl(o.dl, i), dl) && same_bits(fl(o.dr, i), dr));
            }
        }
        // past the shard every array holds what the memset left, and so does everything behind the layout's end
        for (uint32_t i = n; i < pv; i++) {
            CHECK(bits_of(fl(o.gl, i)) == 0 && bits_of(fl(o.gr, i)) == 0 && host[o.bus + i] == 0 && bits_of(fl(o.dl, i)) == 0 && bits_of(fl(o.dr, i)) == 0);
            if (sends) CHECK(bits_of(fl(o.send, i)) == 0 && host[o.send_bus + i] == 0);
        }
        for (size_t k = o.end; k < (size_t)pv * kBusGainBytes; k++) CHECK(host[k] == 0);
        keep.sent(kGainsBus); model.dirty &= ~kGainsBus;
    }
    static uint32_t bits_of(float v) { uint32_t u; std::memcpy(&u, &v, sizeof u); return u; }

    // a panned (buses false) or bus fill of `total` frames, as fill_rows_mixed runs it: split at the frames of the note_ons that wait
    void mixed_fill(bool buses, uint32_t total) {
        settle();
        const bool ramp = buses && keep.faders_moving();
        bool model_moving = false;
        if (model.used & kMixFader) for (const S2rProgramMix &p : model.prog) model_moving = model_moving || p.moving();
        CHECK(ramp == (buses && model_moving));
        if (ramp) { keep.mark_bus(); model.dirty |= kGainsBus; }
        auto segment = [&]() {
            CHECK(keep.dirty() == model.dirty);
            // (the device side sends when its bit is dirty; the bus fill also when the last one was ramped and this one is not, or the
            // reverse — staging more often than that changes nothing the type keeps, so every segment stages)
            if (buses) compare_bus(ramp, total); else compare_pan();
        };
        if (!timed_pending) segment();
        else {
            const std::vector<S2rMixerKeep::Record> q = keep.take_queued();
            CHECK(keep.queued().empty());
            std::vector<Waiting> left;
            left.swap(model.waiting);
            size_t km = 0, k = 0;
            for (uint32_t at = 0; at < total;) {
                keep.apply_through(q, km, at);
                for (; k < left.size() && left[k].frame <= at; k++) { model.land(left[k]); if (left[k].mask || left[k].extra) model.dirty = kGainsAll; }
                segment();
                at = k < left.size() && left[k].frame < total ? left[k].frame : total;
            }
            CHECK(km == q.size() && k == left.size());
        }
        if (buses && (keep.used & kMixFader)) { keep.snap_faders(); for (S2rProgramMix &p : model.prog) { p.fader_app = p.fader; p.shift_app = p.shift; } }
        events.clear(); dev_program = model.program; fill_time = 0; timed_pending = false;
    }

    void step() {
        const uint32_t n_prog = (uint32_t)model.prog.size();
        const uint32_t program = rng.below(n_prog);
        switch (rng.below(allow_sends ? 15u : 13u)) {
        case 0: {                                            // s2r_set_program_pan
            const float pan = rng.coin() ? rng.pan() : 0.0f, spread = rng.coin() ? rng.pan() : 0.0f;
            if (pan != 0.0f || spread != 0.0f) { begin(kMixPan); settle(); }
            keep.prog[program].pan = pan; keep.prog[program].spread = spread; model.prog[program].pan = pan; model.prog[program].spread = spread;
            std::snprintf(what, sizeof what, "program pan"); break;
        }
        case 1: {                                            // s2r_set_program_mix
            const float level = rng.coin() ? rng.unit() : 1.0f, sens = rng.coin() ? rng.unit() : 0.0f; const uint8_t bus = (uint8_t)(rng.coin() ? rng.below(S2R_MAX_BUSES) : 0u);
            if (level != 1.0f || sens != 0.0f || bus != 0u) { begin(kMixLevel); settle(); }
            for (S2rProgramMix *p : {&keep.prog[program], &model.prog[program]}) { p->level = level; p->sens = sens; p->bus = bus; }
            std::snprintf(what, sizeof what, "program mix"); break;
        }
        case 2: {                                            // s2r_set_program_fader (which does not settle)
            const float fader = rng.coin() ? rng.unit() : 1.0f, shift = rng.coin() ? rng.pan() * 2.0f : 0.0f;
            if (fader != 1.0f || shift != 0.0f) begin(kMixFader);
            for (S2rProgramMix *p : {&keep.prog[program], &model.prog[program]}) { p->fader = fader; p->shift = shift; }
            std::snprintf(what, sizeof what, "program fader"); break;
        }
        case 3: case 4:                                      // a note_on at frame 0 (refused behind timed ones) or inside the next fill
            if (rng.coin() && fill_time == 0) note_on(0u);
            else note_on(fill_time + 16u * rng.below(3) + (fill_time == 0 ? 16u : 0u));
            std::snprintf(what, sizeof what, "note_on, fill_time %u", fill_time); break;
        case 5: current = program; std::snprintf(what, sizeof what, "program change"); break;
        case 6:                                              // s2r_fill: renders what waits, asks nothing of the mixer
            rendered();
            std::snprintf(what, sizeof what, "plain fill"); break;
        case 7: case 8: {                                    // s2r_fill_panned / s2r_fill_buses, split at the event frames; ramps over 1 and 48 frames
            const bool buses = rng.coin();
            const uint32_t total = fill_time ? fill_time + 16u * (1u + rng.below(2)) : (rng.coin() ? 1u : 48u);
            std::snprintf(what, sizeof what, "%s fill of %u frames, fill_time %u", buses ? "bus" : "panned", total, fill_time);
            mixed_fill(buses, total); break;
        }
        case 9:                                              // s2r_snap_program_faders
            keep.snap_faders(); keep.mark_bus();
            for (S2rProgramMix &p : model.prog) { p.fader_app = p.fader; p.shift_app = p.shift; }
            model.dirty |= kGainsBus;
            std::snprintf(what, sizeof what, "snap"); break;
        case 10: {                                           // s2r_set_patch_bank: shrink or regrow; voices may stay on a program that fell off
            const uint32_t count = n_prog == 1 ? 1u : 1u + rng.below(8);
            keep.resize_bank(count); model.prog.resize(count);
            if (model.used & kMixFader) model.dirty = kGainsAll;
            if (current >= count) current = 0;
            std::snprintf(what, sizeof what, "bank of %u", count); break;
        }
        case 11: {                                           // s2r_import_state: refused with timed events pending; pending ones belong to the old state
            if (timed_pending) break;
            events.clear();
            for (uint32_t i = 0; i < n; i++) model.program[i] = (uint8_t)rng.below(8);
            dev_program = model.program;
            if (keep.used & kMixFader) {
                keep.restore_programs([this](uint32_t i) { return model.program[i]; });
                std::vector<uint32_t> still;
                for (uint32_t m : unsettled) if (m & ~kMixFader) still.push_back(m & ~kMixFader);
                unsettled.swap(still);
                CHECK(keep.queued().size() == unsettled.size());
                model.dirty = kGainsAll;
            }
            std::snprintf(what, sizeof what, "checkpoint"); break;
        }
        case 12: case 14: {                                  // s2r_set_voice_pans / _mix / _sends
            const uint32_t bit = rng.below(allow_sends ? 3u : 2u) == 0 ? kMixPan : rng.coin() || !allow_sends ? kMixLevel : kMixSend;
            std::vector<float> f(n); std::vector<uint8_t> b(n);
            for (uint32_t i = 0; i < n; i++) { f[i] = bit == kMixPan ? rng.pan() : rng.unit(); b[i] = (uint8_t)rng.below(S2R_MAX_BUSES); }
            begin(bit); settle();
            keep.set_voices(bit, f.data(), bit == kMixPan ? nullptr : b.data());
            (bit == kMixPan ? model.pan : bit == kMixLevel ? model.gain : model.send) = f;
            if (bit != kMixPan) (bit == kMixLevel ? model.bus : model.send_bus) = b;
            model.dirty = kGainsAll;
            std::snprintf(what, sizeof what, "voices of bit %u", bit); break;
        }
        case 13: {                                           // s2r_set_program_send
            const float send = rng.coin() ? rng.unit() : 0.0f; const uint8_t send_bus = (uint8_t)(rng.coin() ? rng.below(S2R_MAX_BUSES) : 0u);
            if (send != 0.0f || send_bus != 0u) { begin(kMixSend); settle(); }
            for (S2rProgramMix *p : {&keep.prog[program], &model.prog[program]}) { p->send = send; p->send_bus = send_bus; }
            std::snprintf(what, sizeof what, "program send"); break;
        }
        }
        CHECK(keep.used == model.used);
        // after the step: nothing (the type settles lazily, and the next step finds it so), or what a getter or a fill would see
        if (rng.below(4) == 0) return;
        if (fill_time == 0) {
            settle();
            CHECK(keep.queued().empty());
            CHECK(keep.dirty() == model.dirty);
            compare_voices();
            if (rng.coin()) compare_pan();
            if (rng.coin()) compare_bus(false, 1u);
            CHECK(keep.dirty() == model.dirty);
        } else {
            CHECK(keep.dirty() == model.dirty);
            compare_voices();
        }
    }
};

// The first fader call with note_ons waiting at two frames, behind records the queue already holds for them: the program-only
// records must fall into frame order (the stable sort), or the segment that begins at the first frame ramps its voice under the
// program it had before.
void fader_begins_behind_timed_note_ons() {
    std::snprintf(what, sizeof what, "fader begins behind timed note_ons");
    Walk w(65u, 8u, 0u);
    w.begin(kMixPan);                                        // (so that the queue holds a record of its own for every note_on)
    w.current = 3;
    w.note_on(16u, 5); w.note_on(32u, 6);
    w.begin(kMixFader);
    w.keep.prog[3].fader = 0.5f; w.model.prog[3].fader = 0.5f;
    CHECK(w.keep.queued().size() == 4 && w.keep.queued()[1].frame == 16u && w.keep.queued()[1].mask == kMixFader && w.keep.queued()[2].frame == 32u);
    w.mixed_fill(true, 48u);
}

}  // namespace

int main() {
    fader_begins_behind_timed_note_ons();
    const uint32_t shapes[4] = {1u, 63u, 64u, 65u};
    size_t walks = 0;
    for (uint32_t voices : shapes)
        for (uint32_t programs : {1u, 8u})
            for (uint64_t seed = 0; seed < 40; seed++) {
                Walk w(voices, programs, seed);
                for (int step = 0; step < 48; step++) w.step();
                // a last fill of each kind, so that every walk ends on staged buffers
                std::snprintf(what, sizeof what, "last fills");
                w.mixed_fill(false, w.fill_time ? w.fill_time + 16u : 48u);
                w.mixed_fill(true, 48u);
                walks++;
            }
    std::printf("mixer ok (%zu walks)\n", walks);
    return 0;
}
