// s2r_mixer_keep.h — the voice mixer's bookkeeping (s2r_fill_panned, s2r_fill_buses): what a program gives the
// voices started under it, what every shard voice got at its note_on, the note_ons still waiting for their frame, and the two loops
// that turn all of it into the gains the mixdown kernels read.  Plain vectors and s2r_rules.h, nothing of HIP and nothing of the
// handle, so that a program of its own checks it on the CPU (tests/native/mixer_keep.cpp).  The device side is S2rVoiceMixer
// (s2r_mixer.h); the handle's code (s2r_host_mix.cpp) calls both.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "s2r_rules.h"

constexpr unsigned kGainsPan = 1u, kGainsBus = 2u, kGainsAll = 3u;   // S2rMixerKeep::dirty(): the panned fill's device arrays, the bus fill's
constexpr uint32_t kMixPan = 1u, kMixLevel = 2u, kMixFader = 4u, kMixSend = 8u;   // S2rMixerKeep::used

// The defaults are a handle that never heard of the mixer.
struct S2rProgramMix {
    float pan = 0.0f, spread = 0.0f;                         // s2r_set_program_pan
    float level = 1.0f, sens = 0.0f; uint8_t bus = 0;        // s2r_set_program_mix
    float send = 0.0f; uint8_t send_bus = 0;                 // s2r_set_program_send
    // s2r_set_program_fader: the pair the caller last set — the target — and the pair the last bus fill left — the applied
    // one; a bus fill ramps every voice's gains from the one to the other
    float fader = 1.0f, shift = 0.0f, fader_app = 1.0f, shift_app = 0.0f;
    bool moving() const { return fader != fader_app || shift != shift_app; }
};

// The bus fill's staging buffer: byte offsets of its [padded_voices] arrays.  gL, gR (floats: pan gain times voice gain, times the
// applied fader), the bus bytes, — once sends are in use — the sends (floats) and the send bus bytes, and behind them, sent with a
// ramped fill only, the gains' steps per frame dL, dR (floats).
constexpr size_t kBusGainBytes = 4 * sizeof(float) + 1 + sizeof(float) + 1;     // per padded voice, everything in use
struct S2rBusLayout { size_t gl, gr, bus, send, send_bus, dl, dr, end; };
inline S2rBusLayout s2r_bus_layout(size_t padded_voices, bool sends) {
    const size_t pv = padded_voices, f = pv * sizeof(float);
    S2rBusLayout o{};
    o.gr = f; o.bus = 2 * f; o.send = o.bus + pv; o.send_bus = o.send + f;
    o.dl = sends ? o.send_bus + pv : o.send;
    o.dr = o.dl + f; o.end = o.dr + f;
    return o;
}

// One bit of `used` per attribute — pan, level (gain and bus), fader (the program the voice was started with: a voice follows that
// program's fader) and send (send and send bus) — set by the first call that leaves the attribute's default (begin); an attribute's
// arrays exist from then on, and until then every voice has its default (pan 0, gain 1 on bus 0, send 0 to bus 0), nothing of it is
// staged or launched, and with used == 0 the note_on paths pay one test.  The voices' arrays are written by the methods below and by
// nobody else: each marks what the device holds of them as stale.
class S2rMixerKeep {
public:
    uint32_t used = 0;                                       // kMixPan | kMixLevel | kMixFader | kMixSend
    std::vector<S2rProgramMix> prog;                         // one entry per bank patch
    // a note_on at a frame INSIDE the next fill: what it gives its voice takes effect there (`mask`: the attributes in use
    // when it came; the other fields hold nothing)
    struct Record { uint32_t local, frame, mask; float pan, gain, send; uint8_t bus, send_bus, program; };

    void shape(uint32_t shard_voices, uint32_t padded_voices) { n = shard_voices; pv = padded_voices; }
    uint32_t voices() const { return n; }
    size_t padded() const { return pv; }
    S2rBusLayout bus_layout() const { return s2r_bus_layout(pv, (used & kMixSend) != 0); }
    // the voices' arrays changed since the gains were last sent to the device (kGainsPan | kGainsBus); sent: by whoever sent them
    unsigned dirty() const { return gains_dirty; }
    void sent(unsigned which) { gains_dirty &= ~which; }
    void mark_bus() { gains_dirty |= kGainsBus; }            // the faders' applied pairs changed, or a ramp is about to be staged
    const std::vector<Record> &queued() const { return timed; }

    // Records of note_ons that had a frame inside a fill which has been rendered since (by any fill: fill_time is back at 0) are the
    // voices' values now.  Called before anything reads or writes the voices' arrays.
    void settle(uint32_t fill_time) {
        if (timed.empty() || fill_time != 0) return;
        for (const Record &r : timed) apply(r);
        timed.clear();
        gains_dirty = kGainsAll;
    }
    // The first call that takes pan, level or send off its default: its arrays, and from here on the note_on paths record it.
    void begin(uint32_t bit) {
        if (bit == kMixPan) pan.assign(n, 0.0f);
        if (bit == kMixLevel) { gain.assign(n, 1.0f); bus.assign(n, 0u); }
        if (bit == kMixSend) { send.assign(n, 0.0f); send_bus.assign(n, 0u); }
        used |= bit; gains_dirty = kGainsAll;
    }
    // ... and the faders: the program every voice holds now, and a record for every note_on the caller still holds at a frame inside
    // the next fill, in event order — they join what the queue already holds for those note_ons (a stable sort by frame: the fields
    // are disjoint, and the order within a frame is the events')
    void begin_faders(std::vector<uint8_t> programs, const std::vector<Record> &waiting) {
        program = std::move(programs);
        timed.insert(timed.end(), waiting.begin(), waiting.end());
        std::stable_sort(timed.begin(), timed.end(), [](const Record &a, const Record &b) { return a.frame < b.frame; });
        used |= kMixFader; gains_dirty = kGainsAll;
    }
    // a note_on under `program_now` took shard voice `local` (the caller has settled): what the program gives it, now or at its frame
    void note_on(uint32_t local, uint32_t program_now, uint8_t note, float velocity, uint32_t frame) {
        const S2rProgramMix &p = prog[program_now];
        Record r{local, frame, used, 0.0f, 0.0f, p.send, p.bus, p.send_bus, (uint8_t)program_now};
        if (used & kMixPan) r.pan = rule_voice_pan(p.pan, p.spread, note);
        if (used & kMixLevel) r.gain = rule_voice_gain(p.level, p.sens, velocity);        // (the other fields are copies: apply looks at r.mask)
        if (frame == 0) { apply(r); gains_dirty = kGainsAll; }
        else timed.push_back(r);
    }
    // A fill split at its event frames takes the queue, and in front of the segment that begins at frame `at` applies its records up
    // to there, from record `k` on.
    std::vector<Record> take_queued() { std::vector<Record> q; q.swap(timed); return q; }
    void apply_through(const std::vector<Record> &q, size_t &k, uint32_t at) {
        for (; k < q.size() && q[k].frame <= at; k++) { apply(q[k]); gains_dirty = kGainsAll; }
    }
    void snap_faders() { for (S2rProgramMix &p : prog) { p.fader_app = p.fader; p.shift_app = p.shift; } }
    bool faders_moving() const {
        if (!(used & kMixFader)) return false;
        for (const S2rProgramMix &p : prog) if (p.moving()) return true;
        return false;
    }
    // a new bank of `count` patches: the surviving programs keep their pans, mix, sends and faders
    void resize_bank(uint32_t count) {
        prog.resize(count);
        if (used & kMixFader) gains_dirty = kGainsAll;       // (a voice whose program fell off the bank follows program 0 now)
    }
    // a checkpoint's programs replace the voices' (faders in use): those still queued belong to the state that was replaced
    template <class F> void restore_programs(F program_of) {
        for (uint32_t i = 0; i < n; i++) program[i] = (uint8_t)program_of(i);
        for (Record &r : timed) r.mask &= ~kMixFader;
        timed.erase(std::remove_if(timed.begin(), timed.end(), [](const Record &r) { return r.mask == 0; }), timed.end());
        gains_dirty = kGainsAll;
    }
    // One attribute's per-voice values out (an attribute never used: its default) and in (the caller has begun it); the caller has
    // settled.  `bytes`: the buses or send buses, null for the pans, which have none.
    void get_voices(uint32_t bit, float *values, uint8_t *bytes) const {
        if (!(used & bit)) { std::fill(values, values + n, bit == kMixLevel ? 1.0f : 0.0f); if (bytes) std::memset(bytes, 0, n); return; }
        std::memcpy(values, (bit == kMixPan ? pan : bit == kMixLevel ? gain : send).data(), (size_t)n * sizeof(float));
        if (bytes) std::memcpy(bytes, (bit == kMixLevel ? bus : send_bus).data(), n);
    }
    void set_voices(uint32_t bit, const float *values, const uint8_t *bytes) {
        std::memcpy((bit == kMixPan ? pan : bit == kMixLevel ? gain : send).data(), values, (size_t)n * sizeof(float));
        if (bytes) std::memcpy((bit == kMixLevel ? bus : send_bus).data(), bytes, n);
        gains_dirty = kGainsAll;
    }

    // The panned fill's gains into `host`, [2][padded_voices] floats: gL then gR of every shard voice's pan (the entries past the
    // shard are not touched).
    void stage_pan(float *host) const {
        for (uint32_t i = 0; i < n; i++) rule_pan_gains((used & kMixPan) ? pan[i] : 0.0f, host + i, host + pv + i);
    }
    // What the bus mixdown reads per voice into `host`, padded_voices * kBusGainBytes bytes laid out by bus_layout() — both pan gains
    // times the voice's gain (one rounded multiply each), times its program's applied fader once faders are in use, the bus byte, the
    // send and its bus byte once sends are in use.  `ramp`: a bus fill of `total` frames with a fader on its way: the gains under the
    // applied pairs and their steps per frame towards the gains under the targets — one staging buffer, one copy.
    void stage_bus(char *host, bool ramp, uint32_t total) const {
        const S2rBusLayout o = bus_layout();
        float *gl = reinterpret_cast<float *>(host + o.gl), *gr = reinterpret_cast<float *>(host + o.gr);
        float *dl = reinterpret_cast<float *>(host + o.dl), *dr = reinterpret_cast<float *>(host + o.dr);
        uint8_t *b = reinterpret_cast<uint8_t *>(host + o.bus);
        const size_t n_prog = prog.size();
        const float fn = (float)total;
        if (used & kMixSend) {
            std::memcpy(host + o.send, send.data(), (size_t)n * sizeof(float));
            std::memcpy(host + o.send_bus, send_bus.data(), (size_t)n);
        }
        for (uint32_t i = 0; i < n; i++) {
            const float p_i = (used & kMixPan) ? pan[i] : 0.0f, w = (used & kMixLevel) ? gain[i] : 1.0f;
            b[i] = (used & kMixLevel) ? bus[i] : (uint8_t)0;
            if (!(used & kMixFader)) {
                float l, r;
                rule_pan_gains(p_i, &l, &r);
                gl[i] = l * w; gr[i] = r * w;
                continue;
            }
            const S2rProgramMix &p = prog[program[i] < n_prog ? program[i] : 0u];        // (past a later, smaller bank: program 0, as its patch is)
            float g0l, g0r;
            rule_fader_gains(p_i, w, p.fader_app, p.shift_app, &g0l, &g0r);
            gl[i] = g0l; gr[i] = g0r;
            if (!ramp) continue;
            if (p.moving()) {
                float g1l, g1r;
                rule_fader_gains(p_i, w, p.fader, p.shift, &g1l, &g1r);
                const float sl = g1l - g0l, sr = g1r - g0r;
                dl[i] = sl / fn; dr[i] = sr / fn;
            } else { dl[i] = 0.0f; dr[i] = 0.0f; }
        }
    }

private:
    uint32_t n = 0; size_t pv = 0;                           // shard voices, and the arrays' length on the device
    std::vector<float> pan, gain, send;                      // [shard voices] each, once its bit is set
    std::vector<uint8_t> bus, send_bus, program;
    std::vector<Record> timed;                               // in non-decreasing frame order, event order within a frame
    unsigned gains_dirty = kGainsAll;
    // the only place that writes the voices' arrays from a record
    void apply(const Record &r) {
        if (r.mask & kMixPan) pan[r.local] = r.pan;
        if (r.mask & kMixLevel) { gain[r.local] = r.gain; bus[r.local] = r.bus; }
        if (r.mask & kMixFader) program[r.local] = r.program;
        if (r.mask & kMixSend) { send[r.local] = r.send; send_bus[r.local] = r.send_bus; }
    }
};
