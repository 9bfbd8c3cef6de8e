// s2r_mixer.cpp — the device side of the voice mixer (s2r_mixer.h): once-only allocations, the gains' way to the device, one slice's
// mixdown launch, the timers.  Compiled with hipcc, -ffp-contract=off.
#include "s2r_mixer.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace {

// mapped host memory the host reads behind a synchronise: coherent and portable, as every pinned buffer of s2r_host.cpp
constexpr unsigned kHostPolled = hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable;

#define MIX_HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

}  // namespace

hipError_t S2rVoiceMixer::prepare(const S2rMixCtx &c, uint32_t n_buses, bool stems) {
    if (!pan_rows) {
        // The rows buffer, sized ONCE (s2r.h): whole fills where they fit into 256 MiB, else slices of a multiple of 16 frames —
        // a fill split at a multiple of 16 renders the same bits (s2r.h, s2r_note_events).  (Shorter slices, whose rows would
        // stay closer to the compute units, were measured and are slower: profiles/r05/pan_mix.txt)
        uint32_t slice = (uint32_t)std::min<size_t>((((size_t)256 << 20) / sizeof(float) / c.shard_voices) & ~(size_t)15, 1u << 30);
        if (const char *e = std::getenv("S2R_PAN_SLICE")) slice = (uint32_t)std::atol(e) & ~15u;      // (measurement: tools/pan_time.py)
        const uint32_t whole = (c.max_frames + 15u) & ~15u;
        if (slice < 16u) slice = 16u;
        if (slice > whole) slice = whole;
        MIX_HIP(hipMalloc((void **)&pan_rows, (size_t)c.shard_voices * slice * sizeof(float)));
        pan_slice = slice;
    }
    // the workgroups' partial rows of the mixdown asked for (and the bus fill's pinned output), once each
    if (!n_buses && !pan_partials) MIX_HIP(hipMalloc((void **)&pan_partials, (size_t)c.n_blocks * 2u * pan_slice * sizeof(float)));
    if (n_buses && !bus_partials) MIX_HIP(hipMalloc((void **)&bus_partials, (size_t)c.n_blocks * 2u * S2R_MAX_BUSES * pan_slice * sizeof(float)));
    if (n_buses && stems && !bus_out) {
        MIX_HIP(hipHostMalloc((void **)&bus_out, (size_t)2 * S2R_MAX_BUSES * c.max_frames * sizeof(float), kHostPolled));
        MIX_HIP(hipHostGetDevicePointer((void **)&bus_out_dev, bus_out, 0));
    }
    pan_ev_used = 0;
    return hipSuccess;
}

hipError_t S2rVoiceMixer::send_pan_gains(const S2rMixCtx &c, S2rMixerKeep &keep) {
    if (!(keep.dirty() & kGainsPan)) return hipSuccess;
    const size_t bytes = 2 * (size_t)c.padded_voices * sizeof(float);
    if (!gains_host) {
        MIX_HIP(hipHostMalloc((void **)&gains_host, bytes, hipHostMallocDefault));
        std::memset(gains_host, 0, bytes);
        MIX_HIP(hipMalloc((void **)&gains_dev, bytes));
        MIX_HIP(hipEventCreateWithFlags(&gains_sent, hipEventDisableTiming));
    } else MIX_HIP(hipEventSynchronize(gains_sent));             // (the last copy may still be reading the pinned buffer)
    keep.stage_pan(gains_host);
    MIX_HIP(hipMemcpyAsync(gains_dev, gains_host, bytes, hipMemcpyHostToDevice, c.stream));
    MIX_HIP(hipEventRecord(gains_sent, c.stream));
    keep.sent(kGainsPan);
    return hipSuccess;
}

hipError_t S2rVoiceMixer::send_bus_gains(const S2rMixCtx &c, S2rMixerKeep &keep, bool ramp, uint32_t total) {
    if (!(keep.dirty() & kGainsBus) && bus_dev_ramped == ramp) return hipSuccess;
    const size_t bytes = (size_t)c.padded_voices * kBusGainBytes;
    if (!bus_gains_host) {
        MIX_HIP(hipHostMalloc((void **)&bus_gains_host, bytes, hipHostMallocDefault));
        std::memset(bus_gains_host, 0, bytes);
        MIX_HIP(hipMalloc((void **)&bus_gains_dev, bytes));
        MIX_HIP(hipEventCreateWithFlags(&bus_gains_sent, hipEventDisableTiming));
    } else MIX_HIP(hipEventSynchronize(bus_gains_sent));
    keep.stage_bus(bus_gains_host, ramp, total);
    const S2rBusLayout o = keep.bus_layout();
    MIX_HIP(hipMemcpyAsync(bus_gains_dev, bus_gains_host, ramp ? o.end : o.dl, hipMemcpyHostToDevice, c.stream));
    MIX_HIP(hipEventRecord(bus_gains_sent, c.stream));
    keep.sent(kGainsBus);
    bus_dev_ramped = ramp;
    return hipSuccess;
}

hipError_t S2rVoiceMixer::sends_begin(const S2rMixCtx &c) {
    if (!bus_gains_host) return hipSuccess;
    MIX_HIP(hipEventSynchronize(bus_gains_sent));
    std::memset(bus_gains_host, 0, (size_t)c.padded_voices * kBusGainBytes);
    return hipSuccess;
}

hipError_t S2rVoiceMixer::mix_slice(const S2rMixCtx &c, bool sends, uint32_t at, uint32_t len, uint32_t n_buses, uint32_t total, bool ramp, float *bus_dst) {
    const uint32_t n_groups = c.mix_groups, blocks_per_group = (c.n_blocks + n_groups - 1) / n_groups;
    if (c.timing) {
        while (pan_ev.size() < pan_ev_used + 2) { hipEvent_t e; MIX_HIP(hipEventCreate(&e)); pan_ev.push_back(e); }
        MIX_HIP(hipEventRecord(pan_ev[pan_ev_used], c.stream));
    }
    if (n_buses) {
        S2rBusMix m{};
        const S2rBusLayout o = s2r_bus_layout(c.padded_voices, sends);
        const char *dev = bus_gains_dev;
        m.rows = pan_rows;
        m.gain_l = reinterpret_cast<const float *>(dev + o.gl); m.gain_r = reinterpret_cast<const float *>(dev + o.gr);
        m.bus = reinterpret_cast<const uint8_t *>(dev + o.bus);
        m.n_voices = c.shard_voices; m.block_voices = c.block_voices; m.n_blocks = c.n_blocks;
        m.frames = len; m.stride = len;                          // (the render kernel's rows are `frames` apart)
        m.partials = bus_partials; m.pstride = pan_slice;
        m.n_groups = n_groups; m.blocks_per_group = blocks_per_group;
        m.out = bus_dst + 2u * (size_t)at; m.ostride = 2u * (size_t)total;
        m.n_buses = n_buses;
        if (ramp) {
            m.d_l = reinterpret_cast<const float *>(dev + o.dl); m.d_r = reinterpret_cast<const float *>(dev + o.dr);
            m.frame_base = at;
        }
        if (sends) {
            m.send = reinterpret_cast<const float *>(dev + o.send); m.send_bus = reinterpret_cast<const uint8_t *>(dev + o.send_bus);
        }
        MIX_HIP(s2r_launch_bus_mix(m, c.stream));
    } else {
        S2rPanMix m{};
        m.rows = pan_rows; m.gain_l = gains_dev; m.gain_r = gains_dev + c.padded_voices;
        m.n_voices = c.shard_voices; m.block_voices = c.block_voices; m.n_blocks = c.n_blocks;
        m.frames = len; m.stride = len;                          // (the render kernel's rows are `frames` apart)
        m.partials = pan_partials; m.pstride = pan_slice;
        m.n_groups = n_groups; m.blocks_per_group = blocks_per_group;
        m.out = c.out_host_dev + 2u * (size_t)at;
        MIX_HIP(s2r_launch_pan_mix(m, c.stream));
    }
    if (c.timing) { MIX_HIP(hipEventRecord(pan_ev[pan_ev_used + 1], c.stream)); pan_ev_used += 2; }
    return hipSuccess;
}

hipError_t S2rVoiceMixer::read_timers(uint32_t n_buses) {
    float sum = 0.0f;
    for (size_t k = 0; k < pan_ev_used; k += 2) { float ms = 0.0f; MIX_HIP(hipEventElapsedTime(&ms, pan_ev[k], pan_ev[k + 1])); sum += ms; }
    (n_buses ? bus_mix_ms : pan_mix_ms) = sum;
    return hipSuccess;
}

void S2rVoiceMixer::release() {
    if (gains_host) (void)hipHostFree(gains_host);
    if (gains_dev) (void)hipFree(gains_dev);
    if (gains_sent) (void)hipEventDestroy(gains_sent);
    if (pan_rows) (void)hipFree(pan_rows);
    if (pan_partials) (void)hipFree(pan_partials);
    if (bus_gains_host) (void)hipHostFree(bus_gains_host);
    if (bus_gains_dev) (void)hipFree(bus_gains_dev);
    if (bus_gains_sent) (void)hipEventDestroy(bus_gains_sent);
    if (bus_partials) (void)hipFree(bus_partials);
    if (bus_out) (void)hipHostFree(bus_out);
    for (hipEvent_t e : pan_ev) (void)hipEventDestroy(e);
    *this = S2rVoiceMixer{};
}
