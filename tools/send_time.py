"""Times s2r_fill_buses without and with aux sends on the C3 shape of tools/bus_time.py / fader_time.py (65536
voices, 48 kHz, 1024 frames, eight programs of the default patch on eight buses, bench.py's C3 events moved to frame 0: one render
launch and one mixdown per fill), at 1 and 8 buses, all on ONE handle in one run:

    untouched   bus fills before any send entry point was called: the kernels and arguments of a build without sends
    sends       bus fills with every program sending to the next bus: the static kernels with sends
    sends+ramp  the same with EVERY program's fader and pan shift on their way: the ramped kernels with sends

The untouched fills come first (a handle cannot forget its sends); `sends` and `sends+ramp` are interleaved, so that both see the
same drift of the box.  Device time of the mixdown's kernel pair (HIP events around it, s2r_set_timing) and host wall time per
call, medians of N.

    python tools/send_time.py [--out profiles/r08/send_mix.txt]

No pass threshold."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import bench
import synth2_amd as s2
from synth2_amd import build as s2build

V = int(os.environ.get("V", 65536))
FR = int(os.environ.get("FR", 1024))
SR = 48000
N = int(os.environ.get("N", 12))          # timed fills of each kind
BANK = 8
STATES = [(0.5, 0.25), (1.0, -0.25)]      # every program's (fader, pan_shift) walks between these two


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r08", "send_mix.txt"))
    a = ap.parse_args()
    L = s2.load_library()
    L.s2r_debug_bus_mix_ms.restype = C.c_float
    L.s2r_debug_bus_mix_ms.argtypes = [C.c_void_p]
    s = s2.Synth(V, max_frames=FR)
    s.set_patch_bank([s2.default_patch()] * BANK)
    for p in range(BANK):
        s.set_program_pan(p, -1.0 + 2.0 * p / (BANK - 1), 0.5)
        s.set_program_mix(p, 1.0 - p / 16.0, p / 8.0, p)
    period = bench.PERIOD if V >= bench.PERIOD else 1
    cyc = bench.make_c3_events(V, period, FR)
    rng = np.random.RandomState(1)

    def events(k):
        """period k's events at frame 0, a program change in front of every note_on, velocities in [0, 1] (tools/bus_time.py)"""
        ev = cyc[k % period]
        out = np.zeros(2 * len(ev), dtype=s2.NOTE_EVENT_DTYPE)
        out["kind"][0::2] = 2
        out["note"][0::2] = rng.randint(0, BANK, len(ev))
        out[1::2] = ev
        out["frame"] = 0
        out["velocity"][1::2] = rng.randint(0, 5, len(ev)) / 4.0
        return out

    mono = np.empty(FR, dtype=np.float32)
    for k in range(period + 2):                           # one life of every voice: the stage mix the bench is timed on
        s.note_events(events(k))
        s.sample(mono, SR)
    s.set_timing(True)
    kinds = [(name, nb) for name in ("untouched", "sends", "sends+ramp") for nb in (1, 8)]
    wall = {kd: [] for kd in kinds}
    dev = {kd: [] for kd in kinds}
    k = [period + 2]

    def fill(kd):
        s.note_events(events(k[0]))
        k[0] += 1
        t0 = time.perf_counter()
        s.sample_buses(FR, SR, kd[1])
        wall[kd].append((time.perf_counter() - t0) * 1e3)
        dev[kd].append(float(L.s2r_debug_bus_mix_ms(s.h)))

    for i in range(N + 2):
        for nb in (1, 8):
            fill(("untouched", nb))
    # every program sends to the next bus; the voices already sounding get what a note_on under their bus's program would have
    for p in range(BANK):
        s.set_program_send(p, 0.5 + p / 16.0, (p + 1) % BANK)
    _, buses = s.voice_mix()
    s.set_voice_sends((0.5 + buses / 16.0).astype(np.float32), ((buses + 1) % BANK).astype(np.uint8))
    state = 0
    for i in range(N + 2):
        for nb in (1, 8):
            fill(("sends", nb))
            state ^= 1
            for p in range(BANK):
                s.set_program_fader(p, *STATES[state])
            fill(("sends+ramp", nb))
            assert s.get_program_fader(BANK - 1) == STATES[state] * 2
    sends, sbuses = s.voice_sends()
    assert (sends > 0.0).all() and len(np.unique(sbuses)) == BANK
    block = s.block_voices
    s.close()
    lines = ["tools/send_time.py: %d voices (block %d), %d frames per fill, %d Hz, %d programs of the default patch on %d buses, each sending "
             "(0.5 + p / 16) to the next bus, C3 events at frame 0; medians of %d fills (min .. max); build %s" % (
                 V, block, FR, SR, BANK, BANK, N, L.s2r_build_id().decode()),
             "sends+ramp: every program's (fader, pan_shift) moves between %r and %r across the fill" % (STATES[0], STATES[1])]
    for kd in kinds:
        d, w = np.array(dev[kd][2:]), np.array(wall[kd][2:])
        lines.append("  %-10s %d bus%s  mixdown kernels %7.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms (%.3f .. %.3f)" % (
            kd[0], kd[1], " " if kd[1] == 1 else "es", np.median(d), d.min(), d.max(), np.median(w), w.min(), w.max()))
    for nb in (1, 8):
        u, sd, r = (np.median(dev[(name, nb)][2:]) for name in ("untouched", "sends", "sends+ramp"))
        lines.append("  kernel time at %d bus%s: sends / untouched %.2f, sends+ramp / sends %.2f" % (nb, "" if nb == 1 else "es", sd / u, r / sd))
    res = os.path.join(s2build.OBJ_DIR, "s2r_aux.resources.txt")
    if os.path.exists(res):
        lines.append("compiler resource usage (s2r_aux.hip, -Rpass-analysis=kernel-resource-usage; template arguments W, NB, RAMP, SEND):")
        for l in open(res):
            if "s2r_bus_mix" in l:
                lines.append("  " + l.strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for l in lines:
            print(l, flush=True)
            out.write(l + "\n")


if __name__ == "__main__":
    main()
