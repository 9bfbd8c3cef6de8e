"""Times s2r_fill_buses with and without moving program faders on the C3 shape of tools/bus_time.py (65536
voices, 48 kHz, 1024 frames, eight programs of the default patch on eight buses, bench.py's C3 events moved to frame 0: one
render launch and one mixdown per fill), at 1 and 8 buses, all on ONE handle in one run:

    untouched   bus fills before any fader entry point was called: the static kernels on the mixer's arrays
    steady      bus fills with applied == target (away from the default after the first move): the static kernels on gains the
                host recomputed — the fill after a ramped one sends them again
    ramped      bus fills with EVERY program's fader and pan shift on their way: the ramped kernels

interleaved, so that every kind sees the same drift of the box.  Device time of the mixdown's kernel pair (HIP events around
it, s2r_set_timing) and host wall time per call, medians of N.

    python tools/fader_time.py [--out profiles/r07/fader_mix.txt]

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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r07", "fader_mix.txt"))
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
    kinds = [(name, nb) for name in ("untouched", "steady", "ramped") for nb in (1, 8)]
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
    state = 0
    for i in range(N + 2):
        for nb in (1, 8):
            fill(("steady", nb))
            state ^= 1
            t0 = time.perf_counter()
            for p in range(BANK):
                s.set_program_fader(p, *STATES[state])
            if i == 0 and nb == 1:
                first_set_ms = (time.perf_counter() - t0) * 1e3       # reads the voices' programs back from the device, once
            fill(("ramped", nb))
            assert s.get_program_fader(BANK - 1) == STATES[state] * 2
    block = s.block_voices
    s.close()
    lines = ["tools/fader_time.py: %d voices (block %d), %d frames per fill, %d Hz, %d programs of the default patch on %d buses, C3 events at "
             "frame 0; medians of %d interleaved fills (min .. max); build %s" % (V, block, FR, SR, BANK, BANK, N, L.s2r_build_id().decode()),
             "ramped: every program's (fader, pan_shift) moves between %r and %r across the fill; the first set_program_fader calls "
             "(the programs read back once) took %.3f ms" % (STATES[0], STATES[1], first_set_ms)]
    for kd in kinds:
        d, w = np.array(dev[kd][2:]), np.array(wall[kd][2:])
        lines.append("  %-9s %d bus%s  mixdown kernels %7.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms (%.3f .. %.3f)" % (
            kd[0], kd[1], " " if kd[1] == 1 else "es", np.median(d), d.min(), d.max(), np.median(w), w.min(), w.max()))
    for nb in (1, 8):
        r, st = np.median(dev[("ramped", nb)][2:]), np.median(dev[("steady", nb)][2:])
        lines.append("  ramped / steady kernel time at %d bus%s: %.2f" % (nb, "" if nb == 1 else "es", r / st))
    res = os.path.join(s2build.OBJ_DIR, "s2r_aux.resources.txt")
    if os.path.exists(res):
        lines.append("compiler resource usage (s2r_aux.hip, -Rpass-analysis=kernel-resource-usage; Lb0: static, Lb1: ramped):")
        for l in open(res):
            if "s2r_bus_mix" in l and "ILi4E" in l:
                lines.append("  " + l.strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for l in lines:
            print(l, flush=True)
            out.write(l + "\n")


if __name__ == "__main__":
    main()
