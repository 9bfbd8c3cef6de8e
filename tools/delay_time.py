"""Times the per-bus feedback delay on the C3 shape of tools/reverb_time.py / master_time.py (65536 voices, 48 kHz,
eight programs of the default patch on eight buses, bench.py's C3 events moved to frame 0: one render launch and one mixdown per
rows slice), eight buses per call, all on ONE handle in one run:

    untouched            bus fills before any delay was set: the kernels and arguments of a build without delays
    1 bus,   D frames    a delay of D frames on bus 0
    8 buses, D frames    the same on every bus                        D = 1, 64, 480, 24 000 and 262 144 (S2R_MAX_DELAY_FRAMES)

each in calls of 16, 1024 and max_frames (MAXFR, 8192) frames.  The untouched fills come first; after them every kind is measured in
one block of N + 2 fills (the first two dropped).  Device time of the mixdown's kernels and of the delay kernel (HIP events around
each, s2r_set_timing) and host wall time per call, medians of N with min .. max.  The bytes the delay kernel moves are counted from
the shapes — per bus with a delay 16 bytes per frame (x in, y out) and 16 bytes per frame of the line (old history in, new history
out); 16 bytes per frame for a bus it only copies — and held against the delay kernel's time.

    timeout -k 10 900 python tools/delay_time.py [--out profiles/r13/bus_delay.txt]

One process and one handle; run it under a time limit of its own, and chain whatever follows it on the GPU with &&.  No pass
threshold."""
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
MAXFR = int(os.environ.get("MAXFR", 8192))
SR = 48000
N = int(os.environ.get("N", 12))          # timed fills of each kind
BANK = 8
DELAYS = [1, 64, 480, 24000, s2.MAX_DELAY_FRAMES]
CALLS = [16, 1024, MAXFR]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r13", "bus_delay.txt"))
    a = ap.parse_args()
    L = s2.load_library()
    for name in ("s2r_debug_bus_mix_ms", "s2r_debug_bus_delay_ms"):
        getattr(L, name).restype = C.c_float
        getattr(L, name).argtypes = [C.c_void_p]
    s = s2.Synth(V, max_frames=MAXFR)
    s.set_patch_bank([s2.default_patch()] * BANK)
    for p in range(BANK):
        s.set_program_pan(p, -1.0 + 2.0 * p / (BANK - 1), 0.5)
        s.set_program_mix(p, 1.0 - p / 16.0, p / 8.0, p)
    period = bench.PERIOD if V >= bench.PERIOD else 1
    cyc = bench.make_c3_events(V, period, 1024)
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

    mono = np.empty(1024, dtype=np.float32)
    for k in range(period + 2):                           # one life of every voice: the stage mix the bench is timed on
        s.note_events(events(k))
        s.sample(mono, SR)
    s.set_timing(True)
    kinds = [("untouched", 0, 0, fr) for fr in CALLS] + [("delay", nb, D, fr) for D in DELAYS for fr in CALLS for nb in (1, BANK)]
    wall = {kd: [] for kd in kinds}
    mix = {kd: [] for kd in kinds}
    dly = {kd: [] for kd in kinds}
    k = [period + 2]

    def fill(kd):
        s.note_events(events(k[0]))
        k[0] += 1
        t0 = time.perf_counter()
        out = s.sample_buses(kd[3], SR, BANK)
        wall[kd].append((time.perf_counter() - t0) * 1e3)
        mix[kd].append(float(L.s2r_debug_bus_mix_ms(s.h)))
        dly[kd].append(float(L.s2r_debug_bus_delay_ms(s.h)))
        return out

    for kd in kinds:
        _, nb, D, fr = kd
        if D:                                             # (set afresh for every kind: the history starts from +0.0)
            for b in range(BANK):
                if b < nb:
                    s.set_bus_delay(b, D, 0.5, -0.25, 0.5, 0.5)
                else:
                    s.clear_bus_delay(b)
        for i in range(N + 2):
            out = fill(kd)
        assert np.isfinite(out).all() and s.get_bus_delay(0)[0] == D and s.get_bus_delay(BANK - 1)[0] == (D if nb == BANK else 0)
        assert (np.array(dly[kd]) > 0.0).all() if D else (np.array(dly[kd]) == 0.0).all()
    block = s.block_voices
    s.close()
    lines = ["tools/delay_time.py: %d voices (block %d), %d Hz, %d programs of the default patch on %d buses, %d buses per call, max_frames %d, "
             "C3 events at frame 0; medians of %d fills (min .. max); build %s" % (V, block, SR, BANK, BANK, BANK, MAXFR, N, L.s2r_build_id().decode())]

    def row(kd):
        m, f, w = (np.array(x[kd][2:]) for x in (mix, dly, wall))
        return m, f, w, "mixdown kernels %7.4f ms (%.4f .. %.4f)   delay kernel %7.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms (%.3f .. %.3f)" % (
            np.median(m), m.min(), m.max(), np.median(f), f.min(), f.max(), np.median(w), w.min(), w.max())

    base = {}
    for kd in kinds:
        _, nb, D, fr = kd
        m, f, w, text = row(kd)
        if not D:
            base[fr] = (np.median(m), np.median(w))
            lines.append("  untouched (no delay ever set)  %5d frames   %s" % (fr, text))
            continue
        lines.append("  delay on %d bus%s D = %6d, %5d frames   %s" % (nb, " ,  " if nb == 1 else "es,", D, fr, text))
        moved = 16.0 * (BANK * fr + nb * D)
        lines.append("      %.3e bytes moved by the delay kernel: %.1f GB/s; delay kernel / this run's untouched mixdown of %d frames = %.3f; "
                     "wall - untouched wall = %+.3f ms" % (moved, moved / (np.median(f) * 1e-3) * 1e-9, fr, np.median(f) / base[fr][0], np.median(w) - base[fr][1]))
    res = os.path.join(s2build.OBJ_DIR, "s2r_delay.resources.txt")
    if os.path.exists(res):
        lines.append("compiler resource usage (s2r_delay.hip, -Rpass-analysis=kernel-resource-usage):")
        for l in open(res):
            lines.append("  " + l.strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for l in lines:
            print(l, flush=True)
            out.write(l + "\n")


if __name__ == "__main__":
    main()
