"""Times the loudness and true-peak meters on the C3 shape of tools/limiter_time.py (65536 voices, 48 kHz, eight
programs of the default patch on eight buses, bench.py's C3 events moved to frame 0), eight buses per call, master only (the stems
never cross to the host), at 1024 and at 8192 frames per fill (FR=8192), all kinds on ONE handle in one run:

    s2r_fill_master, no meter              before a meter was ever set
    s2r_fill_master, meter                 hop 4800, an hour of hop rows
    s2r_fill_master, meter and limiter     the limiter (240, 480) at half the peak of the unlimited master in front of the meter
    s2r_fill_master, EQ and dynamics       four bands and a compressor on every bus, no meter: the two other stages that are serial
                                           in the frame index, at the same shape, for comparison

Every kind is measured in one block of N + 2 fills (the first two dropped).  Device time of the master, limiter, loudness, EQ and
dynamics kernels (HIP events around each, s2r_set_timing) and host wall time per call, medians of N.

    python tools/loudness_time.py [--out profiles/r22/master_loudness.txt]

A/B against a library kept from another build (S2R_AB_LIB=<path>, see synth2_amd/build.py): --ab LABEL appends one line per kind the
loaded library has — the serial build (S2R_LOUDNESS_SERIAL=1 python -m synth2_amd.build) for the meter's own kernel, a library kept
from the parent commit, which is timed on the fill without a meter alone — to --out instead of replacing it; run the libraries in
turn, one process each, three rounds, and compare this build's no-meter median with the parent library's min .. max.

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
TIMERS = ("master", "limiter", "loudness", "bus_eq", "dyn")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r22", "master_loudness.txt"))
    ap.add_argument("--ab", default=None, help="a label for this library: append one line per kind to --out")
    a = ap.parse_args()
    L = s2.load_library()
    has_meter = hasattr(L, "s2r_debug_loudness_ms")
    timers = [t for t in TIMERS if hasattr(L, "s2r_debug_%s_ms" % t)]
    for t in timers:
        getattr(L, "s2r_debug_%s_ms" % t).restype = C.c_float
        getattr(L, "s2r_debug_%s_ms" % t).argtypes = [C.c_void_p]
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
    kinds = [("none", "s2r_fill_master, no meter         ")]
    if has_meter:
        kinds += [("meter", "s2r_fill_master, meter            "), ("both", "s2r_fill_master, meter and limiter")]
    if a.ab is None:
        kinds += [("stages", "s2r_fill_master, EQ and dynamics  ")]
    wall = {kd[0]: [] for kd in kinds}
    dev = {kd[0]: {t: [] for t in timers} for kd in kinds}
    k = period + 2
    peak = 0.0
    readings = None
    for kind, _ in kinds:
        if kind in ("meter", "both"):
            s.set_master_loudness(SR, SR // 10, 36000)
        if kind == "both":
            s.set_master_limiter(peak / 2.0, 240, 480)
        if kind == "stages":
            s.clear_master_loudness()
            s.clear_master_limiter()
            band = s2.eq_design(s2.EQ_PEAK, 1000.0, 3.0, 1.0, SR)
            curve = s2.dynamics_curve(-30.0, 4.0, 6.0, 0.0)
            for b in range(BANK):
                s.set_bus_eq(b, np.stack([band] * 4))
                s.set_bus_dynamics(b, b, curve, s2.dynamics_coef(5.0, SR), s2.dynamics_coef(100.0, SR))
        for i in range(N + 2):
            s.note_events(events(k))
            k += 1
            t0 = time.perf_counter()
            out = s.sample_master(FR, SR, BANK, stems=False)[0]
            wall[kind].append((time.perf_counter() - t0) * 1e3)
            for t in timers:
                dev[kind][t].append(float(getattr(L, "s2r_debug_%s_ms" % t)(s.h)))
            if kind == "none":
                peak = max(peak, float(np.abs(out).max()))
        assert np.isfinite(out).all() and np.abs(out).max() > 0.0
        if kind == "meter":
            readings = (s.loudness(BANK), s.true_peak()[1], s.get_master_loudness()[3])
            assert readings[2] == ((N + 2) * FR) // (SR // 10)
    block = s.block_voices
    s.close()

    def row(kind):
        w = np.array(wall[kind][2:])
        parts = []
        for t in timers:
            m = np.array(dev[kind][t][2:])
            parts.append("%s %7.4f ms (%.4f .. %.4f)" % (t, np.median(m), m.min(), m.max()))
        return "   ".join(parts) + "   host wall per call %7.3f ms (%.3f .. %.3f)" % (np.median(w), w.min(), w.max())

    build = L.s2r_build_id().decode()
    if a.ab is not None:
        lines = ["  A/B %-8s %d frames (build %s)  %s %s" % (a.ab, FR, build, name, row(kind)) for kind, name in kinds]
    else:
        lines = ["tools/loudness_time.py: %d voices (block %d), %d frames per fill, %d Hz, %d programs of the default patch on %d buses, %d buses per call, "
                 "master only, C3 events at frame 0; kernel times by HIP events; medians of %d fills (min .. max); build %s" % (V, block, FR, SR, BANK, BANK, BANK, N, build)]
        for kind, name in kinds:
            lines.append("  " + name + " " + row(kind))
        if readings:
            lines.append("  the master after %d hops: momentary %.2f, short-term %.2f, integrated %.2f LKFS; true peak held L %.4f R %.4f"
                         % (readings[2], readings[0][0], readings[0][1], readings[0][2], readings[1][0], readings[1][1]))
        res = os.path.join(s2build.OBJ_DIR, "s2r_loudness.resources.txt")
        if os.path.exists(res):
            lines.append("compiler resource usage (s2r_loudness.hip, -Rpass-analysis=kernel-resource-usage):")
            for l in open(res):
                lines.append("  " + l.strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.ab is not None or FR != 1024 else "w") as out:
        for l in lines:
            print(l, flush=True)
            out.write(l + "\n")


if __name__ == "__main__":
    main()
