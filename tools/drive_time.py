"""Times the per-bus drive on the C3 shape of tools/room_time.py (65536 voices, 48 kHz, eight programs of the default
patch on eight buses, bench.py's C3 events moved to frame 0), eight buses per call, all on ONE handle in one run:

    untouched              bus fills before any drive was set: the kernels and arguments of a build without it
    1 bus                  a drive on bus 0 (the other seven buses are copied by the same launch)
    8 buses                a drive on every bus: tiles x 8 workgroups

each in calls of 1024 and 64 frames.  The untouched fills come first; after them every kind is measured in one block of N + 2 fills
(the first two dropped).  The table is s2r_drive_curve's tanh at amount 3, pre 4, dry 0.25, wet 1.  Device time of the mixdown's kernels
and of the stage's kernel (HIP events around each, s2r_set_timing) and host wall time per call, medians of N with min .. max, and the
kernel's median over the call's frames in ns.

    timeout -k 10 600 python tools/drive_time.py [--out profiles/r20/bus_drive.txt]

--form LABEL names the kernel form the loaded library holds (default: planes); with --append the rows are added to --out instead of
replacing it: the obvious form, one lane per output frame recomputing its own 65 oversampled samples from global memory, is built by
S2R_DRIVE_SERIAL=1 into libs2r_driveserial.so (synth2_amd/build.py) and timed by S2R_AB_LIB=synth2_amd/libs2r_driveserial.so ... --form
serial --append; the tiled form with w[] interleaved in LDS instead of in four phase planes by S2R_DRIVE_INTERLEAVED=1 into
libs2r_driveinterleaved.so, --form interleaved.

A/B against a library kept from another build (S2R_AB_LIB=<path>): --ab LABEL times the plain fills of a handle WITHOUT a drive —
s2r_fill_buses, s2r_fill_master with and without stems, 1024 frames — and appends one line per kind to --out; run the two libraries
in turn, one process each, and compare this build's median with the other library's min .. max (the protocol of
profiles/r16/post_stages.txt).

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
MAXFR = int(os.environ.get("MAXFR", 1024))
SR = 48000
N = int(os.environ.get("N", 12))          # timed fills of each kind
BANK = 8
SHAPES = [1, BANK]                        # buses with a drive
CALLS = [1024, 64]
AB_KINDS = [("buses", "s2r_fill_buses            "), ("stems", "s2r_fill_master, stems    "), ("only", "s2r_fill_master, no stems ")]
LEVELS = (4.0, 0.25, 1.0)                 # pre, dry, wet
AMOUNT = 3.0                              # of the tanh table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r20", "bus_drive.txt"))
    ap.add_argument("--ab", default=None, help="a label for this library: time the plain fills and append one line per kind to --out")
    ap.add_argument("--form", default="planes", help="the kernel form the loaded library holds")
    ap.add_argument("--append", action="store_true", help="add the rows to --out instead of replacing it")
    a = ap.parse_args()
    L = s2.load_library()
    has_drive = hasattr(L, "s2r_debug_bus_drive_ms")       # (the other library of an A/B run may be older than the stage)
    for name in ("s2r_debug_bus_mix_ms", "s2r_debug_master_ms") + (("s2r_debug_bus_drive_ms",) if has_drive else ()):
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
    k = [period + 2]
    build = L.s2r_build_id().decode()
    block = s.block_voices

    def drive_ms():
        return float(L.s2r_debug_bus_drive_ms(s.h)) if has_drive else 0.0

    if a.ab is not None:                                  # the plain fills of a handle without a drive
        wall, mix, mst, rmt = ({kd[0]: [] for kd in AB_KINDS} for _ in range(4))
        for kind, _ in AB_KINDS:
            for i in range(N + 2):
                s.note_events(events(k[0]))
                k[0] += 1
                t0 = time.perf_counter()
                if kind == "buses":
                    out = s.sample_buses(1024, SR, BANK)
                else:
                    out = s.sample_master(1024, SR, BANK, stems=(kind == "stems"))[0]
                wall[kind].append((time.perf_counter() - t0) * 1e3)
                mix[kind].append(float(L.s2r_debug_bus_mix_ms(s.h)))
                mst[kind].append(float(L.s2r_debug_master_ms(s.h)) if kind != "buses" else 0.0)
                rmt[kind].append(drive_ms())
            assert np.isfinite(out).all() and np.abs(out).max() > 0.0 and not np.array(rmt[kind]).any()
        s.close()
        lines = []
        for kind, name in AB_KINDS:
            m, f, w = (np.array(x[kind][2:]) for x in (mix, mst, wall))
            lines.append("  A/B %-8s (build %s)  %s mixdown kernels %7.4f ms (%.4f .. %.4f)   master kernel %7.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms "
                         "(%.3f .. %.3f)" % (a.ab, build, name, np.median(m), m.min(), m.max(), np.median(f), f.min(), f.max(), np.median(w), w.min(), w.max()))
    else:
        curve = s2.drive_curve(s2.DRIVE_TANH, AMOUNT)
        kinds = [("untouched", 0, fr) for fr in CALLS] + [("drive", nb, fr) for nb in SHAPES for fr in CALLS]
        wall, mix, stg = ({kd: [] for kd in kinds} for _ in range(3))
        for kd in kinds:
            what, nb, fr = kd
            for b in range(BANK):                         # (set afresh for every kind: the state starts from silence)
                s.clear_bus_drive(b)
                if b < nb:
                    s.set_bus_drive(b, curve, *LEVELS)
            for i in range(N + 2):
                s.note_events(events(k[0]))
                k[0] += 1
                t0 = time.perf_counter()
                out = s.sample_buses(fr, SR, BANK)
                wall[kd].append((time.perf_counter() - t0) * 1e3)
                mix[kd].append(float(L.s2r_debug_bus_mix_ms(s.h)))
                stg[kd].append(drive_ms())
            assert np.isfinite(out).all() and (s.get_bus_drive(0) is not None) == (what == "drive")
            assert (np.array(stg[kd]) > 0.0).all() if nb else (np.array(stg[kd]) == 0.0).all()
        s.close()
        lines = ["tools/drive_time.py, kernel form: %s.  %d voices (block %d), %d Hz, %d programs of the default patch on %d buses, %d buses per call, max_frames %d, "
                 "C3 events at frame 0; the tanh table at amount %g, pre %g, dry %g, wet %g; medians of %d fills (min .. max); build %s"
                 % ((a.form, V, block, SR, BANK, BANK, BANK, MAXFR, AMOUNT) + LEVELS + (N, build))]
        base = {}
        for kd in kinds:
            what, nb, fr = kd
            m, f, w = (np.array(x[kd][2:]) for x in (mix, stg, wall))
            text = "mixdown kernels %7.4f ms (%.4f .. %.4f)   %s %7.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms (%.3f .. %.3f)" % (
                np.median(m), m.min(), m.max(), "drive kernel", np.median(f), f.min(), f.max(), np.median(w), w.min(), w.max())
            if not nb:
                base[fr] = (np.median(m), np.median(w))
                lines.append("  untouched (no drive ever set)       %5d frames   %s" % (fr, text))
                continue
            lines.append("  %-11s %d bus%s          %5d frames   %s" % (a.form, nb, "  " if nb == 1 else "es", fr, text))
            lines.append("      %.1f ns per frame; stage / this run's untouched mixdown of %d frames = %.3f; wall - untouched wall = %+.3f ms"
                         % (np.median(f) * 1e6 / fr, fr, np.median(f) / base[fr][0], np.median(w) - base[fr][1]))
        res = os.path.join(s2build.OBJ_DIR, "s2r_drive.resources.txt")
        if os.path.exists(res) and not os.environ.get("S2R_AB_LIB"):
            lines.append("compiler resource usage (s2r_drive.hip, -Rpass-analysis=kernel-resource-usage):")
            for l in open(res):
                lines.append("  " + l.strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if (a.ab is not None or a.append) else "w") as out:
        for l in lines:
            print(l, flush=True)
            out.write(l + "\n")


if __name__ == "__main__":
    main()
