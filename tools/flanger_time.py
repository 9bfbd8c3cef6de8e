"""Times the per-bus flanger, eight programs of the default patch on eight buses, eight buses per call, bench.py's C3
events moved to frame 0, all on ONE handle in one run:

    untouched              bus fills before any flanger was set: the kernels and arguments of a build without it
    1 bus                  a flanger on bus 0 (the other seven buses are copied by the same launch)
    8 buses                a flanger on every bus: eight workgroups, one walking wavefront each

each at H = 33 (base 32, no depth), 145 (48 + 96.5) and 4096 (32 + 4063), in calls of 16, 1024 and 8192 frames.  The stage's time does
not depend on the voices in front of it, and a handle of 8192 frames for 65 536 voices is large, so these rows run on 4096 voices (V,
MAXFR in the environment change that).  The untouched fills come first; after them every kind is measured in one block of N + 2 fills
(the first two dropped).  LFO 4 Hz, the right channel a quarter turn ahead, feedback 0.5, cross 0.25, dry 0.5, wet 0.75.  Device time of
the mixdown's kernels and of the stage's kernel (HIP events around each, s2r_set_timing) and host wall time per call, medians of N with
min .. max, and the kernel's median over the call's frames in ns.

    timeout -k 10 900 python tools/flanger_time.py [--out profiles/r21/bus_flanger.txt]

--form LABEL names the kernel form the loaded library holds (default: tiled); with --append the rows are added to --out instead of
replacing it: the obvious form, one lane per bus and channel stepping frame by frame with the line in global memory, is built by
S2R_FLANGER_SERIAL=1 into libs2r_flangerserial.so (synth2_amd/build.py) and timed by S2R_AB_LIB=synth2_amd/libs2r_flangerserial.so ...
--form serial --append.

A/B against a library kept from another build (S2R_AB_LIB=<path>): --ab LABEL times the plain fills of a handle WITHOUT a flanger —
s2r_fill_buses, s2r_fill_master with and without stems, 1024 frames, 65 536 voices, max_frames 1024 — and appends one line per kind to
--out; run the two libraries in turn, one process each, three rounds, and compare this build's median of its rounds' medians with the
other library's min .. max over its rounds' medians (the protocol and the bound of profiles/r12/post_chain.txt).

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

SR = 48000
N = int(os.environ.get("N", 12))          # timed fills of each kind
BANK = 8
BUSES = [1, BANK]                         # buses with a flanger
CALLS = [16, 1024, 8192]
SHAPES = [(33, 32.0, 0.0), (145, 48.0, 96.5), (4096, 32.0, 4063.0)]
AB_KINDS = [("buses", "s2r_fill_buses            "), ("stems", "s2r_fill_master, stems    "), ("only", "s2r_fill_master, no stems ")]
RATE = (89478 * 4, 0x40000000)            # phase_inc, spread
LEVELS = (0.5, 0.25, 0.5, 0.75)           # feedback, cross, dry, wet


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r21", "bus_flanger.txt"))
    ap.add_argument("--ab", default=None, help="a label for this library: time the plain fills and append one line per kind to --out")
    ap.add_argument("--form", default="tiled", help="the kernel form the loaded library holds")
    ap.add_argument("--append", action="store_true", help="add the rows to --out instead of replacing it")
    a = ap.parse_args()
    V = int(os.environ.get("V", 65536 if a.ab is not None else 4096))
    MAXFR = int(os.environ.get("MAXFR", 1024 if a.ab is not None else 8192))
    L = s2.load_library()
    has_stage = hasattr(L, "s2r_debug_bus_flanger_ms")     # (the other library of an A/B run may be older than the stage)
    for name in ("s2r_debug_bus_mix_ms", "s2r_debug_master_ms") + (("s2r_debug_bus_flanger_ms",) if has_stage else ()):
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

    def stage_ms():
        return float(L.s2r_debug_bus_flanger_ms(s.h)) if has_stage else 0.0

    if a.ab is not None:                                  # the plain fills of a handle without a flanger
        wall, mix, mst, stg = ({kd[0]: [] for kd in AB_KINDS} for _ in range(4))
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
                stg[kind].append(stage_ms())
            assert np.isfinite(out).all() and np.abs(out).max() > 0.0 and not np.array(stg[kind]).any()
        s.close()
        lines = []
        for kind, name in AB_KINDS:
            m, f, w = (np.array(x[kind][2:]) for x in (mix, mst, wall))
            lines.append("  A/B %-8s (build %s)  %s mixdown kernels %7.4f ms (%.4f .. %.4f)   master kernel %7.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms "
                         "(%.3f .. %.3f)" % (a.ab, build, name, np.median(m), m.min(), m.max(), np.median(f), f.min(), f.max(), np.median(w), w.min(), w.max()))
    else:
        calls = [fr for fr in CALLS if fr <= MAXFR]
        kinds = [("untouched", 0, 0, fr) for fr in calls] + [("flanger", nb, sh, fr) for sh in range(len(SHAPES)) for nb in BUSES for fr in calls]
        wall, mix, stg = ({kd: [] for kd in kinds} for _ in range(3))
        for kd in kinds:
            what, nb, sh, fr = kd
            for b in range(BANK):                         # (set afresh for every kind: the state starts from silence)
                if has_stage:
                    s.clear_bus_flanger(b)
                if b < nb:
                    s.set_bus_flanger(b, SHAPES[sh][1], SHAPES[sh][2], *RATE, *LEVELS)
            for i in range(N + 2):
                s.note_events(events(k[0]))
                k[0] += 1
                t0 = time.perf_counter()
                out = s.sample_buses(fr, SR, BANK)
                wall[kd].append((time.perf_counter() - t0) * 1e3)
                mix[kd].append(float(L.s2r_debug_bus_mix_ms(s.h)))
                stg[kd].append(stage_ms())
            assert np.isfinite(out).all()
            assert (np.array(stg[kd]) > 0.0).all() if nb else (np.array(stg[kd]) == 0.0).all()
        s.close()
        lines = ["tools/flanger_time.py, kernel form: %s.  %d voices (block %d), %d Hz, %d programs of the default patch on %d buses, %d buses per call, max_frames %d, "
                 "C3 events at frame 0; phase_inc %d, spread 0x%08x, feedback %g, cross %g, dry %g, wet %g; medians of %d fills (min .. max); build %s"
                 % ((a.form, V, block, SR, BANK, BANK, BANK, MAXFR) + RATE + LEVELS + (N, build))]
        base = {}
        for kd in kinds:
            what, nb, sh, fr = kd
            m, f, w = (np.array(x[kd][2:]) for x in (mix, stg, wall))
            text = "mixdown kernels %7.4f ms (%.4f .. %.4f)   %s %7.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms (%.3f .. %.3f)" % (
                np.median(m), m.min(), m.max(), "flanger kernel", np.median(f), f.min(), f.max(), np.median(w), w.min(), w.max())
            if not nb:
                base[fr] = (np.median(m), np.median(w))
                lines.append("  untouched (no flanger ever set)            %5d frames   %s" % (fr, text))
                continue
            lines.append("  %-8s H %4d  %d bus%s          %5d frames   %s" % (a.form, SHAPES[sh][0], nb, "  " if nb == 1 else "es", fr, text))
            lines.append("      %.1f ns per frame; stage / this run's untouched mixdown of %d frames = %.3f; wall - untouched wall = %+.3f ms"
                         % (np.median(f) * 1e6 / fr, fr, np.median(f) / base[fr][0], np.median(w) - base[fr][1]))
        res = os.path.join(s2build.OBJ_DIR, "s2r_flanger.resources.txt")
        if os.path.exists(res) and not os.environ.get("S2R_AB_LIB"):
            lines.append("compiler resource usage (s2r_flanger.hip, -Rpass-analysis=kernel-resource-usage):")
            for l in open(res):
                lines.append("  " + l.strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if (a.ab is not None or a.append) else "w") as out:
        for l in lines:
            print(l, flush=True)
            out.write(l + "\n")


if __name__ == "__main__":
    main()
