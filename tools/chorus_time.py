"""Times the per-bus chorus on the C3 shape of tools/delay_time.py / master_time.py (65536 voices, 48 kHz, eight
programs of the default patch on eight buses, bench.py's C3 events moved to frame 0: one render launch and one mixdown per rows
slice), eight buses per call, all on ONE handle in one run:

    untouched               bus fills before any chorus was set: the kernels and arguments of a build without choruses
    1 bus,   V voices, H    a chorus of V voices and a history of H frames on bus 0
    8 buses, V voices, H    the same on every bus                        V = 1 and 8; H = 2, 145 and 4096

each in calls of 16, 1024 and max_frames (MAXFR, 8192) frames.  The untouched fills come first; after them every kind is measured in
one block of N + 2 fills (the first two dropped).  Device time of the mixdown's kernels and of the chorus kernel (HIP events around
each, s2r_set_timing) and host wall time per call, medians of N with min .. max.  The LFO runs at 1 Hz with the right channel a
quarter turn ahead.  The bytes the chorus kernel asks for are counted from the shapes — per frame of a bus with a chorus 8 bytes of
x in, 8 of y out and 2 * 2 * V taps of 4 bytes, which neighbouring frames share in cache; 16 bytes per frame of its line (old history
in, new out); 16 bytes per frame of a bus it only copies — and held against its time.

    timeout -k 10 900 python tools/chorus_time.py [--out profiles/r15/bus_chorus.txt]

A/B against a library kept from another build (S2R_AB_LIB=<path>, see synth2_amd/build.py): --ab LABEL times the plain fills of a handle
WITHOUT a chorus — s2r_fill_buses, s2r_fill_master with and without stems, 1024 frames — and appends one line per kind to --out
instead of replacing it; run the two libraries in turn, one process each, three rounds, and compare this build's median of medians
with the other library's min .. max (the protocol of profiles/r12/post_chain.txt).

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
VOICES = [1, 8]
SHAPES = [(2, 1.5, 0.25), (145, 96.5, 48.0), (4096, 2000.5, 2094.5)]     # (H, base, depth)
CALLS = [16, 1024, MAXFR]
AB_KINDS = [("buses", "s2r_fill_buses            "), ("stems", "s2r_fill_master, stems    "), ("only", "s2r_fill_master, no stems ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r15", "bus_chorus.txt"))
    ap.add_argument("--ab", default=None, help="a label for this library: time the plain fills and append one line per kind to --out")
    a = ap.parse_args()
    L = s2.load_library()
    has_chorus = hasattr(L, "s2r_debug_bus_chorus_ms")
    for name in ("s2r_debug_bus_mix_ms", "s2r_debug_master_ms") + (("s2r_debug_bus_chorus_ms",) if has_chorus else ()):
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

    def chorus_ms():
        return float(L.s2r_debug_bus_chorus_ms(s.h)) if has_chorus else 0.0

    if a.ab is not None:                                  # the plain fills of a handle without a chorus
        wall, mix, mst, cho = ({kd[0]: [] for kd in AB_KINDS} for _ in range(4))
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
                cho[kind].append(chorus_ms())
            assert np.isfinite(out).all() and np.abs(out).max() > 0.0 and not np.array(cho[kind]).any()
        s.close()
        lines = []
        for kind, name in AB_KINDS:
            m, f, w = (np.array(x[kind][2:]) for x in (mix, mst, wall))
            lines.append("  A/B %-8s (build %s)  %s mixdown kernels %7.4f ms (%.4f .. %.4f)   master kernel %7.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms "
                         "(%.3f .. %.3f)" % (a.ab, build, name, np.median(m), m.min(), m.max(), np.median(f), f.min(), f.max(), np.median(w), w.min(), w.max()))
    else:
        kinds = [("untouched", 0, 0, 0, fr) for fr in CALLS] + [("chorus", nb, nv, sh, fr) for nv in VOICES for sh in SHAPES for fr in CALLS for nb in (1, BANK)]
        wall, mix, cho = ({kd: [] for kd in kinds} for _ in range(3))
        inc, spread = s2.chorus_rate(1.0, SR), 1 << 30
        for kd in kinds:
            _, nb, nv, sh, fr = kd
            if nv:                                        # (set afresh for every kind: history and phase start from zero)
                for b in range(BANK):
                    if b < nb:
                        s.set_bus_chorus(b, nv, sh[1], sh[2], inc, spread, 0.5, 0.5 / nv)
                    else:
                        s.clear_bus_chorus(b)
            for i in range(N + 2):
                s.note_events(events(k[0]))
                k[0] += 1
                t0 = time.perf_counter()
                out = s.sample_buses(fr, SR, BANK)
                wall[kd].append((time.perf_counter() - t0) * 1e3)
                mix[kd].append(float(L.s2r_debug_bus_mix_ms(s.h)))
                cho[kd].append(chorus_ms())
            assert np.isfinite(out).all() and s.get_bus_chorus(0)[0] == nv and s.get_bus_chorus(BANK - 1)[0] == (nv if nb == BANK else 0)
            assert (np.array(cho[kd]) > 0.0).all() if nv else (np.array(cho[kd]) == 0.0).all()
        s.close()
        lines = ["tools/chorus_time.py: %d voices (block %d), %d Hz, %d programs of the default patch on %d buses, %d buses per call, max_frames %d, "
                 "C3 events at frame 0; medians of %d fills (min .. max); build %s" % (V, block, SR, BANK, BANK, BANK, MAXFR, N, build)]
        base = {}
        for kd in kinds:
            _, nb, nv, sh, fr = kd
            m, f, w = (np.array(x[kd][2:]) for x in (mix, cho, wall))
            text = "mixdown kernels %7.4f ms (%.4f .. %.4f)   chorus kernel %7.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms (%.3f .. %.3f)" % (
                np.median(m), m.min(), m.max(), np.median(f), f.min(), f.max(), np.median(w), w.min(), w.max())
            if not nv:
                base[fr] = (np.median(m), np.median(w))
                lines.append("  untouched (no chorus ever set)           %5d frames   %s" % (fr, text))
                continue
            lines.append("  chorus on %d bus%s V = %d, H = %4d, %5d frames   %s" % (nb, " ,  " if nb == 1 else "es,", nv, sh[0], fr, text))
            asked = 16.0 * BANK * fr + nb * (16.0 * sh[0] + 16.0 * nv * fr)
            lines.append("      %.3e bytes asked for by the chorus kernel: %.1f GB/s; chorus kernel / this run's untouched mixdown of %d frames = %.3f; "
                         "wall - untouched wall = %+.3f ms" % (asked, asked / (np.median(f) * 1e-3) * 1e-9, fr, np.median(f) / base[fr][0], np.median(w) - base[fr][1]))
        res = os.path.join(s2build.OBJ_DIR, "s2r_chorus.resources.txt")
        if os.path.exists(res):
            lines.append("compiler resource usage (s2r_chorus.hip, -Rpass-analysis=kernel-resource-usage):")
            for l in open(res):
                lines.append("  " + l.strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.ab is not None else "w") as out:
        for l in lines:
            print(l, flush=True)
            out.write(l + "\n")


if __name__ == "__main__":
    main()
