"""Times the master section on the C3 shape of tools/reverb_time.py / bus_time.py (65536 voices, 48 kHz, 1024 frames,
eight programs of the default patch on eight buses, bench.py's C3 events moved to frame 0: one render launch and one mixdown per
fill), eight buses per call, all on ONE handle in one run:

    s2r_fill_buses              the eight stems through pinned memory, before any master fill was made
    s2r_fill_master, stems      the master and the eight stems
    s2r_fill_master, no stems   the master alone: the stems never cross to the host

Every kind is measured in one block of N + 2 fills (the first two dropped).  Device time of the mixdown's kernel pair and of the
master kernel (HIP events around each, s2r_set_timing) and host wall time per call, medians of N.  Returns and master fader are on
their way in every master fill (the kernel has one form: a pair that stays has a step of +0).

    python tools/master_time.py [--out profiles/r10/master.txt]

A/B against a library kept from another build (S2R_AB_LIB=<path>, see synth2_amd/build.py): --ab LABEL appends one line per kind the
loaded library has — a library without s2r_fill_master is timed on s2r_fill_buses alone — to --out instead of replacing it; run
the two libraries in turn, one process each, three rounds, and compare the master-only median with the other library's min .. max.

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
KINDS = [("buses", "s2r_fill_buses            "), ("stems", "s2r_fill_master, stems    "), ("only", "s2r_fill_master, no stems ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r10", "master.txt"))
    ap.add_argument("--ab", default=None, help="a label for this library: append one line per kind to --out")
    a = ap.parse_args()
    L = s2.load_library()
    has_master = hasattr(L, "s2r_fill_master")
    for name in ("s2r_debug_bus_mix_ms",) + (("s2r_debug_master_ms",) if has_master else ()):
        getattr(L, name).restype = C.c_float
        getattr(L, name).argtypes = [C.c_void_p]
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
    kinds = [kd for kd in KINDS if has_master or kd[0] == "buses"]
    wall = {kd[0]: [] for kd in kinds}
    mix = {kd[0]: [] for kd in kinds}
    mst = {kd[0]: [] for kd in kinds}
    k = period + 2
    for kind, _ in kinds:
        for i in range(N + 2):
            s.note_events(events(k))
            k += 1
            if kind != "buses":
                for b in range(BANK):
                    s.set_bus_return(b, 0.5 + 0.5 * ((i + b) & 1))
                s.set_master_fader(0.5 + 0.25 * (i & 1))
            t0 = time.perf_counter()
            if kind == "buses":
                out = s.sample_buses(FR, SR, BANK)
            else:
                out = s.sample_master(FR, SR, BANK, stems=(kind == "stems"))[0]
            wall[kind].append((time.perf_counter() - t0) * 1e3)
            mix[kind].append(float(L.s2r_debug_bus_mix_ms(s.h)))
            mst[kind].append(float(L.s2r_debug_master_ms(s.h)) if kind != "buses" else 0.0)
        assert np.isfinite(out).all() and np.abs(out).max() > 0.0
    block = s.block_voices
    s.close()

    def row(kind):
        m, f, w = (np.array(x[kind][2:]) for x in (mix, mst, wall))
        return "mixdown kernels %7.4f ms (%.4f .. %.4f)   master kernel %7.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms (%.3f .. %.3f)" % (
            np.median(m), m.min(), m.max(), np.median(f), f.min(), f.max(), np.median(w), w.min(), w.max())

    build = L.s2r_build_id().decode()
    if a.ab is not None:
        lines = ["  A/B %-8s (build %s)  %s %s" % (a.ab, build, name, row(kind)) for kind, name in kinds]
    else:
        lines = ["tools/master_time.py: %d voices (block %d), %d frames per fill, %d Hz, %d programs of the default patch on %d buses, %d buses "
                 "per call, C3 events at frame 0; medians of %d fills (min .. max); build %s" % (V, block, FR, SR, BANK, BANK, BANK, N, build)]
        for kind, name in kinds:
            lines.append("  " + name + row(kind))
        w = {kind: np.median(wall[kind][2:]) for kind, _ in kinds}
        if has_master:
            lines.append("  host wall per call against s2r_fill_buses: with stems %+.3f ms, master only %+.3f ms; pinned floats read back per call: "
                         "%d (bus fill), %d (with stems), %d (master only)" % (w["stems"] - w["buses"], w["only"] - w["buses"],
                                                                            2 * FR * BANK, 2 * FR * (BANK + 1), 2 * FR))
        res = os.path.join(s2build.OBJ_DIR, "s2r_master.resources.txt")
        if os.path.exists(res):
            lines.append("compiler resource usage (s2r_master.hip, -Rpass-analysis=kernel-resource-usage):")
            for l in open(res):
                lines.append("  " + l.strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.ab is not None else "w") as out:
        for l in lines:
            print(l, flush=True)
            out.write(l + "\n")


if __name__ == "__main__":
    main()
