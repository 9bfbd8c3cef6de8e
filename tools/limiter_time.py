"""Times the master limiter on the C3 shape of tools/master_time.py (65536 voices, 48 kHz, 1024 frames, eight
programs of the default patch on eight buses, bench.py's C3 events moved to frame 0), eight buses per call, master only (the stems
never cross to the host), all on ONE handle in one run:

    s2r_fill_master, no limiter            before a limiter was ever set
    s2r_fill_master, limiter (L, H)        for (48, 0), (240, 480) and (1024, 4096), the ceiling at half the peak of the unlimited
                                           master, so the limiter is at work

Every kind is measured in one block of N + 2 fills (the first two dropped).  Device time of the master kernel and of the limiter
kernel (HIP events around each, s2r_set_timing) and host wall time per call, medians of N.

    python tools/limiter_time.py [--out profiles/r11/limiter.txt]

A/B against a library kept from another build (S2R_AB_LIB=<path>, see synth2_amd/build.py): --ab LABEL appends one line per kind the
loaded library has — a library without s2r_set_master_limiter is timed on the master fill alone — to --out instead of replacing
it; run the two libraries in turn, one process each, three rounds, and compare this build's no-limiter median with the other
library's min .. max.

--true-peak times the true-peak detector beside the sample-peak rule: the three pairs with each detector, on the same
handle, into profiles/r26/limiter_true_peak.txt.  The comparison form of its kernel (S2R_LIMITER_TP_NAIVE=1 python -m synth2_amd.build,
then S2R_AB_LIB=synth2_amd/libs2r_limitertpnaive.so) goes beside it with --true-peak --ab naive.

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
PAIRS = [(48, 0), (240, 480), (1024, 4096)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab", default=None, help="a label for this library: append one line per kind to --out")
    ap.add_argument("--true-peak", action="store_true", help="the three pairs with the true-peak detector too (default --out: profiles/r26/limiter_true_peak.txt)")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", *(("r26", "limiter_true_peak.txt") if a.true_peak else ("r11", "limiter.txt")))
    L = s2.load_library()
    has_limiter = hasattr(L, "s2r_debug_limiter_ms")
    for name in ("s2r_debug_master_ms",) + (("s2r_debug_limiter_ms",) if has_limiter else ()):
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
    kinds = [(None, "s2r_fill_master, no limiter         ")]
    if has_limiter:
        kinds += [(p, "s2r_fill_master, limiter (%4d, %4d)" % p) for p in PAIRS]
    if a.true_peak:                                       # a kind of three: the true-peak detector
        kinds += [(p + (True,), "s2r_fill_master, true-peak (%4d, %4d)" % p) for p in PAIRS]
    wall, mst, lim, gain = ({kd[0]: [] for kd in kinds} for _ in range(4))
    k = period + 2
    peak = 0.0
    for kind, _ in kinds:
        if kind is not None:
            s.set_master_limiter(peak / 2.0, *kind[:2], **({"true_peak": True} if len(kind) == 3 else {}))
        for i in range(N + 2):
            s.note_events(events(k))
            k += 1
            t0 = time.perf_counter()
            out = s.sample_master(FR, SR, BANK, stems=False)[0]
            wall[kind].append((time.perf_counter() - t0) * 1e3)
            mst[kind].append(float(L.s2r_debug_master_ms(s.h)))
            lim[kind].append(float(L.s2r_debug_limiter_ms(s.h)) if kind is not None else 0.0)
            if kind is None:
                peak = max(peak, float(np.abs(out).max()))
            else:
                gain[kind].append(s.limiter_meters()[0])
                assert np.abs(out).max() <= np.float32(peak / 2.0)
        assert np.isfinite(out).all() and np.abs(out).max() > 0.0
        if kind is not None:
            assert min(gain[kind]) < 1.0                  # the limiter was at work
    block = s.block_voices
    s.close()

    def row(kind):
        m, f, w = (np.array(x[kind][2:]) for x in (mst, lim, wall))
        return "master kernel %7.4f ms (%.4f .. %.4f)   limiter kernel %7.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms (%.3f .. %.3f)" % (
            np.median(m), m.min(), m.max(), np.median(f), f.min(), f.max(), np.median(w), w.min(), w.max())

    build = L.s2r_build_id().decode()
    if a.ab is not None:
        lines = ["  A/B %-8s (build %s)  %s %s" % (a.ab, build, name, row(kind)) for kind, name in kinds]
    else:
        lines = ["tools/limiter_time.py: %d voices (block %d), %d frames per fill, %d Hz, %d programs of the default patch on %d buses, %d buses "
                 "per call, master only, C3 events at frame 0; ceiling %.4g (half the unlimited peak); medians of %d fills (min .. max); build %s"
                 % (V, block, FR, SR, BANK, BANK, BANK, peak / 2.0, N, build)]
        for kind, name in kinds:
            lines.append("  " + name + " " + row(kind))
        w = {kind: np.median(wall[kind][2:]) for kind, _ in kinds}
        lines.append("  host wall per call against the fill without a limiter: " + ", ".join("(%d, %d) %+.3f ms" % (p + (w[p] - w[None],)) for p in PAIRS)
                     + "; smallest min_gain seen: " + ", ".join("%.4f" % min(gain[p]) for p in PAIRS))
        if a.true_peak:
            lines.append("  the true-peak detector against the sample-peak rule, limiter kernel: " + ", ".join(
                "(%d, %d) %+.4f ms" % (p + (np.median(lim[p + (True,)][2:]) - np.median(lim[p][2:]),)) for p in PAIRS)
                + "; smallest min_gain seen: " + ", ".join("%.4f" % min(gain[p + (True,)]) for p in PAIRS))
        for src, more in (("s2r_limiter", "2 * (256 + 2 L + H) floats"),) + ((("s2r_limiter_tp", "2 * (256 + 2 L + H) floats and 256 + 2 L + H + 16 frames"),) if a.true_peak else ()):
            res = os.path.join(s2build.OBJ_DIR, src + ".resources.txt")
            if os.path.exists(res):
                lines.append("compiler resource usage (%s.hip, -Rpass-analysis=kernel-resource-usage; plus %s of dynamic LDS):" % (src, more))
                for l in open(res):
                    lines.append("  " + l.strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.ab is not None else "w") as out:
        for l in lines:
            print(l, flush=True)
            out.write(l + "\n")


if __name__ == "__main__":
    main()
