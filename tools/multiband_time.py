"""Times the master multiband compressor on the shape of tools/limiter_time.py (V voices, 48 kHz, FR frames, eight
programs of the default patch on eight buses, bench.py's C3 events moved to frame 0), eight buses per call, master only (the stems
never cross to the host), all on ONE handle in one run:

    s2r_fill_master, no multiband          before the stage was ever set
    s2r_fill_master, multiband B           for B = 1, 2 and 4 bands, splits at 200 / 1500 / 6000 Hz, every band's threshold at half the
                                           band's peak in the unprocessed master, so every gain is at work; the master fader
                                           brings the mix's peak to 0.5 first, for every kind (the curves end at a level of 256)

Every kind is measured in one block of N + 2 fills (the first two dropped).  Device time of the master kernel and of the multiband
kernel (HIP events around each, s2r_set_timing) and host wall time per call, medians of N.

    python tools/multiband_time.py [--out profiles/r27/master_multiband.txt]          (FR=16 and FR=8192 in the environment: other call lengths)

A/B against a library kept from another build (S2R_AB_LIB=<path>, see synth2_amd/build.py): --ab LABEL appends one line per kind the
loaded library has — a library without s2r_set_master_multiband is timed on the master fill alone — to --out instead of replacing it.
The comparison form of the kernel: S2R_MULTIBAND_SERIAL=1 python -m synth2_amd.build, then S2R_AB_LIB=synth2_amd/libs2r_multibandserial.so
with --ab serial; run the two libraries in turn, one process each, in alternating rounds.

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
BANDS = [1, 2, 4]
SPLITS = [200.0, 1500.0, 6000.0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r27", "master_multiband.txt"))
    ap.add_argument("--ab", default=None, help="a label for this library: append one line per kind to --out")
    a = ap.parse_args()
    L = s2.load_library()
    has_stage = hasattr(L, "s2r_debug_multiband_ms")
    for name in ("s2r_debug_master_ms",) + (("s2r_debug_multiband_ms",) if has_stage else ()):
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
    # the mix of V voices is many times full scale, past the curves' top level of 256: the master fader brings its peak to 0.5
    k = period + 2
    peak = 0.0
    for i in range(2):
        s.note_events(events(k))
        k += 1
        peak = max(peak, float(np.abs(s.sample_master(FR, SR, BANK, stems=False)[0]).max()))
    fader = min(1.0, 0.5 / peak)
    s.set_master_fader(fader)
    s.snap_master()
    s.set_timing(True)
    kinds = [(None, "s2r_fill_master, no multiband")] + ([(B, "s2r_fill_master, multiband %d   " % B) for B in BANDS] if has_stage else [])
    wall, mst, mbt, gain = ({kd[0]: [] for kd in kinds} for _ in range(4))
    plain = []
    for kind, _ in kinds:
        if kind is not None:
            B = kind
            coeffs = s2.multiband_design(float(SR), SPLITS[:B - 1]) if B > 1 else None
            x = np.concatenate(plain)
            bands = s2.multiband_reference(coeffs, np.ones((B, s2.DYN_CURVE_POINTS), np.float32), [0.0] * B, [0.0] * B, x, want_bands=True)[3]
            curves = np.stack([s2.dynamics_curve(20.0 * np.log10(max(float(np.abs(bands[j]).max()), 1e-6) / 2.0), 4.0, 6.0, 0.0) for j in range(B)])
            s.set_master_multiband(curves, [float(s2.dynamics_coef(1.0, SR))] * B, [float(s2.dynamics_coef(50.0, SR))] * B, coeffs=coeffs)
        for i in range(N + 2):
            s.note_events(events(k))
            k += 1
            t0 = time.perf_counter()
            out = s.sample_master(FR, SR, BANK, stems=False)[0]
            wall[kind].append((time.perf_counter() - t0) * 1e3)
            mst[kind].append(float(L.s2r_debug_master_ms(s.h)))
            mbt[kind].append(float(L.s2r_debug_multiband_ms(s.h)) if kind is not None else 0.0)
            if kind is None:
                plain.append(out.copy())
            else:
                gain[kind].append(float(s.multiband_meters().min()))
        assert np.isfinite(out).all() and np.abs(out).max() > 0.0
        if kind is not None:
            assert min(gain[kind]) < 1.0                  # the gains were at work
    block = s.block_voices
    s.close()

    def row(kind):
        m, f, w = (np.array(x[kind][2:]) for x in (mst, mbt, wall))
        return "master kernel %7.4f ms (%.4f .. %.4f)   multiband kernel %7.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms (%.3f .. %.3f)" % (
            np.median(m), m.min(), m.max(), np.median(f), f.min(), f.max(), np.median(w), w.min(), w.max())

    build = L.s2r_build_id().decode()
    if a.ab is not None:
        lines = ["  A/B %-8s %5d frames (build %s)  %s %s" % (a.ab, FR, build, name, row(kind)) for kind, name in kinds]
    else:
        lines = ["tools/multiband_time.py: %d voices (block %d), %d frames per fill, %d Hz, %d programs of the default patch on %d buses, %d buses "
                 "per call, master only, C3 events at frame 0, master fader %.4g (a peak of 0.5); splits at 200 / 1500 / 6000 Hz, thresholds at half "
                 "each band's peak; medians of %d fills (min .. max); build %s" % (V, block, FR, SR, BANK, BANK, BANK, fader, N, build)]
        for kind, name in kinds:
            lines.append("  " + name + " " + row(kind))
        w = {kind: np.median(wall[kind][2:]) for kind, _ in kinds}
        lines.append("  host wall per call against the fill without the stage: " + ", ".join("%d bands %+.3f ms" % (B, w[B] - w[None]) for B in BANDS)
                     + "; smallest gain seen: " + ", ".join("%.4f" % min(gain[B]) for B in BANDS))
        res = os.path.join(s2build.OBJ_DIR, "s2r_multiband.resources.txt")
        if os.path.exists(res):
            lines.append("compiler resource usage (s2r_multiband.hip, -Rpass-analysis=kernel-resource-usage):")
            for l in open(res):
                lines.append("  " + l.strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.ab is not None else "w") as out:
        for l in lines:
            print(l, flush=True)
            out.write(l + "\n")


if __name__ == "__main__":
    main()
