"""Times the master sample-rate converter on a pool of 4096 voices (48 kHz, eight programs of the default patch on
eight buses; the stage's kernel does not depend on the pool), master only (the stems never cross to the host), all cases on ONE handle in
one run:

    147/160 at T 48, 1/2 at T 64, 2/1 at T 32, 8 buses, 1024 frames per fill      48 -> 44.1 kHz, halving and doubling
    147/160 at T 48, 8 buses, 16 frames and 8192 frames per fill                  a short call and a long one
    no stage, 8 buses, 1024 frames                                                the master fill as it was, for the comparison with the parent

Every case is measured in one block of N + 2 fills (the first two dropped).  Device time of the master and resampler kernels (HIP events
around each, s2r_set_timing) and host wall time per call, medians of N with min .. max.

    python tools/resampler_time.py [--out profiles/r25/master_resampler.txt]

A/B against a library kept from another build (S2R_AB_LIB=<path>, see synth2_amd/build.py): --ab LABEL appends one line per case the
loaded library has — the serial build (S2R_RESAMPLER_SERIAL=1 python -m synth2_amd.build), or a library kept from the parent commit,
which is timed on the fill without the stage alone — to --out instead of replacing it; run the libraries in turn, one process each.

No pass threshold."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import synth2_amd as s2
from synth2_amd import build as s2build

V = int(os.environ.get("V", 4096))
SR = 48000
N = int(os.environ.get("N", 20))          # timed fills of each case
BANK = 8
MAX_FRAMES = 8192
CASES = [(147, 160, 48, 1024), (1, 2, 64, 1024), (2, 1, 32, 1024), (147, 160, 48, 16), (147, 160, 48, 8192)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r25", "master_resampler.txt"))
    ap.add_argument("--ab", default=None, help="a label for this library: append one line per case to --out")
    a = ap.parse_args()
    L = s2.load_library()
    has_stage = hasattr(L, "s2r_debug_resampler_ms")
    timers = [t for t in ("master", "resampler") if hasattr(L, "s2r_debug_%s_ms" % t)]
    for t in timers:
        getattr(L, "s2r_debug_%s_ms" % t).restype = C.c_float
        getattr(L, "s2r_debug_%s_ms" % t).argtypes = [C.c_void_p]
    s = s2.Synth(V, max_frames=MAX_FRAMES)
    s.set_patch_bank([s2.default_patch()] * BANK)
    for p in range(BANK):
        s.set_program_pan(p, -1.0 + 2.0 * p / (BANK - 1), 0.5)
        s.set_program_mix(p, 1.0 - p / 16.0, p / 8.0, p)
    for v in range(V):
        if v % (V // 64) == 0:
            s.program_change((v * 64 // V) % BANK)
        s.note_on(36 + v % 61, 0.5)
    s.set_master_fader(1.0 / 1024.0)      # (4096 voices at once: the master stays below full scale)
    s.snap_master()
    s.sample_master(1024, SR, BANK, stems=False)
    s.set_timing(True)
    cases = [None] + (CASES if has_stage else [])
    lines = []
    for case in cases:
        frames = 1024 if case is None else case[3]
        if case is not None:
            rl, rm, rt, _ = case
            s.set_master_resampler(rl, rm, s2.resampler_design(rl, rm, rt))
        wall, dev = [], {t: [] for t in timers}
        for i in range(N + 2):
            t0 = time.perf_counter()
            out = s.sample_master(frames, SR, BANK, stems=False)[0]
            wall.append((time.perf_counter() - t0) * 1e3)
            for t in timers:
                dev[t].append(float(getattr(L, "s2r_debug_%s_ms" % t)(s.h)))
        assert np.isfinite(out).all() and np.abs(out).max() > 0.0
        if case is not None:                  # (a sanity check, not the parity test: the frames made, and a level that follows the master's)
            got = s.resampled(BANK)
            total = (N + 2) * frames * rl
            assert s.resampler_state()[1] == (-total) % rm and abs(got.shape[0] - frames * rl / rm) <= 1.0
            assert np.isfinite(got).all() and 0.25 * np.abs(out).max() < np.abs(got).max() < 4.0 * np.abs(out).max(), "the outputs follow the master"
        w = np.array(wall[2:])
        parts = []
        for t in timers:
            m = np.array(dev[t][2:])
            parts.append("%s %7.4f ms (%.4f .. %.4f)" % (t, np.median(m), m.min(), m.max()))
        name = "%3d/%3d, T %3d, %d buses, %4d frames" % (rl, rm, rt, BANK, frames) if case is not None else "no stage, %d buses, %4d frames" % (BANK, frames)
        lines.append((name, "   ".join(parts) + "   host wall per call %7.3f ms (%.3f .. %.3f)" % (np.median(w), w.min(), w.max())))
    block = s.block_voices
    s.close()
    build = L.s2r_build_id().decode()
    if a.ab is not None:
        text = ["  A/B %-8s (build %s)  %s  %s" % (a.ab, build, name, row) for name, row in lines]
    else:
        text = ["tools/resampler_time.py: %d voices (block %d), %d Hz, %d programs of the default patch on %d buses, master only, Kaiser tables (beta 10, rolloff "
                "0.9); kernel times by HIP events; medians of %d fills (min .. max); build %s" % (V, block, SR, BANK, BANK, N, build)]
        text += ["  %s  %s" % (name, row) for name, row in lines]
        res = os.path.join(s2build.OBJ_DIR, "s2r_resampler.resources.txt")
        if os.path.exists(res):
            text.append("compiler resource usage (s2r_resampler.hip, -Rpass-analysis=kernel-resource-usage):")
            for l in open(res):
                text.append("  " + l.strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.ab is not None else "w") as out:
        for l in text:
            print(l, flush=True)
            out.write(l + "\n")


if __name__ == "__main__":
    main()
