"""Times s2r_fill_buses without and with per-bus convolution reverbs on the C3 shape of tools/bus_time.py /
send_time.py (65536 voices, 48 kHz, 1024 frames, eight programs of the default patch on eight buses, bench.py's C3 events moved to
frame 0: one render launch and one mixdown per fill), eight buses per call, all on ONE handle in one run:

    untouched        bus fills before any reverb was set: the kernels and arguments of a build without reverbs
    1 bus,  K taps   a reverb of K taps (a stereo response) on bus 0
    8 buses, K taps  the same on every bus                                     K = 4800, 48000 and 65536

The untouched fills come first; after them every kind is measured in one block of N + 2 fills (the first two dropped).  Device time
of the mixdown's kernel pair and of the reverb's three kernels (HIP events around each, s2r_set_timing) and host wall time per call,
medians of N.  The reverb's multiplies and adds are counted as executed — the last segment is padded to 256 taps, a tile to 1024
frames — and held against the fp32 VALU ceiling without fma: half of 157.3 TFLOP/s, which counts an fma as two.

    python tools/reverb_time.py [--out profiles/r09/bus_reverb.txt]

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
TAPS = [4800, 48000, 65536]
TILE = 1024                               # frames per workgroup of the convolve kernel (s2r_fx.hip)
CEILING = 157.3e12 / 2.0                  # fp32 VALU without fma, FLOP/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r09", "bus_reverb.txt"))
    a = ap.parse_args()
    L = s2.load_library()
    for name in ("s2r_debug_bus_mix_ms", "s2r_debug_bus_fx_ms"):
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
    kinds = [("untouched", 0, 0)] + [("reverb", nb, K) for K in TAPS for nb in (1, BANK)]
    wall = {kd: [] for kd in kinds}
    mix = {kd: [] for kd in kinds}
    fx = {kd: [] for kd in kinds}
    k = [period + 2]

    def fill(kd):
        s.note_events(events(k[0]))
        k[0] += 1
        t0 = time.perf_counter()
        out = s.sample_buses(FR, SR, BANK)
        wall[kd].append((time.perf_counter() - t0) * 1e3)
        mix[kd].append(float(L.s2r_debug_bus_mix_ms(s.h)))
        fx[kd].append(float(L.s2r_debug_bus_fx_ms(s.h)))
        return out

    for i in range(N + 2):
        fill(kinds[0])
    irng = np.random.RandomState(2)
    for kd in kinds[1:]:
        _, nb, K = kd
        ir = (irng.standard_normal((K, 2)) * np.exp(-np.arange(K) / (K / 6.0))[:, None] * 0.05).astype(np.float32)
        for b in range(BANK):
            if b < nb:
                s.set_bus_reverb(b, ir, 0.5, 0.5)
            else:
                s.clear_bus_reverb(b)
        for i in range(N + 2):
            out = fill(kd)
        assert np.isfinite(out).all() and s.get_bus_reverb(0)[0] == K and s.get_bus_reverb(BANK - 1)[0] == (K if nb == BANK else 0)
    block = s.block_voices
    s.close()
    lines = ["tools/reverb_time.py: %d voices (block %d), %d frames per fill, %d Hz, %d programs of the default patch on %d buses, %d buses "
             "per call, C3 events at frame 0; medians of %d fills (min .. max); build %s" % (V, block, FR, SR, BANK, BANK, BANK, N, L.s2r_build_id().decode())]

    def row(kd):
        m, f, w = (np.array(x[kd][2:]) for x in (mix, fx, wall))
        return m, f, w, "mixdown kernels %7.4f ms (%.4f .. %.4f)   reverb kernels %8.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms (%.3f .. %.3f)" % (
            np.median(m), m.min(), m.max(), np.median(f), f.min(), f.max(), np.median(w), w.min(), w.max())

    m0, _, w0, text = row(kinds[0])
    lines.append("  untouched (no reverb ever set)   " + text)
    lines.append("  untouched: run-to-run spread of the mixdown kernels (max - min) / median = %.1f %%, of the wall time %.1f %%" % (
        100.0 * (m0.max() - m0.min()) / np.median(m0), 100.0 * (w0.max() - w0.min()) / np.median(w0)))
    for kd in kinds[1:]:
        _, nb, K = kd
        m, f, w, text = row(kd)
        lines.append("  reverb on %d bus%s K = %5d      %s" % (nb, " ,  " if nb == 1 else "es,", K, text))
        n_seg = (K + s2.IR_SEGMENT - 1) // s2.IR_SEGMENT
        flop = 2.0 * nb * 2 * n_seg * s2.IR_SEGMENT * ((FR + TILE - 1) // TILE) * TILE
        rate = flop / (np.median(f) * 1e-3)
        lines.append("      executed %.3e multiplies and adds: %.2f TFLOP/s = %.1f %% of the fp32 ceiling without fma (%.2f TFLOP/s); "
                     "reverb kernels / this visit's untouched 8-bus mixdown = %.2f; wall - untouched wall = %+.3f ms" % (
                         flop, rate * 1e-12, 100.0 * rate / CEILING, CEILING * 1e-12, np.median(f) / np.median(m0), np.median(w) - np.median(w0)))
    res = os.path.join(s2build.OBJ_DIR, "s2r_fx.resources.txt")
    if os.path.exists(res):
        lines.append("compiler resource usage (s2r_fx.hip, -Rpass-analysis=kernel-resource-usage):")
        for l in open(res):
            lines.append("  " + l.strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for l in lines:
            print(l, flush=True)
            out.write(l + "\n")


if __name__ == "__main__":
    main()
