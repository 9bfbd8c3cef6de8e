"""Times s2r_fill_buses at 1, 2, 4 and 8 buses on the C3 shape (65536 voices, 48 kHz, 1024 frames, the default patch, bench.py's
C3 events moved to frame 0: one render launch and one mixdown per fill) beside s2r_fill_panned on the SAME handle in the same
run: device time of the mixdown's kernel pair (HIP events around it) and host wall time per call.

    python tools/bus_time.py [--out profiles/r06/bus_mix.txt]

The programs' settings spread the voices over all eight buses with several levels and velocity sensitivities.  The note also
carries the register / LDS / scratch figures of every instantiation: the compiler's resource-usage remarks kept by the build
(synth2_amd/build.py) and the dynamic LDS the launcher asks for.  No pass threshold."""
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


def lds_bytes(block_voices, n_buses, wide=True):
    """what s2r_launch_bus_mix asks for: (lanes, bytes)"""
    nb = 1 if n_buses <= 1 else 2 if n_buses <= 2 else 4 if n_buses <= 4 else 8
    w, lanes, n_grp = (4 if wide else 1), 32, block_voices // 16
    while lanes > 1 and n_grp * 2 * nb * lanes * w * 4 > (32 << 10):
        lanes >>= 1
    return lanes, n_grp * 2 * nb * lanes * w * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r06", "bus_mix.txt"))
    a = ap.parse_args()
    L = s2.load_library()
    for name in ("s2r_debug_pan_mix_ms", "s2r_debug_bus_mix_ms"):
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
        """period k's events at frame 0, a program change in front of every note_on, velocities in [0, 1]"""
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
    gains, buses = s.voice_mix()
    s.set_timing(True)
    kinds = [("panned", 0), ("buses", 1), ("buses", 2), ("buses", 4), ("buses", 8)]
    wall = {kd: [] for kd in kinds}
    dev = {kd: [] for kd in kinds}
    k = period + 2
    for i in range(N + 2):                                # interleaved: every kind sees the same drift of the box
        for kd in kinds:
            s.note_events(events(k))
            k += 1
            t0 = time.perf_counter()
            if kd[0] == "panned":
                s.sample_panned(FR, SR)
                wall[kd].append((time.perf_counter() - t0) * 1e3)
                dev[kd].append(float(L.s2r_debug_pan_mix_ms(s.h)))
            else:
                s.sample_buses(FR, SR, kd[1])
                wall[kd].append((time.perf_counter() - t0) * 1e3)
                dev[kd].append(float(L.s2r_debug_bus_mix_ms(s.h)))
    block = s.block_voices
    s.close()
    rows_bytes = V * FR * 4
    lines = ["tools/bus_time.py: %d voices (block %d), %d frames per fill, %d Hz, %d programs of the default patch on %d buses, C3 events at frame 0; "
             "medians of %d interleaved fills (min .. max); build %s" % (V, block, FR, SR, BANK, BANK, N, L.s2r_build_id().decode()),
             "voices per bus: %s; distinct voice gains: %d" % (np.bincount(buses, minlength=8).tolist(), len(np.unique(gains))),
             "rows buffer read per fill: %.1f MiB" % (rows_bytes / 2.0 ** 20)]
    for kd in kinds:
        d, w = np.array(dev[kd][2:]), np.array(wall[kd][2:])
        nb = max(kd[1], 1)
        moved = rows_bytes + 2 * FR * 4 * nb
        lines.append("  %-6s %s  mixdown kernels %7.4f ms (%.4f .. %.4f) -> %7.1f GB/s over the rows   host wall per call %7.3f ms (%.3f .. %.3f)" % (
            kd[0], ("%d bus%s" % (kd[1], "" if kd[1] == 1 else "es")).ljust(7) if kd[1] else "       ",
            np.median(d), d.min(), d.max(), moved / (np.median(d) * 1e-3) / 1e9, np.median(w), w.min(), w.max()))
    lines.append("launch geometry at block %d, 16-byte loads: " % block + "; ".join(
        "%d buses: %d lanes x 4 frames, %d KiB LDS" % ((nb,) + (lambda t: (t[0], t[1] >> 10))(lds_bytes(block, nb))) for nb in (1, 2, 4, 8)))
    res = os.path.join(s2build.OBJ_DIR, "s2r_aux.resources.txt")
    if os.path.exists(res):
        lines.append("compiler resource usage (s2r_aux.hip, -Rpass-analysis=kernel-resource-usage; LDS is dynamic, see above):")
        for l in open(res):
            if "s2r_bus_" in l or "s2r_pan_" in l:
                lines.append("  " + l.strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for l in lines:
            print(l, flush=True)
            out.write(l + "\n")


if __name__ == "__main__":
    main()
