"""Times the per-bus room reverb on the C3 shape of tools/dyn_time.py (65536 voices, 48 kHz, eight programs of the default
patch on eight buses, bench.py's C3 events moved to frame 0), eight buses per call, all on ONE handle in one run:

    untouched              bus fills before any room was set: the kernels and arguments of a build without it
    1 bus                  a room on bus 0 (the other seven buses are copied by the same launch)
    8 buses                a room on every bus: eight workgroups, one per bus
    reverb                 beside them, the convolution reverb with a response of 65 536 taps on bus 0 and on all eight, rooms off

each in calls of 1024 and 64 frames.  The untouched fills come first; after them every kind is measured in one block of N + 2 fills
(the first two dropped).  The rooms are s2r_room_design's at 48 kHz (delays of 245 to 1785 frames), feedback 0.84, damp 0.2.  Device
time of the mixdown's kernels and of the stage's kernel (HIP events around each, s2r_set_timing) and host wall time per call, medians
of N with min .. max.  The stage is serial in time, so its figure of merit is time per frame: the kernel's median over the call's
frames is printed in ns.

    timeout -k 10 600 python tools/room_time.py [--out profiles/r19/bus_room.txt]

--form LABEL names the kernel form the loaded library holds (default: tiled); with --append the rows are added to --out instead of
replacing it: the obvious form, one thread per comb doing its own loads, recursion and stores, is built by S2R_ROOM_SERIAL=1 into
libs2r_roomserial.so (synth2_amd/build.py) and timed by S2R_AB_LIB=synth2_amd/libs2r_roomserial.so ... --form serial --append (the
reverb is not timed again then).

A/B against a library kept from another build (S2R_AB_LIB=<path>): --ab LABEL times the plain fills of a handle WITHOUT a room —
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
SHAPES = [1, BANK]                        # buses with a room
CALLS = [1024, 64]
AB_KINDS = [("buses", "s2r_fill_buses            "), ("stems", "s2r_fill_master, stems    "), ("only", "s2r_fill_master, no stems ")]
LEVELS = (0.84, 0.2, 0.5, 0.015, 1.0, 0.5, 0.125)      # feedback, damp, g, gain, dry, wet, cross
TAPS = 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r19", "bus_room.txt"))
    ap.add_argument("--ab", default=None, help="a label for this library: time the plain fills and append one line per kind to --out")
    ap.add_argument("--form", default="tiled", help="the kernel form the loaded library holds")
    ap.add_argument("--append", action="store_true", help="add the rows to --out instead of replacing it")
    a = ap.parse_args()
    L = s2.load_library()
    has_room = hasattr(L, "s2r_debug_bus_room_ms")
    for name in ("s2r_debug_bus_mix_ms", "s2r_debug_master_ms", "s2r_debug_bus_fx_ms") + (("s2r_debug_bus_room_ms",) if has_room else ()):
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

    def room_ms():
        return float(L.s2r_debug_bus_room_ms(s.h)) if has_room else 0.0

    if a.ab is not None:                                  # the plain fills of a handle without a room
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
                rmt[kind].append(room_ms())
            assert np.isfinite(out).all() and np.abs(out).max() > 0.0 and not np.array(rmt[kind]).any()
        s.close()
        lines = []
        for kind, name in AB_KINDS:
            m, f, w = (np.array(x[kind][2:]) for x in (mix, mst, wall))
            lines.append("  A/B %-8s (build %s)  %s mixdown kernels %7.4f ms (%.4f .. %.4f)   master kernel %7.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms "
                         "(%.3f .. %.3f)" % (a.ab, build, name, np.median(m), m.min(), m.max(), np.median(f), f.min(), f.max(), np.median(w), w.min(), w.max()))
    else:
        cd, ad, spread = s2.room_design(float(SR))
        kinds = [("untouched", 0, fr) for fr in CALLS] + [("room", nb, fr) for nb in SHAPES for fr in CALLS]
        if a.form == "tiled":
            kinds += [("reverb", nb, fr) for nb in SHAPES for fr in CALLS]
        ir = (np.random.RandomState(2).standard_normal(TAPS) * np.exp(-np.arange(TAPS) / (TAPS / 6.0)) * 0.01).astype(np.float32)
        wall, mix, stg = ({kd: [] for kd in kinds} for _ in range(3))
        for kd in kinds:
            what, nb, fr = kd
            for b in range(BANK):                         # (set afresh for every kind: the state starts from silence)
                s.clear_bus_room(b)
                s.clear_bus_reverb(b)
                if b < nb and what == "room":
                    s.set_bus_room(b, cd, ad, spread, *LEVELS)
                if b < nb and what == "reverb":
                    s.set_bus_reverb(b, ir, 1.0, 0.5)
            for i in range(N + 2):
                s.note_events(events(k[0]))
                k[0] += 1
                t0 = time.perf_counter()
                out = s.sample_buses(fr, SR, BANK)
                wall[kd].append((time.perf_counter() - t0) * 1e3)
                mix[kd].append(float(L.s2r_debug_bus_mix_ms(s.h)))
                stg[kd].append(float(L.s2r_debug_bus_fx_ms(s.h)) if what == "reverb" else room_ms())
            assert np.isfinite(out).all() and (s.get_bus_room(0) is not None) == (what == "room")
            assert (np.array(stg[kd]) > 0.0).all() if nb else (np.array(stg[kd]) == 0.0).all()
        s.close()
        lines = ["tools/room_time.py, kernel form: %s.  %d voices (block %d), %d Hz, %d programs of the default patch on %d buses, %d buses per call, max_frames %d, "
                 "C3 events at frame 0; combs %s, allpasses %s, spread %d; feedback %g, damp %g, g %g, gain %g, dry %g, wet %g, cross %g; the reverb beside "
                 "it: %d taps; medians of %d fills (min .. max); build %s"
                 % ((a.form, V, block, SR, BANK, BANK, BANK, MAXFR, list(map(int, cd)), list(map(int, ad)), spread) + LEVELS + (TAPS, N, build))]
        base = {}
        for kd in kinds:
            what, nb, fr = kd
            m, f, w = (np.array(x[kd][2:]) for x in (mix, stg, wall))
            text = "mixdown kernels %7.4f ms (%.4f .. %.4f)   %s %7.4f ms (%.4f .. %.4f)   host wall per call %7.3f ms (%.3f .. %.3f)" % (
                np.median(m), m.min(), m.max(), "reverb kernels" if what == "reverb" else "room kernel   ", np.median(f), f.min(), f.max(), np.median(w), w.min(), w.max())
            if not nb:
                base[fr] = (np.median(m), np.median(w))
                lines.append("  untouched (no room ever set)        %5d frames   %s" % (fr, text))
                continue
            lines.append("  %-9s %d bus%s            %5d frames   %s" % (a.form if what == "room" else "reverb", nb, "  " if nb == 1 else "es", fr, text))
            lines.append("      %.1f ns per frame; stage / this run's untouched mixdown of %d frames = %.3f; wall - untouched wall = %+.3f ms"
                         % (np.median(f) * 1e6 / fr, fr, np.median(f) / base[fr][0], np.median(w) - base[fr][1]))
        res = os.path.join(s2build.OBJ_DIR, "s2r_room.resources.txt")
        if os.path.exists(res) and not os.environ.get("S2R_AB_LIB"):
            lines.append("compiler resource usage (s2r_room.hip, -Rpass-analysis=kernel-resource-usage):")
            for l in open(res):
                lines.append("  " + l.strip())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if (a.ab is not None or a.append) else "w") as out:
        for l in lines:
            print(l, flush=True)
            out.write(l + "\n")


if __name__ == "__main__":
    main()
