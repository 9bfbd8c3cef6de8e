"""Times s2r_fill_panned on the C3 shape (65536 voices, 48 kHz, 1024 frames, the default patch, bench.py's C3 events) against
s2r_fill_stereo on the same handle, and the panned mixdown's kernels against a device-to-device copy of the rows buffer.

    python tools/pan_time.py [--out profiles/r05/pan_mix.txt] [--slices default,256,64]

One handle per rows-buffer slice length (S2R_PAN_SLICE frames; `default`: the library's own choice, s2r.h), each after one
untimed period of the schedule.  Two event forms per handle: the schedule as bench.py submits it (note-offs at their
16-frame boundaries: the panned fill is split at every distinct event frame) and the same events moved to frame 0 (one
render launch and one mixdown per slice — the form the kernel figures are taken from).  No pass threshold."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import bench
import synth2_amd as s2

V = int(os.environ.get("V", 65536))
FR = int(os.environ.get("FR", 1024))
SR = 48000
N = int(os.environ.get("N", 24))          # timed fills of each kind


def copy_rate(nbytes):
    """(bytes per second, milliseconds) of a device-to-device hipMemcpyAsync of `nbytes`, timed with HIP events on the null
    stream, best of ten — through the HIP runtime libs2r.so itself is linked against"""
    hip = C.CDLL("libamdhip64.so")
    P = C.c_void_p

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: hipError %d" % (what, rc))
    a, b, e0, e1 = P(), P(), P(), P()
    ok(hip.hipMalloc(C.byref(a), C.c_size_t(nbytes)), "hipMalloc")
    ok(hip.hipMalloc(C.byref(b), C.c_size_t(nbytes)), "hipMalloc")
    ok(hip.hipMemset(a, 1, C.c_size_t(nbytes)), "hipMemset")
    ok(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    best = None
    for k in range(13):
        ok(hip.hipEventRecord(e0, None), "hipEventRecord")
        ok(hip.hipMemcpyAsync(b, a, C.c_size_t(nbytes), 3, None), "hipMemcpyAsync")       # 3: hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(e1, None), "hipEventRecord")
        ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
        if k >= 3:
            best = ms.value if best is None else min(best, ms.value)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    hip.hipFree(a); hip.hipFree(b)
    return nbytes / (best * 1e-3), best


def run(slice_arg, out):
    if slice_arg == "default":
        os.environ.pop("S2R_PAN_SLICE", None)
    else:
        os.environ["S2R_PAN_SLICE"] = slice_arg
    L = s2.load_library()
    L.s2r_debug_pan_mix_ms.restype = C.c_float
    L.s2r_debug_pan_mix_ms.argtypes = [C.c_void_p]
    L.s2r_debug_pan_slice.restype = C.c_uint32
    L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    s = s2.Synth(V, max_frames=FR)
    s.set_program_pan(0, 0.0, 1.0)                        # the keyboard spread over the stereo field
    period = bench.PERIOD if V >= bench.PERIOD else 1
    cyc = bench.make_c3_events(V, period, FR)
    mono = np.empty(FR, dtype=np.float32)
    for k in range(period + 2):                           # one life of every voice: the stage mix the bench is timed on
        s.note_events(cyc[k % period])
        s.sample(mono, SR)
    s.set_timing(True)
    res = {}
    k = period + 2
    for form in ("timed", "frame0"):
        t_pan, t_st, t_kern = [], [], []
        for i in range(2 * N):
            ev = cyc[k % period].copy()
            k += 1
            if form == "frame0":
                ev["frame"] = 0
            s.note_events(ev)
            t0 = time.perf_counter()
            if i % 2 == 0:
                s.sample_panned(FR, SR)
                t_pan.append((time.perf_counter() - t0) * 1e3)
                t_kern.append(float(L.s2r_debug_pan_mix_ms(s.h)))
            else:
                s.sample_stereo(FR, SR)
                t_st.append((time.perf_counter() - t0) * 1e3)
        res[form] = (np.median(t_pan[2:]), np.median(t_st[2:]), np.median(t_kern[2:]))
    slice_frames = int(L.s2r_debug_pan_slice(s.h))
    rows_bytes = V * slice_frames * 4
    s.close()
    rate, copy_ms = copy_rate(rows_bytes)
    moved = V * FR * 4 + 2 * FR * 4                       # rows read plus output written, per fill
    kern_ms = res["frame0"][2]
    lines = ["slice %s: %d frames per slice, rows buffer %.1f MiB (%d voices)" % (slice_arg, slice_frames, rows_bytes / 2.0 ** 20, V)]
    for form in ("timed", "frame0"):
        p, st, kk = res[form]
        lines.append("  events %-6s  s2r_fill_panned %8.3f ms   s2r_fill_stereo %7.3f ms   pan-mix kernels %7.3f ms per fill" % (form, p, st, kk))
    lines.append("  pan-mix kernels (frame0 form): %.3f ms for %.1f MiB -> %.1f GB/s (rows read + output written)" % (
        kern_ms, moved / 2.0 ** 20, moved / (kern_ms * 1e-3) / 1e9))
    lines.append("  device-to-device copy of the rows buffer: %.3f ms -> %.1f GB/s copied (%.1f GB/s read + written)" % (
        copy_ms, rate / 1e9, 2 * rate / 1e9))
    for l in lines:
        print(l, flush=True)
        out.write(l + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r05", "pan_mix.txt"))
    ap.add_argument("--slices", default="default,256,64")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write("tools/pan_time.py: %d voices, %d frames per fill, %d Hz, default patch, key spread 1.0, C3 events; medians of %d fills; build %s\n" % (
            V, FR, SR, N - 2, s2.load_library().s2r_build_id().decode()))
        for sl in a.slices.split(","):
            run(sl.strip(), out)


if __name__ == "__main__":
    main()
