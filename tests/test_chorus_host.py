"""The per-bus chorus, the host side: s2r_chorus_reference — the rule restated in plain C++ — held against a numpy
float32 model of the rule written here (np_chorus, which tests/test_gpu_chorus.py holds the device against too) and against a scalar,
frame-by-frame restatement, and the range checks of the entry points, which answer without a device.  Every comparison is on bits
(helpers.assert_bits_equal_finite)."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_reverb_host import _new_or_skip

F = np.float32
NAN = float("nan")
INF = float("inf")
M32 = 0xFFFFFFFF
VOICES = [1, 2, 3, 8]
SHAPES = [(1.0, 0.0), (1.0, 1.0), (1.5, 0.25), (96.0, 48.0), (255.5, 0.75), (1.0, 4094.0), (4095.0, 0.0), (2000.3, 2094.6)]
INCS = [0, 1, 89478, 1 << 31, M32]
PAST = float(np.nextafter(F(4095.0), F(INF)))                    # one ulp past S2R_CHORUS_MAX_DELAY
# (voices, base, depth, dry, wet): one value out of its range or not finite
BAD = [(9, 1.0, 0.0, 1.0, 1.0), (M32, 1.0, 0.0, 1.0, 1.0), (1, 0.99999994, 0.0, 1.0, 1.0), (1, 0.0, 8.0, 1.0, 1.0), (1, -2.0, 8.0, 1.0, 1.0),
       (1, 1.0, -1e-9, 1.0, 1.0), (1, NAN, 0.0, 1.0, 1.0), (1, 1.0, NAN, 1.0, 1.0), (1, INF, 0.0, 1.0, 1.0), (1, 1.0, INF, 1.0, 1.0),
       (1, PAST, 0.0, 1.0, 1.0), (1, 4095.0, 0.00025, 1.0, 1.0), (1, 1.0, PAST - 1.0, 1.0, 1.0), (8, 4096.0, 0.0, 1.0, 1.0),
       (1, 1.0, 0.0, 1.5, 1.0), (1, 1.0, 0.0, 1.0, 1.0000001), (1, 1.0, 0.0, -0.25, 1.0), (1, 1.0, 0.0, 1.0, -1e-9), (1, 1.0, 0.0, NAN, 1.0),
       (1, 1.0, 0.0, 1.0, NAN), (1, 1.0, 0.0, INF, 0.0)]
# in range, the edges among them: 4095 + 0.0001 rounds to 4095 in binary32, and the sum is what the rule looks at
GOOD = [(1, 1.0, 0.0, 0.0, 0.0), (8, 4095.0, 0.0, 1.0, 1.0), (8, 1.0, 4094.0, 1.0, 1.0), (3, 4095.0, 0.0001, 0.5, 0.25), (2, 1.5, 0.25, 1.0, 0.5)]


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def history_frames(base, depth):
    """H = floor(fl(base + depth)) + 1, the sum in binary32"""
    return int(np.floor(F(base) + F(depth))) + 1


def np_chorus(V, base, depth, phase_inc, spread, dry, wet, x, history, phase):
    """The rule in numpy float32, both channels, all frames of the call at once: the phase in uint64 masked to 32 bits, and every
    operation of the rule ONE float32 array operation over the call's frames.  x [N, 2], history [H, 2] (oldest first; left as it is)
    -> (y [N, 2], the history after the call [H, 2], the phase after the call)."""
    x = np.ascontiguousarray(x, dtype=F)
    hist = np.ascontiguousarray(history, dtype=F)
    N, H = x.shape[0], history_frames(base, depth)
    assert x.shape == (N, 2) and hist.shape == (H, 2) and 1 <= V <= 8
    s = np.concatenate([hist, x], axis=0)                        # x[-H .. N): x[j] sits at row H + j
    n = np.arange(N, dtype=np.uint64)
    y = np.empty((N, 2), dtype=F)
    with np.errstate(under="ignore"):
        for c in range(2):
            acc = None
            for v in range(V):
                off = (((v << 32) // V) + c * int(spread)) & M32
                p = (np.uint64(int(phase) & M32) + np.uint64(off) + np.uint64(int(phase_inc) & M32) * n) & np.uint64(M32)
                q = p >> np.uint64(8)
                h = np.where(q < np.uint64(1 << 23), q, np.uint64(1 << 24) - q)
                m = h.astype(F) * F(2.0 ** -23)
                dm = F(depth) * m
                d = F(base) + dm
                i = d.astype(np.int64)
                f = d - i.astype(F)
                assert d.dtype == F and f.dtype == F and (i >= 1).all() and (i + 1 <= H).all() and (f >= 0).all() and (f < 1).all()
                j = H + n.astype(np.int64) - i
                a, bb = s[j, c], s[j - 1, c]
                e = bb - a
                g = f * e
                tap = a + g
                acc = tap if acc is None else acc + tap
            dx = F(dry) * x[:, c]
            wa = F(wet) * acc
            y[:, c] = dx + wa
    assert y.dtype == F
    return y, s[N:].copy(), (int(phase) + int(phase_inc) * N) & M32


def scalar_chorus(V, base, depth, phase_inc, spread, dry, wet, x, history, phase, offs=None):
    """the rule once more, frame by frame and voice by voice in numpy float32 scalars and Python integers: (y, history, phase)"""
    H = history_frames(base, depth)
    s = [tuple(r) for r in np.ascontiguousarray(history, dtype=F)] + [tuple(r) for r in np.ascontiguousarray(x, dtype=F)]
    y = np.empty((x.shape[0], 2), dtype=F)
    with np.errstate(under="ignore"):
        for n in range(x.shape[0]):
            for c in range(2):
                acc = None
                for v in range(V):
                    off = ((offs[v] if offs else (v << 32) // V) + c * spread) & M32
                    p = (phase + off + phase_inc * n) & M32
                    q = p >> 8
                    h = q if q < (1 << 23) else (1 << 24) - q
                    m = F(h) * F(2.0 ** -23)
                    d = F(F(base) + F(F(depth) * m))
                    i = int(d)
                    f = F(d - F(i))
                    a, bb = s[H + n - i][c], s[H + n - i - 1][c]
                    e = F(bb - a)
                    g = F(f * e)
                    tap = F(a + g)
                    acc = tap if acc is None else F(acc + tap)
                y[n, c] = F(F(F(dry) * s[H + n][c]) + F(F(wet) * acc))
    return y, np.array(s[len(s) - H:], dtype=F).reshape(H, 2), (phase + phase_inc * x.shape[0]) & M32


def _p(a):
    return a.ctypes.data_as(s2s._f32p)


def _signal(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2)) * scale).astype(F)


@pytest.mark.parametrize("V", VOICES)
def test_reference_is_the_numpy_model(V):
    """s2r_chorus_reference against np_chorus over every shape and rate, in calls of 1, 17 and 1000 frames with the state carried
    from call to call: output, history and phase"""
    for k, (base, depth) in enumerate(SHAPES):
        H = history_frames(base, depth)
        for inc in INCS:
            hist, ph = _signal(H, 31 * k + V, 0.5), (0x9E3779B9 * (k + 1)) & M32
            mh, mp = hist, ph
            for N in (1, 17, 1000):
                x = _signal(N, 1000 * k + 10 * V + N + (inc & 0xff))
                want, mh, mp = np_chorus(V, base, depth, inc, 0x40000000, 0.5, 0.25, x, mh, mp)
                got, hist, ph = s2.chorus_reference(V, base, depth, inc, 0x40000000, 0.5, 0.25, x, hist, ph)
                what = "V %d, base %g, depth %g, phase_inc %d, %d frames" % (V, base, depth, inc, N)
                assert_bits_equal_finite(got, want, what)
                assert_bits_equal_finite(hist, mh, what + ": the history")
                assert ph == mp, what


@pytest.mark.parametrize("V", VOICES)
def test_reference_is_the_scalar_restatement(V):
    for k, (base, depth) in enumerate([(1.0, 0.0), (1.5, 0.25), (96.0, 48.0), (2000.3, 2094.6)]):
        H = history_frames(base, depth)
        x, hist = _signal(40, 5 * k + V), _signal(H, 77 + k)
        for inc, spread, ph in ((89478 * 500, 0x40000000, 0), (M32, 7, 0xFFFFFF00), (1 << 31, 0, 1 << 30)):
            want = scalar_chorus(V, base, depth, inc, spread, 0.75, 0.5, x, hist, ph)
            got = s2.chorus_reference(V, base, depth, inc, spread, 0.75, 0.5, x, hist, ph)
            model = np_chorus(V, base, depth, inc, spread, 0.75, 0.5, x, hist, ph)
            for g, w, m, name in zip(got[:2], want[:2], model[:2], ("output", "history")):
                assert_bits_equal_finite(g, w, "V %d, base %g: %s against the scalar restatement" % (V, base, name))
                assert_bits_equal_finite(m, w, "V %d, base %g: %s, the numpy model against the scalar restatement" % (V, base, name))
            assert got[2] == want[2] == model[2]


@pytest.mark.parametrize("base,depth", [(1.0, 0.0), (1.5, 0.25), (96.0, 48.0), (1.0, 4094.0)])
def test_two_calls_are_one(base, depth):
    """calls of a and b frames equal one call of a + b, in output, history and phase"""
    H = history_frames(base, depth)
    for a, b in ((1, 1), (H - 1, 2), (H, H + 1), (7, 3 * H), (0, 3), (3, 0)):
        x, hist = _signal(a + b, 31 * H + a), _signal(H, 5 * H + b)
        args = (3, base, depth, 0x01234567, 0x80000001, 0.5, 1.0)
        whole, whole_hist, whole_ph = s2.chorus_reference(*args, x, hist, 0xFEDCBA98)
        first, mid, mid_ph = s2.chorus_reference(*args, x[:a], hist, 0xFEDCBA98)
        second, end, end_ph = s2.chorus_reference(*args, x[a:], mid, mid_ph)
        assert_bits_equal_finite(np.concatenate([first, second], axis=0), whole, "H %d: %d + %d frames" % (H, a, b))
        assert_bits_equal_finite(end, whole_hist, "H %d: %d + %d frames, the history" % (H, a, b))
        assert end_ph == whole_ph == (0xFEDCBA98 + 0x01234567 * (a + b)) & M32


@pytest.mark.parametrize("base,depth", [(1.0, 1.0), (1.5, 0.25), (1.0, 4094.0), (2000.3, 2094.6)])
def test_the_top_of_the_triangle_reads_the_oldest_frame(base, depth):
    """phase 2^31 and phase_inc 0: m == 1 at every frame, so d = fl(base + depth), i = floor(d) = H - 1, and frame 0 reads a = x[-(H - 1)]
    and bb = x[-H], the oldest frame of the history"""
    H = history_frames(base, depth)
    d = F(base) + F(depth)
    f = F(d - F(H - 1))
    hist = np.zeros((H, 2), dtype=F)
    hist[0] = (3.0, -5.0)                                        # the oldest frame alone
    out, new, ph = s2.chorus_reference(1, base, depth, 0, 0, 0.0, 1.0, np.zeros((2, 2), dtype=F), hist, 1 << 31)
    assert ph == 1 << 31
    assert np.array_equal(out[0], np.array([f * F(3.0), f * F(-5.0)], dtype=F))
    hist[0], hist[1] = (0.0, 0.0), (3.0, -5.0)                   # the frame in front of it: a = hist[1], bb = hist[0] = 0
    out, _, _ = s2.chorus_reference(1, base, depth, 0, 0, 0.0, 1.0, np.zeros((2, 2), dtype=F), hist, 1 << 31)
    want_a = np.array([F(3.0) + f * F(-3.0), F(-5.0) + f * F(5.0)], dtype=F)
    assert np.array_equal(out[0], want_a)
    assert np.array_equal(out[1], np.array([f * F(3.0), f * F(-5.0)], dtype=F))     # one frame on it is bb
    assert_bits_equal_finite(out, np_chorus(1, base, depth, 0, 0, 0.0, 1.0, np.zeros((2, 2), dtype=F), hist, 1 << 31)[0], "the model agrees")


def test_denormal_products_survive():
    """a history of 2^-120 .. 2^-119 under a wet of 2^-10 and f = 0.5: f * e and wet * acc are denormals, none is flushed"""
    base, depth, N = 2.5, 0.0, 6
    H = history_frames(base, depth)
    hist = (np.ldexp(1.0 + np.arange(2 * H) / (4.0 * H), -120)).astype(F).reshape(H, 2)
    x = (np.ldexp(1.0 + np.arange(2 * N) / (3.0 * N), -121)).astype(F).reshape(N, 2)
    wet = float(np.ldexp(1.0, -10))
    want, want_hist, _ = np_chorus(2, base, depth, 12345, 0, 0.0, wet, x, hist, 0)
    tiny = float(np.finfo(F).tiny)
    mag = np.abs(want.astype(np.float64))
    assert (mag > 0.0).all() and (mag < tiny).all()
    got, got_hist, _ = s2.chorus_reference(2, base, depth, 12345, 0, 0.0, wet, x, hist, 0)
    assert_bits_equal_finite(got, want, "denormal products")
    assert_bits_equal_finite(got_hist, want_hist, "denormal products: the history")
    # nothing is skipped for f == 0 or a zero coefficient: -0.0 through a + 0 * (bb - a) comes out +0.0, and dry * x keeps its sign
    x = np.full((3, 2), -0.0, dtype=F)
    out, _, _ = s2.chorus_reference(1, 1.0, 0.0, 0, 0, 0.0, 1.0, x, np.full((2, 2), -0.0, dtype=F), 0)
    assert not bits(out).any(), "(+0.0 * -0.0 = -0.0) + (1 * (-0.0 + 0 * 0 = +0.0)) is +0.0"
    out, _, _ = s2.chorus_reference(1, 1.0, 0.0, 0, 0, 1.0, 0.0, x, np.full((2, 2), -0.0, dtype=F), 0)
    assert not bits(out).any(), "(1 * -0.0) + (0 * +0.0) is +0.0"


def test_three_voices_sit_a_third_of_a_turn_apart():
    """V = 3: the offsets are floor(v * 2^32 / 3) — 0, 0x55555555, 0xAAAAAAAA.  2 * 2^32 / 3 ends in .67, so rounding to nearest would
    give 0xAAAAAAAB; with a phase of 0x55 that one unit carries into p >> 8 and moves the tap of voice 2 by depth * 2^-23 frames: the
    reference equals the restatement with the floors and differs from the one with the rounded offset"""
    offs = [(v << 32) // 3 for v in range(3)]
    assert offs == [0, 0x55555555, 0xAAAAAAAA]
    base, depth = 1.0, 4094.0
    H = history_frames(base, depth)
    x, hist = _signal(8, 3), _signal(H, 4)
    got = s2.chorus_reference(3, base, depth, 0, 0, 0.0, 1.0, x, hist, 0x55)
    want = scalar_chorus(3, base, depth, 0, 0, 0.0, 1.0, x, hist, 0x55)
    other = scalar_chorus(3, base, depth, 0, 0, 0.0, 1.0, x, hist, 0x55, offs=[0, 0x55555555, 0xAAAAAAAB])
    assert_bits_equal_finite(got[0], want[0], "V = 3")
    assert (bits(got[0]) != bits(other[0])).all(), "the rounded offset is another chorus"


def test_history_frames():
    L = s2.load_library()
    assert s2.CHORUS_MAX_VOICES == 8 and s2.CHORUS_MAX_DELAY == 4095.0
    for base, depth in SHAPES + [(g[1], g[2]) for g in GOOD] + [(1.0, 0.99999994), (2.9999998, 0.0), (1.0, 1.9999999), (4094.0, 0.9998)]:
        assert L.s2r_chorus_history_frames(base, depth) == history_frames(base, depth) == s2.chorus_history_frames(base, depth), (base, depth)
        assert 2 <= history_frames(base, depth) <= 4096
    assert history_frames(1.0, 0.0) == 2 and history_frames(4095.0, 0.0) == 4096 and history_frames(4095.0, 0.0001) == 4096
    for _, base, depth, dry, wet in BAD:                         # (the entries that are bad for their delay range)
        if dry == 1.0 and wet == 1.0 and _ <= 8:
            assert L.s2r_chorus_history_frames(base, depth) == 0, (base, depth)
    assert L.s2r_chorus_history_frames(PAST, 0.0) == 0 and L.s2r_chorus_history_frames(0.5, 1.0) == 0
    assert s2.chorus_rate(1.0, 48000) == 89478 and s2.chorus_rate(0.0, 48000) == 0 and s2.chorus_rate(24000.0, 48000) == 1 << 31
    assert s2.Synth.chorus_rate(1.0, 48000) == 89478 and s2.Synth.chorus_history_frames(1.5, 0.25) == 2


def test_range_errors_without_a_handle():
    """every entry looks at the values before it looks at the handle, so the range checks answer without a device, and a refused
    reference call leaves history, phase and output alone; S2R_ERR_INVALID is what no handle gets for values in range"""
    L = s2.load_library()
    for v, base, depth, dry, wet in BAD:
        assert L.s2r_set_bus_chorus(None, 0, v, base, depth, 1, 2, dry, wet) == s2s.S2R_ERR_PATCH_RANGE, (v, base, depth, dry, wet)
    for v, base, depth, dry, wet in GOOD:
        assert L.s2r_set_bus_chorus(None, 7, v, base, depth, M32, M32, dry, wet) == s2s.S2R_ERR_INVALID, (v, base, depth, dry, wet)
        assert L.s2r_set_bus_chorus_mix(None, 7, dry, wet) == s2s.S2R_ERR_INVALID
    for dry, wet in [(b[3], b[4]) for b in BAD if (b[3], b[4]) != (1.0, 1.0)]:
        assert L.s2r_set_bus_chorus_mix(None, 0, dry, wet) == s2s.S2R_ERR_PATCH_RANGE, (dry, wet)
    assert L.s2r_set_bus_chorus(None, 0, 0, NAN, NAN, 0, 0, NAN, NAN) == s2s.S2R_ERR_INVALID     # voices 0 removes: the rest is not looked at
    for bus in (8, 255, M32):
        assert L.s2r_set_bus_chorus(None, bus, 1, 1.0, 0.0, 0, 0, 1.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_chorus(None, bus, 0, 0.0, 0.0, 0, 0, 0.0, 0.0) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_chorus_mix(None, bus, 1.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_chorus_rate(None, bus, 1, 1) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_get_bus_chorus(None, bus, None, None, None, None, None, None, None) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_chorus_rate(None, 0, 1, 1) == s2s.S2R_ERR_INVALID
    n = C.c_uint32()
    assert L.s2r_get_bus_chorus(None, 0, C.byref(n), None, None, None, None, None, None) == s2s.S2R_ERR_INVALID
    buf = np.zeros(8, dtype=F)
    assert L.s2r_get_bus_chorus_state(None, 0, _p(buf), 8, C.byref(n)) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_chorus_state(None, 0, _p(buf), 8, 0) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_chorus_state(None, 8, _p(buf), 8, C.byref(n)) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_chorus_state(None, 8, _p(buf), 8, 0) == s2s.S2R_ERR_PATCH_RANGE
    # the reference: a refusal changes neither the history, nor the phase, nor the output
    x, hist, out = _signal(3, 1), _signal(4, 2), np.full((3, 2), 9.0, dtype=F)
    keep, ph = hist.copy(), C.c_uint32(77)
    for v, base, depth, dry, wet in BAD + [(0, 1.0, 0.0, 1.0, 1.0)]:
        assert L.s2r_chorus_reference(v, base, depth, 1, 2, dry, wet, _p(x), 3, _p(hist), C.byref(ph), _p(out)) == s2s.S2R_ERR_PATCH_RANGE, (v, base, depth, dry, wet)
    assert L.s2r_chorus_reference(1, 2.5, 1.0, 1, 2, 1.0, 1.0, _p(x), 3, None, C.byref(ph), _p(out)) == s2s.S2R_ERR_INVALID
    assert L.s2r_chorus_reference(1, 2.5, 1.0, 1, 2, 1.0, 1.0, _p(x), 3, _p(hist), None, _p(out)) == s2s.S2R_ERR_INVALID
    assert L.s2r_chorus_reference(1, 2.5, 1.0, 1, 2, 1.0, 1.0, None, 3, _p(hist), C.byref(ph), _p(out)) == s2s.S2R_ERR_INVALID
    assert np.array_equal(bits(hist), bits(keep)) and (out == 9.0).all() and ph.value == 77
    assert L.s2r_chorus_reference(1, 2.5, 1.0, 1, 2, 1.0, 1.0, None, 0, _p(hist), C.byref(ph), None) == s2s.S2R_OK     # no frames: no x, and out may be null
    assert np.array_equal(bits(hist), bits(keep)) and ph.value == 77
    h = keep.copy()
    assert L.s2r_chorus_reference(2, 2.5, 1.0, 5, 2, 1.0, 1.0, _p(x), 3, _p(h), C.byref(ph), None) == s2s.S2R_OK
    assert ph.value == 92
    assert_bits_equal_finite(h, np_chorus(2, 2.5, 1.0, 5, 2, 1.0, 1.0, x, keep, 77)[1], "out_lr NULL: the state moves on all the same")
    with pytest.raises(ValueError):
        s2.chorus_reference(1, 2.5, 1.0, 0, 0, 1.0, 1.0, x, hist[:3], 0)
    with pytest.raises(s2.S2rError) as err:
        s2.chorus_reference(9, 2.5, 1.0, 0, 0, 1.0, 1.0, x, hist, 0)
    assert err.value.status == s2s.S2R_ERR_PATCH_RANGE
    assert s2.Synth.chorus_reference(1, 2.5, 1.0, 0, 0, 1.0, 1.0, x, hist, 0)[0].shape == (3, 2)
    syn = _new_or_skip(num_voices=8, max_frames=64)              # with a device the rest runs on a real handle
    if syn is not None:
        check_ranges(syn)


def test_abi_version_stays():
    assert s2.load_library().s2r_abi_version() == 4


NONE = (0, 0.0, 0.0, 0, 0, 0.0, 0.0)


def check_ranges(syn):
    """the setters' range checks on a live handle, and the mix, rate and state entries on a bus without a chorus (also called by
    tests/test_gpu_chorus.py)"""
    L, h = syn.L, syn.h
    assert all(syn.get_bus_chorus(b) == NONE for b in range(s2.MAX_BUSES))       # a fresh handle: no chorus anywhere
    for v, base, depth, dry, wet in BAD:
        assert L.s2r_set_bus_chorus(h, 0, v, base, depth, 1, 2, dry, wet) == s2s.S2R_ERR_PATCH_RANGE, (v, base, depth, dry, wet)
    assert L.s2r_set_bus_chorus(h, 8, 1, 1.0, 0.0, 0, 0, 1.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
    assert syn.get_bus_chorus(0) == NONE                         # a refused call changes nothing
    buf, ph = np.zeros(16, dtype=F), C.c_uint32(5)
    assert L.s2r_set_bus_chorus_mix(h, 0, 1.0, 1.0) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_chorus_rate(h, 0, 1, 1) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_chorus_state(h, 0, _p(buf), 16, C.byref(ph)) == s2s.S2R_ERR_INVALID and ph.value == 5
    assert L.s2r_set_bus_chorus_state(h, 0, _p(buf), 8, 0) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_chorus_state(h, 8, _p(buf), 16, None) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_chorus_state(h, 8, _p(buf), 16, 0) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_chorus(h, 8, None, None, None, None, None, None, None) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_chorus(h, 0, None, None, None, None, None, None, None) == s2s.S2R_OK     # any pointer may be null
    syn.clear_bus_chorus(3)                                      # removing what is not there is no error
    syn.set_bus_chorus(3, 3, 2.5, 1.0, 89478, 0x40000000, 0.25, 1.0)
    assert syn.get_bus_chorus(3) == (3, 2.5, 1.0, 89478, 0x40000000, 0.25, 1.0) and syn.get_bus_chorus(0)[0] == 0
    hist, phase = syn.bus_chorus_state(3)
    assert hist.shape == (4, 2) and not bits(hist).any() and phase == 0     # +0.0 everywhere and phase 0 right after the chorus is set
    for count in (0, 6, 7, 9, 16):
        assert L.s2r_set_bus_chorus_state(h, 3, _p(buf), count, 1) == s2s.S2R_ERR_INVALID, count
    assert L.s2r_set_bus_chorus_state(h, 3, None, 8, 1) == s2s.S2R_ERR_INVALID
    for cap in (0, 7):
        assert L.s2r_get_bus_chorus_state(h, 3, _p(buf), cap, C.byref(ph)) == s2s.S2R_ERR_INVALID, cap
    assert L.s2r_get_bus_chorus_state(h, 3, None, 8, C.byref(ph)) == s2s.S2R_ERR_INVALID
    assert syn.bus_chorus_state(3)[1] == 0                       # the refused setters left the phase alone
    assert L.s2r_get_bus_chorus_state(h, 3, _p(buf), 16, None) == s2s.S2R_OK      # a larger buffer will do, and the phase may be null
    new = np.arange(8, dtype=F).reshape(4, 2) - F(3.5)
    syn.set_bus_chorus_state(3, new, 0xDEADBEEF)
    got, phase = syn.bus_chorus_state(3)
    assert np.array_equal(bits(got), bits(new)) and phase == 0xDEADBEEF
    for v, base, depth, dry, wet in BAD:
        assert L.s2r_set_bus_chorus(h, 3, v, base, depth, 1, 2, dry, wet) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_chorus_mix(h, 3, 1.5, 0.0) == s2s.S2R_ERR_PATCH_RANGE and L.s2r_set_bus_chorus_mix(h, 3, 0.0, NAN) == s2s.S2R_ERR_PATCH_RANGE
    assert syn.get_bus_chorus(3) == (3, 2.5, 1.0, 89478, 0x40000000, 0.25, 1.0)
    syn.set_bus_chorus_mix(3, 1.0, 0.0)
    syn.set_bus_chorus_rate(3, M32, 1)
    assert syn.get_bus_chorus(3) == (3, 2.5, 1.0, M32, 1, 1.0, 0.0)
    got, phase = syn.bus_chorus_state(3)
    assert np.array_equal(bits(got), bits(new)) and phase == 0xDEADBEEF      # the mix and the rate keep the state
    syn.set_bus_chorus(3, 1, 4.0, 1.5, 0, 0, 1.0, 1.0)           # setting it again zeroes it
    got, phase = syn.bus_chorus_state(3)
    assert got.shape == (6, 2) and not bits(got).any() and phase == 0
    syn.clear_bus_chorus(3)
    assert syn.get_bus_chorus(3) == NONE
    assert L.s2r_get_bus_chorus_state(h, 3, _p(buf), 16, None) == s2s.S2R_ERR_INVALID
