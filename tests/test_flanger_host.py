"""The per-bus flanger, the host side: s2r_flanger_reference — the rule restated in plain C++ — held against a numpy
float32 model of the rule written here (np_flanger) and against a scalar, frame-by-frame restatement, against the chorus's reference
where the two rules meet, and the range checks of the entry points, which answer without a device.  Every comparison is on bits
(helpers.assert_bits_equal_finite) but the one that says why it is not."""
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
BLOCK = 32                                                       # no tap is younger than 32 frames: a block of 32 frames is frame-parallel
SHAPES = [(32.0, 0.0), (32.0, 0.5), (32.75, 1.0), (40.0, 24.5), (48.0, 97.0), (100.0, 924.0), (32.0, 4063.0)]
INCS = [0, 1, 89478, 1 << 31, M32]
MIXES = [(0.0, 0.0), (0.7, 0.0), (-0.7, 0.3), (0.0, 1.0), (1.0, 0.0)]
PAST = float(np.nextafter(F(4095.0), F(INF)))                    # one ulp past S2R_FLANGER_MAX_DELAY
OVER = float(np.nextafter(F(0.5), F(INF)))                       # 0.5 + OVER is just past 1, in double
# (base, depth, feedback, cross, dry, wet): one value out of its range or not finite
BAD = [(31.999, 0.0, 0.0, 0.0, 1.0, 1.0), (0.0, 40.0, 0.0, 0.0, 1.0, 1.0), (-32.0, 0.0, 0.0, 0.0, 1.0, 1.0), (1.0, 31.0, 0.0, 0.0, 1.0, 1.0),
       (32.0, -1e-9, 0.0, 0.0, 1.0, 1.0), (NAN, 0.0, 0.0, 0.0, 1.0, 1.0), (32.0, NAN, 0.0, 0.0, 1.0, 1.0), (INF, 0.0, 0.0, 0.0, 1.0, 1.0),
       (32.0, INF, 0.0, 0.0, 1.0, 1.0), (PAST, 0.0, 0.0, 0.0, 1.0, 1.0), (4095.0, 0.00025, 0.0, 0.0, 1.0, 1.0), (32.0, PAST - 32.0, 0.0, 0.0, 1.0, 1.0),
       (4096.0, 0.0, 0.0, 0.0, 1.0, 1.0),
       (32.0, 0.0, 1.0000001, 0.0, 1.0, 1.0), (32.0, 0.0, 0.0, -1.0000001, 1.0, 1.0), (32.0, 0.0, 0.5, OVER, 1.0, 1.0), (32.0, 0.0, -OVER, -0.5, 1.0, 1.0),
       (32.0, 0.0, 1.0, 1e-7, 1.0, 1.0), (32.0, 0.0, NAN, 0.0, 1.0, 1.0), (32.0, 0.0, 0.0, NAN, 1.0, 1.0), (32.0, 0.0, INF, 0.0, 1.0, 1.0),
       (32.0, 0.0, 0.0, 0.0, 1.5, 1.0), (32.0, 0.0, 0.0, 0.0, 1.0, 1.0000001), (32.0, 0.0, 0.0, 0.0, -0.25, 1.0), (32.0, 0.0, 0.0, 0.0, 1.0, -1e-9),
       (32.0, 0.0, 0.0, 0.0, NAN, 1.0), (32.0, 0.0, 0.0, 0.0, 1.0, NAN), (32.0, 0.0, 0.0, 0.0, INF, 0.0)]
# in range, the edges among them: 4095 + 0.0001 rounds to 4095 in binary32, and the sum is what the rule looks at
GOOD = [(32.0, 0.0, 0.0, 0.0, 0.0, 0.0), (4095.0, 0.0, 1.0, 0.0, 1.0, 1.0), (32.0, 4063.0, 0.0, -1.0, 1.0, 1.0), (4095.0, 0.0001, 0.5, 0.5, 0.5, 0.25),
        (32.75, 1.0, -0.5, -0.5, 1.0, 0.5)]


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def history_frames(base, depth):
    """H = floor(fl(base + depth)) + 1, the sum in binary32"""
    return int(np.floor(F(base) + F(depth))) + 1


def np_flanger(base, depth, phase_inc, spread, feedback, cross, dry, wet, x, history, phase):
    """The rule in numpy float32, both channels, walked in blocks of 32 frames: inside a block every frame reads only what earlier blocks
    wrote (i >= 32), so every operation of the rule is ONE float32 array operation over the block's frames; the phase in uint64 masked
    to 32 bits.  x [N, 2], history [H, 2] (oldest first; left as it is) -> (y [N, 2], the history after the call [H, 2], the phase
    after the call)."""
    x = np.ascontiguousarray(x, dtype=F)
    hist = np.ascontiguousarray(history, dtype=F)
    N, H = x.shape[0], history_frames(base, depth)
    assert x.shape == (N, 2) and hist.shape == (H, 2) and 33 <= H <= 4096
    w = np.concatenate([hist, np.zeros((N, 2), dtype=F)], axis=0)    # w[-H .. N): w[j] sits at row H + j
    y = np.empty((N, 2), dtype=F)
    with np.errstate(under="ignore"):
        for n0 in range(0, N, BLOCK):
            n = np.arange(n0, min(n0 + BLOCK, N), dtype=np.uint64)
            tap = []
            for c in range(2):
                p = (np.uint64(int(phase) & M32) + np.uint64((c * int(spread)) & M32) + np.uint64(int(phase_inc) & M32) * n) & np.uint64(M32)
                q = p >> np.uint64(8)
                h = np.where(q < np.uint64(1 << 23), q, np.uint64(1 << 24) - q)
                m = h.astype(F) * F(2.0 ** -23)
                dm = F(depth) * m
                d = F(base) + dm
                i = d.astype(np.int64)
                f = d - i.astype(F)
                assert d.dtype == F and f.dtype == F and (i >= 32).all() and (i + 1 <= H).all() and (f >= 0).all() and (f < 1).all()
                j = H + n.astype(np.int64) - i
                assert (j < H + n0).all()                            # nothing of this block
                a, bb = w[j, c], w[j - 1, c]
                e = bb - a
                g = f * e
                tap.append(a + g)
            for c in range(2):
                xc = x[n0:n0 + len(n), c]
                pf = F(feedback) * tap[c]
                pc = F(cross) * tap[1 - c]
                s = pf + pc
                w[H + n0:H + n0 + len(n), c] = xc + s
                dx = F(dry) * xc
                wt = F(wet) * tap[c]
                y[n0:n0 + len(n), c] = dx + wt
    assert y.dtype == F and w.dtype == F
    return y, w[N:].copy(), (int(phase) + int(phase_inc) * N) & M32


def scalar_flanger(base, depth, phase_inc, spread, feedback, cross, dry, wet, x, history, phase):
    """the rule once more, frame by frame in numpy float32 scalars and Python integers: (y, history, phase)"""
    H = history_frames(base, depth)
    w = [tuple(r) for r in np.ascontiguousarray(history, dtype=F)]
    x = np.ascontiguousarray(x, dtype=F)
    y = np.empty((x.shape[0], 2), dtype=F)
    with np.errstate(under="ignore"):
        for n in range(x.shape[0]):
            tap = []
            for c in range(2):
                p = (phase + c * spread + phase_inc * n) & M32
                q = p >> 8
                h = q if q < (1 << 23) else (1 << 24) - q
                m = F(h) * F(2.0 ** -23)
                d = F(F(base) + F(F(depth) * m))
                i = int(d)
                f = F(d - F(i))
                a, bb = w[H + n - i][c], w[H + n - i - 1][c]
                tap.append(F(a + F(f * F(bb - a))))
            w.append(tuple(F(x[n, c] + F(F(F(feedback) * tap[c]) + F(F(cross) * tap[1 - c]))) for c in range(2)))
            for c in range(2):
                y[n, c] = F(F(F(dry) * x[n, c]) + F(F(wet) * tap[c]))
    return y, np.array(w[len(w) - H:], dtype=F).reshape(H, 2), (phase + phase_inc * x.shape[0]) & M32


def _p(a):
    return a.ctypes.data_as(s2s._f32p)


def _signal(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2)) * scale).astype(F)


@pytest.mark.parametrize("feedback,cross", MIXES)
def test_reference_is_the_numpy_model(feedback, cross):
    """s2r_flanger_reference against np_flanger over every shape and rate, in calls of 1, 17, 32, 33 and 1000 frames with the state
    carried from call to call: output, history and phase"""
    for k, (base, depth) in enumerate(SHAPES):
        H = history_frames(base, depth)
        for inc in INCS:
            hist, ph = _signal(H, 31 * k + 7, 0.5), (0x9E3779B9 * (k + 1)) & M32
            mh, mp = hist, ph
            for N in (1, 17, 32, 33, 1000):
                x = _signal(N, 1000 * k + N + (inc & 0xff), 0.25)
                want, mh, mp = np_flanger(base, depth, inc, 0x40000000, feedback, cross, 0.5, 0.25, x, mh, mp)
                got, hist, ph = s2.flanger_reference(base, depth, inc, 0x40000000, feedback, cross, 0.5, 0.25, x, hist, ph)
                what = "base %g, depth %g, phase_inc %d, feedback %g, cross %g, %d frames" % (base, depth, inc, feedback, cross, N)
                assert_bits_equal_finite(got, want, what)
                assert_bits_equal_finite(hist, mh, what + ": the history")
                assert ph == mp, what


@pytest.mark.parametrize("feedback,cross", MIXES)
def test_reference_is_the_scalar_restatement(feedback, cross):
    for k, (base, depth) in enumerate([(32.0, 0.0), (32.75, 1.0), (40.0, 24.5), (100.0, 924.0)]):
        H = history_frames(base, depth)
        x, hist = _signal(75, 5 * k + 1, 0.25), _signal(H, 77 + k, 0.5)
        for inc, spread, ph in ((89478 * 500, 0x40000000, 0), (M32, 7, 0xFFFFFF00), (1 << 31, 0, 1 << 30)):
            args = (base, depth, inc, spread, feedback, cross, 0.75, 0.5, x, hist, ph)
            want, got, model = scalar_flanger(*args), s2.flanger_reference(*args), np_flanger(*args)
            for g, w, m, name in zip(got[:2], want[:2], model[:2], ("output", "history")):
                assert_bits_equal_finite(g, w, "base %g: %s against the scalar restatement" % (base, name))
                assert_bits_equal_finite(m, w, "base %g: %s, the numpy model against the scalar restatement" % (base, name))
            assert got[2] == want[2] == model[2]


@pytest.mark.parametrize("base,depth", [(32.0, 0.0), (32.75, 1.0), (48.0, 97.0), (32.0, 4063.0)])
def test_two_calls_are_one(base, depth):
    """calls of a and b frames equal one call of a + b, in output, history and phase"""
    H = history_frames(base, depth)
    for a, b in ((1, 1), (H - 1, 2), (H, H + 1), (7, 3 * H), (0, 3), (3, 0)):
        x, hist = _signal(a + b, 31 * H + a, 0.25), _signal(H, 5 * H + b, 0.5)
        args = (base, depth, 0x01234567, 0x80000001, -0.625, 0.375, 0.5, 1.0)
        whole, whole_hist, whole_ph = s2.flanger_reference(*args, x, hist, 0xFEDCBA98)
        first, mid, mid_ph = s2.flanger_reference(*args, x[:a], hist, 0xFEDCBA98)
        second, end, end_ph = s2.flanger_reference(*args, x[a:], mid, mid_ph)
        assert_bits_equal_finite(np.concatenate([first, second], axis=0), whole, "H %d: %d + %d frames" % (H, a, b))
        assert_bits_equal_finite(end, whole_hist, "H %d: %d + %d frames, the history" % (H, a, b))
        assert end_ph == whole_ph == (0xFEDCBA98 + 0x01234567 * (a + b)) & M32


@pytest.mark.parametrize("base,depth", [(32.0, 0.5), (32.75, 1.0), (40.0, 24.5), (100.0, 924.0)])
def test_without_feedback_it_is_a_one_voice_chorus(base, depth):
    """feedback = cross = 0: w = x + ((0 * tap) + (0 * tap)), the line is the input and the tap the chorus's one voice.  As VALUES, not on
    bits: x + (+0.0) turns a -0.0 of the input over, so the flanger's line holds +0.0 where the chorus's history holds -0.0 — equal as
    numbers, and the taps taken from them are too."""
    H = history_frames(base, depth)
    assert H == s2.chorus_history_frames(base, depth)
    x, hist = _signal(300, 3 * H, 0.25), _signal(H, H, 0.5)
    x[5], x[290], x[295, 1] = (-0.0, -0.0), (-0.0, -0.0), -0.0     # (frames 290 and 295 are in the history the call leaves)
    got, gh, gp = s2.flanger_reference(base, depth, 89478 * 64, 0x40000000, 0.0, 0.0, 0.5, 0.75, x, hist, 12345)
    want, wh, wp = s2.chorus_reference(1, base, depth, 89478 * 64, 0x40000000, 0.5, 0.75, x, hist, 12345)
    assert np.array_equal(got, want) and np.array_equal(gh, wh) and gp == wp
    assert bits(wh)[H - 10, 0] == 0x80000000                     # the chorus keeps the input's -0.0 ...
    differ = bits(gh) != bits(wh)                                # ... and where the flanger's line differs from it on bits, both are zeros
    assert not gh[differ].any() and not wh[differ].any()


@pytest.mark.parametrize("D", [32, 33, 100])
def test_an_impulse_comes_back_every_d_frames(D):
    """depth 0, an integer base D, feedback 1, wet 1, dry 0: f == 0, tap[n] = w[n - D], w[n] = x[n] + w[n - D] — an impulse at frame 3
    is heard at 3 + D, 3 + 2 D, ... at full height, and nowhere else"""
    N = 6 * D + 10
    x = np.zeros((N, 2), dtype=F)
    x[3] = (0.75, -0.5)
    y, hist, ph = s2.flanger_reference(float(D), 0.0, 12345, 678, 1.0, 0.0, 0.0, 1.0, x, np.zeros((D + 1, 2), dtype=F), 99)
    want = np.zeros((N, 2), dtype=F)
    want[3 + D::D] = (0.75, -0.5)
    assert np.array_equal(y, want)
    assert ph == (99 + 12345 * N) & M32 and hist.shape == (D + 1, 2)


@pytest.mark.parametrize("base,depth", [(32.0, 1.0), (32.75, 1.0), (32.0, 4063.0), (2000.3, 2094.6)])
def test_the_top_of_the_triangle_reads_the_oldest_frame(base, depth):
    """phase 2^31 and phase_inc 0: m == 1 at every frame, so d = fl(base + depth), i = floor(d) = H - 1, and frame 0 reads a = w[-(H - 1)]
    and bb = w[-H], the oldest frame of the history"""
    H = history_frames(base, depth)
    d = F(base) + F(depth)
    f = F(d - F(H - 1))
    hist = np.zeros((H, 2), dtype=F)
    hist[0] = (3.0, -5.0)                                        # the oldest frame alone
    out, new, ph = s2.flanger_reference(base, depth, 0, 0, 0.5, 0.25, 0.0, 1.0, np.zeros((2, 2), dtype=F), hist, 1 << 31)
    assert ph == 1 << 31
    assert np.array_equal(out[0], np.array([f * F(3.0), f * F(-5.0)], dtype=F))
    hist[0], hist[1] = (0.0, 0.0), (3.0, -5.0)                   # the frame in front of it: a = hist[1], bb = hist[0] = 0
    out, _, _ = s2.flanger_reference(base, depth, 0, 0, 0.5, 0.25, 0.0, 1.0, np.zeros((2, 2), dtype=F), hist, 1 << 31)
    want_a = np.array([F(3.0) + f * F(-3.0), F(-5.0) + f * F(5.0)], dtype=F)
    assert np.array_equal(out[0], want_a)
    assert np.array_equal(out[1], np.array([f * F(3.0), f * F(-5.0)], dtype=F))     # one frame on it is bb
    assert_bits_equal_finite(out, np_flanger(base, depth, 0, 0, 0.5, 0.25, 0.0, 1.0, np.zeros((2, 2), dtype=F), hist, 1 << 31)[0], "the model agrees")


def test_denormal_products_survive():
    """a history of 2^-120 .. 2^-119 under a wet and a feedback of 2^-10 and f = 0.5: f * e, wet * tap and feedback * tap are denormals,
    none is flushed"""
    base, depth, N = 32.5, 0.0, 40
    H = history_frames(base, depth)
    hist = (np.ldexp(1.0 + np.arange(2 * H) / (4.0 * H), -120)).astype(F).reshape(H, 2)
    x = np.zeros((N, 2), dtype=F)
    lvl = float(np.ldexp(1.0, -10))
    want, want_hist, _ = np_flanger(base, depth, 12345, 0, lvl, lvl, 0.0, lvl, x, hist, 0)
    tiny = float(np.finfo(F).tiny)
    mag = np.abs(want.astype(np.float64))
    assert (mag[:32] > 0.0).all() and (mag < tiny).all()
    line = np.abs(want_hist[H - N:].astype(np.float64))
    assert (line[:32] > 0.0).all() and (line < tiny).all()       # w = +0.0 + (feedback * tap + cross * tap): denormals in the line
    got, got_hist, _ = s2.flanger_reference(base, depth, 12345, 0, lvl, lvl, 0.0, lvl, x, hist, 0)
    assert_bits_equal_finite(got, want, "denormal products")
    assert_bits_equal_finite(got_hist, want_hist, "denormal products: the history")
    # nothing is skipped for f == 0 or a zero coefficient: -0.0 through a + 0 * (bb - a) comes out +0.0
    x = np.full((3, 2), -0.0, dtype=F)
    out, hist, _ = s2.flanger_reference(32.0, 0.0, 0, 0, 0.0, 0.0, 0.0, 1.0, x, np.full((33, 2), -0.0, dtype=F), 0)
    assert not bits(out).any(), "(+0.0 * -0.0 = -0.0) + (1 * (-0.0 + 0 * 0 = +0.0)) is +0.0"
    assert not bits(hist[30:]).any(), "-0.0 + ((0 * +0.0) + (0 * +0.0)) is +0.0"


def test_history_frames():
    L = s2.load_library()
    assert s2.FLANGER_MIN_DELAY == 32.0 and s2.FLANGER_MAX_DELAY == 4095.0
    for base, depth in SHAPES + [(g[0], g[1]) for g in GOOD] + [(32.0, 0.99999994), (33.999996, 0.0), (32.0, 1.9999999), (4094.0, 0.9998)]:
        assert L.s2r_flanger_history_frames(base, depth) == history_frames(base, depth) == s2.flanger_history_frames(base, depth), (base, depth)
        assert 33 <= history_frames(base, depth) <= 4096
    assert history_frames(32.0, 0.0) == 33 and history_frames(4095.0, 0.0) == 4096 and history_frames(4095.0, 0.0001) == 4096
    for base, depth in [(b[0], b[1]) for b in BAD[:13]]:         # (the entries that are bad for their delay range)
        assert L.s2r_flanger_history_frames(base, depth) == 0, (base, depth)
    assert s2.Synth.flanger_history_frames(32.75, 1.0) == 34


def test_range_errors_without_a_handle():
    """every entry looks at the values before it looks at the handle, so the range checks answer without a device, and a refused
    reference call leaves history, phase and output alone; S2R_ERR_INVALID is what no handle gets for values in range"""
    L = s2.load_library()
    for base, depth, fb, cr, dry, wet in BAD:
        assert L.s2r_set_bus_flanger(None, 0, base, depth, 1, 2, fb, cr, dry, wet) == s2s.S2R_ERR_PATCH_RANGE, (base, depth, fb, cr, dry, wet)
    for base, depth, fb, cr, dry, wet in GOOD:
        assert L.s2r_set_bus_flanger(None, 7, base, depth, M32, M32, fb, cr, dry, wet) == s2s.S2R_ERR_INVALID, (base, depth, fb, cr, dry, wet)
        assert L.s2r_set_bus_flanger_params(None, 7, 1, 2, fb, cr, dry, wet) == s2s.S2R_ERR_INVALID
    for fb, cr, dry, wet in [b[2:] for b in BAD[13:]]:
        assert L.s2r_set_bus_flanger_params(None, 0, 1, 2, fb, cr, dry, wet) == s2s.S2R_ERR_PATCH_RANGE, (fb, cr, dry, wet)
    for bus in (8, 255, M32):
        assert L.s2r_set_bus_flanger(None, bus, 32.0, 0.0, 0, 0, 0.0, 0.0, 1.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_clear_bus_flanger(None, bus) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_flanger_params(None, bus, 1, 1, 0.0, 0.0, 1.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_get_bus_flanger(None, bus, None, None, None, None, None, None, None, None) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_clear_bus_flanger(None, 0) == s2s.S2R_ERR_INVALID
    n, b = C.c_uint32(), C.c_float()
    assert L.s2r_get_bus_flanger(None, 0, C.byref(b), None, C.byref(n), None, None, None, None, None) == s2s.S2R_ERR_INVALID
    buf = np.zeros(80, dtype=F)
    assert L.s2r_get_bus_flanger_state(None, 0, _p(buf), 80, C.byref(n)) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_flanger_state(None, 0, _p(buf), 66, 0) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_flanger_state(None, 8, _p(buf), 80, C.byref(n)) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_flanger_state(None, 8, _p(buf), 66, 0) == s2s.S2R_ERR_PATCH_RANGE
    # the reference: a refusal changes neither the history, nor the phase, nor the output
    x, hist, out = _signal(3, 1), _signal(34, 2), np.full((3, 2), 9.0, dtype=F)
    keep, ph = hist.copy(), C.c_uint32(77)
    for base, depth, fb, cr, dry, wet in BAD:
        assert L.s2r_flanger_reference(base, depth, 1, 2, fb, cr, dry, wet, _p(x), 3, _p(hist), C.byref(ph), _p(out)) == s2s.S2R_ERR_PATCH_RANGE, (base, depth, fb, cr)
    ok = (32.75, 1.0, 5, 2, 0.5, -0.5, 1.0, 1.0)
    assert L.s2r_flanger_reference(*ok, _p(x), 3, None, C.byref(ph), _p(out)) == s2s.S2R_ERR_INVALID
    assert L.s2r_flanger_reference(*ok, _p(x), 3, _p(hist), None, _p(out)) == s2s.S2R_ERR_INVALID
    assert L.s2r_flanger_reference(*ok, None, 3, _p(hist), C.byref(ph), _p(out)) == s2s.S2R_ERR_INVALID
    assert np.array_equal(bits(hist), bits(keep)) and (out == 9.0).all() and ph.value == 77
    assert L.s2r_flanger_reference(*ok, None, 0, _p(hist), C.byref(ph), None) == s2s.S2R_OK     # no frames: no x, and out may be null
    assert np.array_equal(bits(hist), bits(keep)) and ph.value == 77
    h = keep.copy()
    assert L.s2r_flanger_reference(*ok, _p(x), 3, _p(h), C.byref(ph), None) == s2s.S2R_OK
    assert ph.value == 92
    assert_bits_equal_finite(h, np_flanger(*ok, x, keep, 77)[1], "out_lr NULL: the state moves on all the same")
    with pytest.raises(ValueError):
        s2.flanger_reference(*ok, x, hist[:3], 0)
    with pytest.raises(s2.S2rError) as err:
        s2.flanger_reference(31.0, 0.0, 0, 0, 0.0, 0.0, 1.0, 1.0, x, hist, 0)
    assert err.value.status == s2s.S2R_ERR_PATCH_RANGE
    assert s2.Synth.flanger_reference(*ok, x, hist, 0)[0].shape == (3, 2)
    syn = _new_or_skip(num_voices=8, max_frames=64)              # with a device the rest runs on a real handle
    if syn is not None:
        check_ranges(syn)


def test_abi_version_stays():
    assert s2.load_library().s2r_abi_version() == 4


NONE = (0.0, 0.0, 0, 0, 0.0, 0.0, 0.0, 0.0)


def check_ranges(syn):
    """the setters' range checks on a live handle, and the params and state entries on a bus without a flanger (also called by
    tests/test_gpu_flanger.py)"""
    L, h = syn.L, syn.h
    assert all(syn.get_bus_flanger(b) == NONE for b in range(s2.MAX_BUSES))      # a fresh handle: no flanger anywhere
    for base, depth, fb, cr, dry, wet in BAD:
        assert L.s2r_set_bus_flanger(h, 0, base, depth, 1, 2, fb, cr, dry, wet) == s2s.S2R_ERR_PATCH_RANGE, (base, depth, fb, cr, dry, wet)
    assert L.s2r_set_bus_flanger(h, 8, 32.0, 0.0, 0, 0, 0.0, 0.0, 1.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
    assert syn.get_bus_flanger(0) == NONE                        # a refused call changes nothing
    buf, ph = np.zeros(80, dtype=F), C.c_uint32(5)
    assert L.s2r_set_bus_flanger_params(h, 0, 1, 1, 0.0, 0.0, 1.0, 1.0) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_flanger_state(h, 0, _p(buf), 80, C.byref(ph)) == s2s.S2R_ERR_INVALID and ph.value == 5
    assert L.s2r_set_bus_flanger_state(h, 0, _p(buf), 68, 0) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_flanger_state(h, 8, _p(buf), 80, None) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_flanger_state(h, 8, _p(buf), 68, 0) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_flanger(h, 8, None, None, None, None, None, None, None, None) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_flanger(h, 0, None, None, None, None, None, None, None, None) == s2s.S2R_OK      # any pointer may be null
    syn.clear_bus_flanger(3)                                     # removing what is not there is no error
    syn.set_bus_flanger(3, 32.75, 1.0, 89478, 0x40000000, -0.5, 0.25, 0.25, 1.0)
    assert syn.get_bus_flanger(3) == (32.75, 1.0, 89478, 0x40000000, -0.5, 0.25, 0.25, 1.0) and syn.get_bus_flanger(0)[0] == 0
    hist, phase = syn.bus_flanger_state(3)
    assert hist.shape == (34, 2) and not bits(hist).any() and phase == 0     # +0.0 everywhere and phase 0 right after the flanger is set
    for count in (0, 66, 67, 69, 80):
        assert L.s2r_set_bus_flanger_state(h, 3, _p(buf), count, 1) == s2s.S2R_ERR_INVALID, count
    assert L.s2r_set_bus_flanger_state(h, 3, None, 68, 1) == s2s.S2R_ERR_INVALID
    for cap in (0, 67):
        assert L.s2r_get_bus_flanger_state(h, 3, _p(buf), cap, C.byref(ph)) == s2s.S2R_ERR_INVALID, cap
    assert L.s2r_get_bus_flanger_state(h, 3, None, 68, C.byref(ph)) == s2s.S2R_ERR_INVALID
    assert syn.bus_flanger_state(3)[1] == 0                      # the refused setters left the phase alone
    assert L.s2r_get_bus_flanger_state(h, 3, _p(buf), 80, None) == s2s.S2R_OK     # a larger buffer will do, and the phase may be null
    new = np.arange(68, dtype=F).reshape(34, 2) - F(3.5)
    syn.set_bus_flanger_state(3, new, 0xDEADBEEF)
    got, phase = syn.bus_flanger_state(3)
    assert np.array_equal(bits(got), bits(new)) and phase == 0xDEADBEEF
    for base, depth, fb, cr, dry, wet in BAD:
        assert L.s2r_set_bus_flanger(h, 3, base, depth, 1, 2, fb, cr, dry, wet) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_flanger_params(h, 3, 1, 2, 0.75, 0.5, 1.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_flanger_params(h, 3, 1, 2, 0.0, 0.0, 0.0, NAN) == s2s.S2R_ERR_PATCH_RANGE
    assert syn.get_bus_flanger(3) == (32.75, 1.0, 89478, 0x40000000, -0.5, 0.25, 0.25, 1.0)
    syn.set_bus_flanger_params(3, M32, 1, 1.0, 0.0, 1.0, 0.0)
    assert syn.get_bus_flanger(3) == (32.75, 1.0, M32, 1, 1.0, 0.0, 1.0, 0.0)
    got, phase = syn.bus_flanger_state(3)
    assert np.array_equal(bits(got), bits(new)) and phase == 0xDEADBEEF      # the parameters keep the state
    syn.set_bus_flanger(3, 40.0, 24.5, 0, 0, 0.0, 0.0, 1.0, 1.0)   # setting it again zeroes it
    got, phase = syn.bus_flanger_state(3)
    assert got.shape == (65, 2) and not bits(got).any() and phase == 0
    syn.clear_bus_flanger(3)
    assert syn.get_bus_flanger(3) == NONE
    assert L.s2r_get_bus_flanger_state(h, 3, _p(buf), 80, None) == s2s.S2R_ERR_INVALID
