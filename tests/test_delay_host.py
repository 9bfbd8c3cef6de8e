"""The per-bus feedback delay, the host side: s2r_delay_reference — the rule restated in plain C++ — held against a
numpy float32 model of the rule written here (np_delay, which tests/test_gpu_delay.py holds the device against too), and the range
checks of the entry points, which answer without a device.  Every comparison is on bits (helpers.assert_bits_equal_finite)."""
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
DELAYS = [1, 2, 3, 63, 64, 65, 256, 1000]
# (feedback, cross).  The last pair stands for "(0.6, -0.4)": as binary32 those two are 0.60000002... and 0.40000000596..., whose
# magnitudes add up to 1 + 2^-25 in double, which the rule's own sum condition refuses (BAD_MIX below holds that pair).  The cross
# used here is the binary32 next to -0.4 towards zero, 1 - 0.6f exactly: the largest that the rule admits beside a feedback of 0.6f.
NEAR_04 = float(F(1.0) - F(0.6))
FEEDS = [(0.0, 0.0), (0.9, 0.0), (0.0, 1.0), (-0.5, 0.5), (0.6, -NEAR_04)]
# (feedback, cross, dry, wet): one value out of its range, a NaN, or the sum condition — 0.6 and 0.4 as floats add up to more
# than 1 in double (0.6f > 0.6, 0.4f > 0.4; in binary32 the sum would round to 1), 0.75 + 0.25 and 0.5 + 0.5 to exactly 1
BAD_MIX = [(1.5, 0.0, 1.0, 1.0), (-1.0000001, 0.0, 1.0, 1.0), (0.0, 1.5, 1.0, 1.0), (0.0, -1.5, 1.0, 1.0), (0.75, 0.5, 1.0, 1.0), (-0.75, 0.5, 1.0, 1.0),
           (0.6, 0.4, 1.0, 1.0), (0.6, -0.4, 1.0, 1.0), (1.0, 1e-7, 1.0, 1.0), (NAN, 0.0, 1.0, 1.0), (0.0, NAN, 1.0, 1.0), (INF, 0.0, 1.0, 1.0), (0.0, -INF, 1.0, 1.0),
           (0.5, 0.5, 1.5, 1.0), (0.5, 0.5, 1.0, 1.5), (0.5, 0.5, -0.25, 1.0), (0.5, 0.5, 1.0, -1e-9), (0.5, 0.5, NAN, 1.0), (0.5, 0.5, 1.0, NAN),
           (0.5, 0.5, INF, 0.0)]
GOOD_MIX = [(0.0, 0.0, 0.0, 0.0), (1.0, 0.0, 1.0, 1.0), (0.0, -1.0, 0.0, 1.0), (0.75, 0.25, 1.0, 0.5), (-0.5, -0.5, 0.25, 1.0), (0.6, -NEAR_04, 0.5, 0.5), (1.0, 1e-30, 1.0, 1.0)]


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def np_delay(D, feedback, cross, dry, wet, x, history):
    """The rule in numpy float32, both channels: frames n and n - D are a block of D frames apart, so the call is walked in blocks of
    D frames — the last one shorter — and every operation of the rule is ONE float32 array operation over a block: p = feedback * t,
    q = cross * u, s = x + p, W = s + q, y = (dry * x) + (wet * t), with t the block before of W and u the same with its channels
    swapped.  x [N, 2], history [D, 2] (oldest first; left as it is) -> (y [N, 2], the history after the call [D, 2])."""
    x = np.ascontiguousarray(x, dtype=F)
    hist = np.ascontiguousarray(history, dtype=F)
    N = x.shape[0]
    assert x.shape == (N, 2) and hist.shape == (D, 2) and D >= 1
    fb, cr, dr, we = F(feedback), F(cross), F(dry), F(wet)
    w = np.concatenate([hist, np.zeros((N, 2), dtype=F)], axis=0)       # W[-D .. N)
    y = np.empty((N, 2), dtype=F)
    with np.errstate(under="ignore"):
        for k0 in range(0, N, D):
            k1 = min(N, k0 + D)
            t = w[k0:k1]                                                 # W[n - D] sits at row n
            u = t[:, ::-1]
            xb = x[k0:k1]
            p = fb * t
            q = cr * u
            s = xb + p
            w[k0 + D:k1 + D] = s + q
            a = dr * xb
            b = we * t
            y[k0:k1] = a + b
    assert y.dtype == F and w.dtype == F
    return y, w[N:].copy()


def _p(a):
    return a.ctypes.data_as(s2s._f32p)


def _signal(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2)) * scale).astype(F)


def _frames(D):
    return sorted({0, 1, D - 1, D, D + 1, 5 * D + 7})


@pytest.mark.parametrize("D", DELAYS)
def test_reference_is_the_numpy_model(D):
    """s2r_delay_reference against np_delay, outputs and the history left behind, from a non-zero history; and the history is the
    last D of (history, W), with W restated once more, frame by frame (_line_signal)"""
    for j, (fb, cr) in enumerate(FEEDS):
        for dry, wet in ((1.0, 1.0), (0.25, 0.5)):
            for N in _frames(D):
                x, hist = _signal(N, 1000 * D + 10 * j + N), _signal(D, 7 * D + j, 0.5)
                want, want_hist = np_delay(D, fb, cr, dry, wet, x, hist)
                got, got_hist = s2.delay_reference(D, fb, cr, dry, wet, x, hist)
                what = "D %d, feedback %g, cross %g, dry %g, wet %g, %d frames" % (D, fb, cr, dry, wet, N)
                assert_bits_equal_finite(got, want, what)
                assert_bits_equal_finite(got_hist, want_hist, what + ": the history")
                if dry == 1.0:
                    w_all = np.concatenate([hist, _line_signal(D, fb, cr, x, hist)], axis=0)
                    assert_bits_equal_finite(got_hist, w_all[w_all.shape[0] - D:], what + ": the last D of (history, W)")


def _line_signal(D, fb, cr, x, hist):
    """W[0 .. N) frame by frame in Python floats rounded to float32 after every operation: a third restatement, scalar"""
    w = [tuple(r) for r in np.ascontiguousarray(hist, dtype=F)]
    with np.errstate(under="ignore"):
        for n in range(x.shape[0]):
            t = w[n]
            new = []
            for c in range(2):
                p = F(fb) * t[c]
                q = F(cr) * t[1 - c]
                s = x[n, c] + p
                new.append(F(s + q))
            w.append(tuple(new))
    return np.array(w[D:], dtype=F).reshape(-1, 2)


@pytest.mark.parametrize("D", [1, 3, 64, 1000])
def test_two_calls_are_one(D):
    """calls of a and b frames equal one call of a + b, in output and history"""
    for a, b in ((1, 1), (D - 1, 2), (D, D + 1), (7, 5 * D), (0, 3), (3, 0)):
        x, hist = _signal(a + b, 31 * D + a), _signal(D, 5 * D + b)
        whole, whole_hist = s2.delay_reference(D, 0.6, -NEAR_04, 0.5, 1.0, x, hist)
        first, mid = s2.delay_reference(D, 0.6, -NEAR_04, 0.5, 1.0, x[:a], hist)
        second, end = s2.delay_reference(D, 0.6, -NEAR_04, 0.5, 1.0, x[a:], mid)
        assert_bits_equal_finite(np.concatenate([first, second], axis=0), whole, "D %d: %d + %d frames" % (D, a, b))
        assert_bits_equal_finite(end, whole_hist, "D %d: %d + %d frames, the history" % (D, a, b))


def test_denormal_products_survive():
    """a line of 2^-120 .. 2^-119 under a feedback of 2^-10: every feedback * t is a denormal, none is zero, and it arrives in W
    (x is zero) and, D frames later, in the output; the second pass leaves smaller ones in the history"""
    D, N = 5, 10
    hist = (np.ldexp(1.0 + np.arange(2 * D) / (4.0 * D), -120)).astype(F).reshape(D, 2)
    fb = float(np.ldexp(1.0, -10))
    x = np.zeros((N, 2), dtype=F)
    want, want_hist = np_delay(D, fb, 0.0, 0.0, 1.0, x, hist)
    tiny = float(np.finfo(F).tiny)
    first = np.abs(want[D:2 * D].astype(np.float64))
    assert (first > 0.0).all() and (first < tiny).all()          # the products of the first pass, read out in the second
    got, got_hist = s2.delay_reference(D, fb, 0.0, 0.0, 1.0, x, hist)
    assert_bits_equal_finite(got, want, "denormal products")
    assert_bits_equal_finite(got_hist, want_hist, "denormal products: the history")
    assert (np.abs(got_hist.astype(np.float64)) < tiny).all() and bits(got_hist).any()


def test_minus_zero_plus_plus_zero_is_plus_zero():
    """x = -0.0 over a line of -0.0, feedback 0.5, cross -0.5: p = -0.0 and s = -0.0 + -0.0 = -0.0; q = (-0.5) * (-0.0) = +0.0; and
    W = s + q = +0.0, as the rule says.  y = (1 * -0.0) + (1 * -0.0) stays -0.0."""
    D, N = 2, 2
    x = np.full((N, 2), -0.0, dtype=F)
    hist = np.full((D, 2), -0.0, dtype=F)
    out, new = s2.delay_reference(D, 0.5, -0.5, 1.0, 1.0, x, hist)
    want, want_hist = np_delay(D, 0.5, -0.5, 1.0, 1.0, x, hist)
    assert not bits(new).any(), "W = (-0.0) + (+0.0) is +0.0"
    assert_bits_equal_finite(new, want_hist, "the model agrees")
    assert (bits(out) == 0x80000000).all(), "y = (1 * -0.0) + (1 * -0.0) is -0.0"
    assert_bits_equal_finite(out, want, "the model agrees on y")
    # a zero coefficient skips nothing either: cross = +0.0 over a positive line gives q = +0.0, s = -0.0 + (0 * t = +0.0) = +0.0
    hist = np.full((D, 2), 1.0, dtype=F)
    _, new = s2.delay_reference(D, 0.0, 0.0, 1.0, 1.0, x, hist)
    assert not bits(new).any()


def test_ping_pong():
    """cross 1, feedback 0, input on the left only, one impulse: echo k — k = 0 the first repeat, at frame D — is on channel k mod 2
    only, at full height"""
    D, N = 7, 7 * 6 + 3
    x = np.zeros((N, 2), dtype=F)
    x[0, 0] = 0.75
    out, _ = s2.delay_reference(D, 0.0, 1.0, 0.0, 1.0, x, np.zeros((D, 2), dtype=F))
    want = np.zeros((N, 2), dtype=F)
    for k in range(1, N // D + 1):
        want[k * D, (k + 1) % 2] = 0.75                          # the first echo reads W_L: left; the second what crossed over: right
    assert np.array_equal(out, want)
    echoes = out[D::D]
    assert all(e[(k + 1) % 2] == 0.0 and e[k % 2] == F(0.75) for k, e in enumerate(echoes))


def test_range_errors_without_a_handle():
    """every entry looks at the values before it looks at the handle, so the range checks answer without a device, and a refused
    reference call leaves its history and output alone; S2R_ERR_INVALID is what no handle gets for values in range"""
    L = s2.load_library()
    assert s2.MAX_DELAY_FRAMES == 262144
    for mix in BAD_MIX:
        assert L.s2r_set_bus_delay(None, 0, 100, *mix) == s2s.S2R_ERR_PATCH_RANGE, mix
        assert L.s2r_set_bus_delay(None, 0, 0, *mix) == s2s.S2R_ERR_PATCH_RANGE, mix
        assert L.s2r_set_bus_delay_mix(None, 0, *mix) == s2s.S2R_ERR_PATCH_RANGE, mix
    for mix in GOOD_MIX:
        assert L.s2r_set_bus_delay(None, 7, 100, *mix) == s2s.S2R_ERR_INVALID, mix
        assert L.s2r_set_bus_delay_mix(None, 7, *mix) == s2s.S2R_ERR_INVALID, mix
    for bus in (8, 255, 0xffffffff):
        assert L.s2r_set_bus_delay(None, bus, 100, 0.5, 0.5, 1.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_delay(None, bus, 0, 0.0, 0.0, 0.0, 0.0) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_delay_mix(None, bus, 0.5, 0.5, 1.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_get_bus_delay(None, bus, None, None, None, None, None) == s2s.S2R_ERR_PATCH_RANGE
    for d in (s2.MAX_DELAY_FRAMES + 1, 0xffffffff):
        assert L.s2r_set_bus_delay(None, 0, d, 0.5, 0.5, 1.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_delay(None, 0, s2.MAX_DELAY_FRAMES, 0.5, 0.5, 1.0, 1.0) == s2s.S2R_ERR_INVALID
    n = C.c_uint32()
    assert L.s2r_get_bus_delay(None, 0, C.byref(n), None, None, None, None) == s2s.S2R_ERR_INVALID
    buf = np.zeros(8, dtype=F)
    assert L.s2r_get_bus_delay_history(None, 0, _p(buf), 8) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_delay_history(None, 0, _p(buf), 8) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_delay_history(None, 8, _p(buf), 8) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_delay_history(None, 8, _p(buf), 8) == s2s.S2R_ERR_PATCH_RANGE
    # the reference: a refusal changes neither the history nor the output
    x, hist, out = _signal(3, 1), _signal(4, 2), np.full((3, 2), 9.0, dtype=F)
    keep = hist.copy()
    for mix in BAD_MIX:
        assert L.s2r_delay_reference(4, *mix, _p(x), 3, _p(hist), _p(out)) == s2s.S2R_ERR_PATCH_RANGE, mix
    for d in (0, s2.MAX_DELAY_FRAMES + 1, 0xffffffff):
        assert L.s2r_delay_reference(d, 0.5, 0.5, 1.0, 1.0, _p(x), 3, _p(hist), _p(out)) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_delay_reference(4, 0.5, 0.5, 1.0, 1.0, _p(x), 3, None, _p(out)) == s2s.S2R_ERR_INVALID
    assert L.s2r_delay_reference(4, 0.5, 0.5, 1.0, 1.0, None, 3, _p(hist), _p(out)) == s2s.S2R_ERR_INVALID
    assert np.array_equal(bits(hist), bits(keep)) and (out == 9.0).all()
    assert L.s2r_delay_reference(4, 0.5, 0.5, 1.0, 1.0, None, 0, _p(hist), None) == s2s.S2R_OK      # no frames: no x, and out may be null
    assert np.array_equal(bits(hist), bits(keep))
    for mix in GOOD_MIX:
        h = keep.copy()
        assert L.s2r_delay_reference(4, *mix, _p(x), 3, _p(h), None) == s2s.S2R_OK, mix
        assert_bits_equal_finite(h, np_delay(4, *mix, x, keep)[1], "out_lr NULL: the history moves on all the same")
    with pytest.raises(ValueError):
        s2.delay_reference(4, 0.0, 0.0, 1.0, 1.0, x, hist[:3])
    with pytest.raises(s2.S2rError) as err:
        s2.delay_reference(4, 0.75, 0.5, 1.0, 1.0, x, hist)
    assert err.value.status == s2s.S2R_ERR_PATCH_RANGE
    assert s2.Synth.delay_reference(4, 0.0, 0.0, 1.0, 1.0, x, hist)[0].shape == (3, 2)
    syn = _new_or_skip(num_voices=8, max_frames=64)              # with a device the rest runs on a real handle
    if syn is not None:
        check_ranges(syn)


def test_abi_version_stays():
    assert s2.load_library().s2r_abi_version() == 4


def check_ranges(syn):
    """the four setters' range checks on a live handle, and the mix and history entries on a bus without a delay (also called by
    tests/test_gpu_delay.py)"""
    L, h = syn.L, syn.h
    assert all(syn.get_bus_delay(b) == (0, 0.0, 0.0, 0.0, 0.0) for b in range(s2.MAX_BUSES))      # a fresh handle: no delay anywhere
    for mix in BAD_MIX:
        assert L.s2r_set_bus_delay(h, 0, 100, *mix) == s2s.S2R_ERR_PATCH_RANGE, mix
    assert L.s2r_set_bus_delay(h, 8, 100, 0.5, 0.5, 1.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_delay(h, 0, s2.MAX_DELAY_FRAMES + 1, 0.5, 0.5, 1.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
    assert syn.get_bus_delay(0) == (0, 0.0, 0.0, 0.0, 0.0)       # a refused call changes nothing
    buf = np.zeros(16, dtype=F)
    assert L.s2r_set_bus_delay_mix(h, 0, 0.5, 0.5, 1.0, 1.0) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_delay_history(h, 0, _p(buf), 16) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_delay_history(h, 0, _p(buf), 8) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_delay_history(h, 8, _p(buf), 16) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_delay_history(h, 8, _p(buf), 16) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_delay(h, 8, None, None, None, None, None) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_delay(h, 0, None, None, None, None, None) == s2s.S2R_OK      # any pointer may be null
    syn.clear_bus_delay(3)                                       # removing what is not there is no error
    syn.set_bus_delay(3, 4, 0.75, -0.25, 0.25, 1.0)
    assert syn.get_bus_delay(3) == (4, 0.75, -0.25, 0.25, 1.0) and syn.get_bus_delay(0)[0] == 0
    hist = syn.bus_delay_history(3)
    assert hist.shape == (4, 2) and not bits(hist).any()         # +0.0 everywhere right after the delay is set
    for count in (0, 6, 7, 9, 16):
        assert L.s2r_set_bus_delay_history(h, 3, _p(buf), count) == s2s.S2R_ERR_INVALID, count
    assert L.s2r_set_bus_delay_history(h, 3, None, 8) == s2s.S2R_ERR_INVALID
    for cap in (0, 7):
        assert L.s2r_get_bus_delay_history(h, 3, _p(buf), cap) == s2s.S2R_ERR_INVALID, cap
    assert L.s2r_get_bus_delay_history(h, 3, None, 8) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_delay_history(h, 3, _p(buf), 16) == s2s.S2R_OK       # a larger buffer will do
    new = np.arange(8, dtype=F).reshape(4, 2) - F(3.5)
    syn.set_bus_delay_history(3, new)
    assert np.array_equal(bits(syn.bus_delay_history(3)), bits(new))
    for mix in BAD_MIX:
        assert L.s2r_set_bus_delay_mix(h, 3, *mix) == s2s.S2R_ERR_PATCH_RANGE, mix
        assert L.s2r_set_bus_delay(h, 3, 9, *mix) == s2s.S2R_ERR_PATCH_RANGE, mix
    assert syn.get_bus_delay(3) == (4, 0.75, -0.25, 0.25, 1.0)
    assert np.array_equal(bits(syn.bus_delay_history(3)), bits(new))     # the refused setters left the history alone
    syn.set_bus_delay_mix(3, -0.5, 0.5, 1.0, 0.0)
    assert syn.get_bus_delay(3) == (4, -0.5, 0.5, 1.0, 0.0)
    assert np.array_equal(bits(syn.bus_delay_history(3)), bits(new))     # the mix keeps the history
    syn.set_bus_delay(3, 6, 0.0, 0.0, 1.0, 1.0)                  # setting it again zeroes it
    assert syn.bus_delay_history(3).shape == (6, 2) and not bits(syn.bus_delay_history(3)).any()
    syn.clear_bus_delay(3)
    assert syn.get_bus_delay(3) == (0, 0.0, 0.0, 0.0, 0.0)
    assert L.s2r_get_bus_delay_history(h, 3, _p(buf), 16) == s2s.S2R_ERR_INVALID
