"""The per-bus parametric EQ, the host side: s2r_eq_reference — the rule restated in plain C++ — held against a numpy
float32 model of the rule written here (np_eq: a loop over frames, vectorised over the two channels), s2r_eq_design against the
Audio-EQ-Cookbook formulas in numpy float64 (np_design), and the range checks of the entry points, which answer without a device.
Comparisons of signals and states are on bits (helpers.assert_bits_equal_finite).

Run as a program (PYTHONPATH=.:tests python tests/test_eq_host.py, from the repository's root) this file measures how far the numpy design, rounded to binary32, is from the ideal magnitude at each band's
defining frequency, and writes twice that — the bound the library's design is held to — into profiles/truth/eq_design_deviation.json."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_reverb_host import _new_or_skip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUTH = os.path.join(ROOT, "profiles", "truth", "eq_design_deviation.json")
F = np.float32
NAN = float("nan")
INF = float("inf")
M32 = 0xFFFFFFFF
KINDS = {"peak": s2.EQ_PEAK, "low_shelf": s2.EQ_LOW_SHELF, "high_shelf": s2.EQ_HIGH_SHELF, "lowpass": s2.EQ_LOWPASS, "highpass": s2.EQ_HIGHPASS}
# (kind, freq_hz, gain_db, q, sample_rate): every kind low and high in the band, cut and boost, narrow and wide, the gain's ends
DESIGNS = [("peak", 1000.0, 6.0, 1.0, 48000.0), ("peak", 100.0, -12.0, 4.0, 48000.0), ("peak", 15000.0, 48.0, 0.5, 44100.0),
           ("peak", 40.0, -48.0, 0.7071, 96000.0), ("low_shelf", 200.0, 9.0, 0.7071, 48000.0), ("low_shelf", 80.0, -15.0, 1.0, 44100.0),
           ("high_shelf", 8000.0, 4.5, 0.7071, 48000.0), ("high_shelf", 12000.0, -24.0, 0.5, 96000.0), ("lowpass", 5000.0, 0.0, 0.7071, 48000.0),
           ("lowpass", 300.0, 0.0, 3.0, 44100.0), ("highpass", 120.0, 0.0, 0.7071, 48000.0), ("highpass", 9000.0, 0.0, 2.0, 48000.0)]
UNIT = np.array([1.0, 0.0, 0.0, 0.0, 0.0], dtype=F)


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def _p(a):
    return a.ctypes.data_as(s2s._f32p)


def np_eq(coeffs, x, state):
    """the rule in numpy float32: a loop over frames and bands, both channels at once; every product and every sum is one float32
    operation.  coeffs [n_bands, 5], x [frames, 2], state [n_bands, 4]; returns (out [frames, 2], the state after the call)"""
    c = np.asarray(coeffs, dtype=F).reshape(-1, 5)
    st = np.array(state, dtype=F).reshape(-1, 2, 2)              # [band][s1 | s2][channel]
    x = np.asarray(x, dtype=F)
    out = np.empty_like(x)
    with np.errstate(under="ignore"):
        for n in range(x.shape[0]):
            v = x[n]
            for k in range(c.shape[0]):
                b0, b1, b2, a1, a2 = c[k]
                y = b0 * v + st[k, 0]
                s1 = (b1 * v - a1 * y) + st[k, 1]
                st[k, 1] = b2 * v - a2 * y
                st[k, 0] = s1
                v = y
            out[n] = v
    assert out.dtype == F and st.dtype == F
    return out, st.reshape(-1, 4)


def np_design(kind, f, gain_db, q, sr):
    """the Audio-EQ-Cookbook band in float64, divided by a0: (b0, b1, b2, a1, a2) as float64"""
    w0 = 2.0 * np.pi * f / sr
    cw, alpha = np.cos(w0), np.sin(w0) / (2.0 * q)
    A = np.power(10.0, gain_db / 40.0)
    if kind == "peak":
        b = (1.0 + alpha * A, -2.0 * cw, 1.0 - alpha * A)
        a = (1.0 + alpha / A, -2.0 * cw, 1.0 - alpha / A)
    elif kind == "low_shelf":
        t = 2.0 * np.sqrt(A) * alpha
        b = (A * ((A + 1.0) - (A - 1.0) * cw + t), 2.0 * A * ((A - 1.0) - (A + 1.0) * cw), A * ((A + 1.0) - (A - 1.0) * cw - t))
        a = ((A + 1.0) + (A - 1.0) * cw + t, -2.0 * ((A - 1.0) + (A + 1.0) * cw), (A + 1.0) + (A - 1.0) * cw - t)
    elif kind == "high_shelf":
        t = 2.0 * np.sqrt(A) * alpha
        b = (A * ((A + 1.0) + (A - 1.0) * cw + t), -2.0 * A * ((A - 1.0) + (A + 1.0) * cw), A * ((A + 1.0) + (A - 1.0) * cw - t))
        a = ((A + 1.0) - (A - 1.0) * cw + t, 2.0 * ((A - 1.0) - (A + 1.0) * cw), (A + 1.0) - (A - 1.0) * cw - t)
    elif kind == "lowpass":
        b = ((1.0 - cw) / 2.0, 1.0 - cw, (1.0 - cw) / 2.0)
        a = (1.0 + alpha, -2.0 * cw, 1.0 - alpha)
    else:
        b = ((1.0 + cw) / 2.0, -(1.0 + cw), (1.0 + cw) / 2.0)
        a = (1.0 + alpha, -2.0 * cw, 1.0 - alpha)
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]], dtype=np.float64)


def ideal(kind, gain_db, q):
    """the magnitude the formulas give at the defining frequency: the whole gain at a peak's centre, half of it in dB at a shelf's
    corner, Q at the corner of a low-pass or high-pass"""
    return {"peak": 10.0 ** (gain_db / 20.0), "low_shelf": 10.0 ** (gain_db / 40.0), "high_shelf": 10.0 ** (gain_db / 40.0)}.get(kind, q)


def magnitude(c, f, sr):
    """|H(e^jw)| of a band at f, in float64 from the coefficients as given"""
    b0, b1, b2, a1, a2 = [float(v) for v in c]
    z = np.exp(-1j * 2.0 * np.pi * f / sr)
    return float(abs((b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)))


def deviation(c, kind, f, gain_db, q, sr):
    want = ideal(kind, gain_db, q)
    return abs(magnitude(c, f, sr) - want) / want


def measure():
    """per design: the relative deviation of the numpy design, rounded to binary32, from the ideal, and the bound: twice that"""
    rows = []
    for kind, f, g, q, sr in DESIGNS:
        d = deviation(np_design(kind, f, g, q, sr).astype(F), kind, f, g, q, sr)
        rows.append({"kind": kind, "freq_hz": f, "gain_db": g, "q": q, "sample_rate": sr, "reference_deviation": d, "bound": 2.0 * d})
    return {"what": "relative deviation |H(f0)| / ideal - 1 of the Audio-EQ-Cookbook band computed in numpy float64 and rounded to binary32; "
                    "bound = 2 x that; s2r_eq_design is held to the bound (tests/test_eq_host.py)", "designs": rows}


def _signal(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((n, 2)) * scale).astype(F)


def _bands(n_bands, seed=0):
    picks = [("peak", 1000.0, 6.0, 1.0), ("low_shelf", 200.0, -9.0, 0.7071), ("highpass", 60.0, 0.0, 0.7071), ("peak", 7000.0, -18.0, 8.0),
             ("lowpass", 12000.0, 0.0, 1.5), ("high_shelf", 9000.0, 12.0, 0.9)]
    return np.stack([s2.eq_design(KINDS[k], f, g, q, 48000.0) for k, f, g, q in (picks[(seed + i) % len(picks)] for i in range(n_bands))])


@pytest.mark.parametrize("n_bands", [1, 2, 3, 4])
@pytest.mark.parametrize("frames", [0, 1, 2, 5, 1000])
def test_reference_is_the_numpy_model(n_bands, frames):
    c = _bands(n_bands, n_bands)
    x = _signal(frames, 10 * n_bands + frames)
    st0 = (_signal(2 * n_bands, 99 + frames, 0.25).reshape(n_bands, 4) if frames % 2 else np.zeros((n_bands, 4), dtype=F))
    want, st_want = np_eq(c, x, st0)
    got, st_got = s2.eq_reference(c, x, st0)
    assert_bits_equal_finite(got, want, "%d bands, %d frames: the output" % (n_bands, frames))
    assert_bits_equal_finite(st_got, st_want, "%d bands, %d frames: the state" % (n_bands, frames))
    if frames == 1000:
        assert bits(got).any() and not np.array_equal(bits(got), bits(x))


@pytest.mark.parametrize("n_bands", [1, 4])
def test_two_calls_are_one(n_bands):
    c = _bands(n_bands, 2)
    x = _signal(337, 5)
    zero = np.zeros((n_bands, 4), dtype=F)
    whole, st_whole = s2.eq_reference(c, x, zero)
    for cut in (0, 1, 2, 100, 336, 337):
        a, st = s2.eq_reference(c, x[:cut], zero)
        b, st = s2.eq_reference(c, x[cut:], st)
        assert_bits_equal_finite(np.concatenate([a, b]), whole, "cut at %d" % cut)
        assert_bits_equal_finite(st, st_whole, "the state, cut at %d" % cut)


def test_the_denormal_tail_is_kept():
    """an impulse through a band with poles at radius 0.5 (a2 = 0.25), run until the state is subnormal and on until it is zero: the
    reference follows the numpy model through the subnormals bit for bit, and does not flush them"""
    c = np.array([[1.0, 0.5, 0.25, -0.5, 0.25]], dtype=F)
    x = np.zeros((400, 2), dtype=F)
    x[0] = (1.0, -0.75)
    want, st_want = np_eq(c, x, np.zeros((1, 4), dtype=F))
    got, st_got = s2.eq_reference(c, x, np.zeros((1, 4), dtype=F))
    tiny = float(np.finfo(F).tiny)
    sub = (np.abs(want) > 0.0) & (np.abs(want) < tiny)
    assert sub.any(), "the tail never reaches the subnormals: choose another band"
    assert_bits_equal_finite(got, want, "the denormal tail")
    assert_bits_equal_finite(st_got, st_want, "the state behind it")
    # stopped inside the tail, the state itself is subnormal and is carried
    first = int(np.nonzero(sub.any(axis=1))[0][0]) + 2
    _, st_mid = s2.eq_reference(c, x[:first], np.zeros((1, 4), dtype=F))
    assert ((np.abs(st_mid) > 0.0) & (np.abs(st_mid) < tiny)).any()
    assert_bits_equal_finite(st_mid, np_eq(c, x[:first], np.zeros((1, 4), dtype=F))[1], "a subnormal state")


def test_a_unit_band_is_not_a_wire_for_minus_zero():
    """(1, 0, 0, 0, 0) passes every value through but gives up the sign of a zero: -0.0 + +0.0 = +0.0, and the rule says so"""
    x = np.array([[-0.0, 1.5], [2.0, -0.0], [-3.0, 0.0]], dtype=F)
    got, st = s2.eq_reference(UNIT, x, np.zeros((1, 4), dtype=F))
    assert np.array_equal(got, x)
    assert bits(got)[0, 0] == 0 and bits(got)[1, 1] == 0 and bits(x)[0, 0] == 0x80000000
    assert_bits_equal_finite(got, np_eq(UNIT, x, np.zeros((1, 4), dtype=F))[0], "the unit band")


def _triangle_edge():
    up = float(np.nextafter(F(1.0), F(2.0)))
    below = float(np.nextafter(F(1.0), F(0.0)))
    bad = [(0.0, 1.0), (0.0, -1.0), (0.0, up), (2.0, 1.0), (1.0 + below, below), (-(1.0 + below), below), (0.5, -0.5), (-0.5, -0.5), (2.0, below),
           (0.0, -up), (1e-3, -below - 0.0)]
    good = [(0.0, 0.0), (0.0, below), (0.0, -below), (1.9, 0.95), (-1.9, 0.95), (0.49, -0.5), (float(np.nextafter(F(1.0 + below), F(0.0))), below)]
    return bad, good


def bad_bands():
    """one band each, out of range: a coefficient that is not finite, or (a1, a2) on or outside the stability triangle"""
    out = []
    for i in range(5):
        for v in (NAN, INF, -INF):
            c = np.array([1.0, 0.25, 0.125, -0.5, 0.25], dtype=F)
            c[i] = v
            out.append(c)
    for a1, a2 in _triangle_edge()[0]:
        out.append(np.array([1.0, 0.0, 0.0, a1, a2], dtype=F))
    return out


def good_bands():
    return [np.array([3.0e38, -3.0e38, 0.0, a1, a2], dtype=F) for a1, a2 in _triangle_edge()[1]]


def test_the_triangle_is_evaluated_in_double_from_the_floats():
    for c in bad_bands():
        a1, a2 = float(c[3]), float(c[4])
        assert not (np.isfinite(c).all() and abs(a2) < 1.0 and abs(a1) < 1.0 + a2), c
    for c in good_bands():
        a1, a2 = float(c[3]), float(c[4])
        assert abs(a2) < 1.0 and abs(a1) < 1.0 + a2, c


def test_range_errors_without_a_handle():
    """every entry looks at the values before it looks at the handle, so the range checks answer without a device, and a refused
    reference call leaves state and output alone; S2R_ERR_INVALID is what no handle gets for values in range"""
    L = s2.load_library()
    ok4 = np.ascontiguousarray(_bands(4))
    for setter in (L.s2r_set_bus_eq, L.s2r_set_bus_eq_coeffs):
        for c in bad_bands():
            assert setter(None, 0, 1, _p(c)) == s2s.S2R_ERR_PATCH_RANGE, c
            four = ok4.copy()
            four[3] = c                                          # ... and in the last of four bands
            assert setter(None, 0, 4, _p(four)) == s2s.S2R_ERR_PATCH_RANGE, c
        for c in good_bands():
            assert setter(None, 7, 1, _p(c)) == s2s.S2R_ERR_INVALID, c
        five = np.concatenate([ok4, ok4[:1]])
        assert setter(None, 0, 5, _p(five)) == s2s.S2R_ERR_PATCH_RANGE and setter(None, 0, M32, _p(five)) == s2s.S2R_ERR_PATCH_RANGE
        for bus in (8, 255, M32):
            assert setter(None, bus, 1, _p(ok4)) == s2s.S2R_ERR_PATCH_RANGE
            assert setter(None, bus, 0, None) == s2s.S2R_ERR_PATCH_RANGE
        assert setter(None, 0, 4, _p(ok4)) == s2s.S2R_ERR_INVALID
        assert setter(None, 0, 0, None) == s2s.S2R_ERR_INVALID   # no bands: nothing to look at but the handle
    n = C.c_uint32(5)
    buf = np.zeros(20, dtype=F)
    assert L.s2r_get_bus_eq(None, 8, C.byref(n), _p(buf), 20) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_eq(None, 0, C.byref(n), _p(buf), 20) == s2s.S2R_ERR_INVALID and n.value == 5
    assert L.s2r_get_bus_eq_state(None, 8, _p(buf), 16) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_eq_state(None, 8, _p(buf), 16) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_eq_state(None, 0, _p(buf), 16) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_eq_state(None, 0, _p(buf), 16) == s2s.S2R_ERR_INVALID
    # the reference: a refusal changes neither the state nor the output
    x, st, out = _signal(3, 1), _signal(2, 2).reshape(1, 4), np.full((3, 2), 9.0, dtype=F)
    keep = st.copy()
    for c in bad_bands():
        assert L.s2r_eq_reference(1, _p(c), _p(x), 3, _p(st), _p(out)) == s2s.S2R_ERR_PATCH_RANGE, c
    assert L.s2r_eq_reference(0, _p(ok4), _p(x), 3, _p(st), _p(out)) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_eq_reference(5, _p(np.concatenate([ok4, ok4])), _p(x), 3, _p(st), _p(out)) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_eq_reference(1, None, _p(x), 3, _p(st), _p(out)) == s2s.S2R_ERR_INVALID
    assert L.s2r_eq_reference(1, _p(ok4), _p(x), 3, None, _p(out)) == s2s.S2R_ERR_INVALID
    assert L.s2r_eq_reference(1, _p(ok4), None, 3, _p(st), _p(out)) == s2s.S2R_ERR_INVALID
    assert np.array_equal(bits(st), bits(keep)) and (out == 9.0).all()
    assert L.s2r_eq_reference(1, _p(ok4), None, 0, _p(st), None) == s2s.S2R_OK      # no frames: no x, and out may be null
    assert np.array_equal(bits(st), bits(keep))
    assert L.s2r_eq_reference(1, _p(ok4), _p(x), 3, _p(st), None) == s2s.S2R_OK
    assert_bits_equal_finite(st, np_eq(ok4[:1], x, keep)[1], "out_lr NULL: the state moves on all the same")
    with pytest.raises(ValueError):
        s2.eq_reference(ok4, x, keep)                            # four bands, the state of one
    with pytest.raises(s2.S2rError) as err:
        s2.eq_reference(bad_bands()[0], x, keep)
    assert err.value.status == s2s.S2R_ERR_PATCH_RANGE
    assert s2.Synth.eq_reference(ok4[:1], x, keep)[0].shape == (3, 2)
    syn = _new_or_skip(num_voices=8, max_frames=64)              # with a device the rest runs on a real handle
    if syn is not None:
        check_ranges(syn)


def test_design_range_checks():
    L = s2.load_library()
    out = np.full(5, 9.0, dtype=F)
    bad = [(0, NAN, 0.0, 1.0, 48000.0), (0, 1000.0, NAN, 1.0, 48000.0), (0, 1000.0, 0.0, NAN, 48000.0), (0, 1000.0, 0.0, 1.0, NAN),
           (3, 1000.0, NAN, 1.0, 48000.0),                       # (a NaN is a NaN, whether the kind looks at the gain or not)
           (0, 0.0, 0.0, 1.0, 48000.0), (0, -1.0, 0.0, 1.0, 48000.0), (0, 24000.0, 0.0, 1.0, 48000.0), (0, 30000.0, 0.0, 1.0, 48000.0),
           (0, INF, 0.0, 1.0, 48000.0), (0, 1000.0, 0.0, 0.0, 48000.0), (0, 1000.0, 0.0, -1.0, 48000.0), (0, 1000.0, 48.000001, 1.0, 48000.0),
           (0, 1000.0, -48.000001, 1.0, 48000.0), (0, 1000.0, INF, 1.0, 48000.0), (1, 1000.0, 50.0, 1.0, 48000.0), (-1, 1000.0, 0.0, 1.0, 48000.0),
           (5, 1000.0, 0.0, 1.0, 48000.0), (0, 1000.0, 0.0, 1.0, 0.0), (0, 1000.0, 0.0, 1.0, -48000.0),
           (3, 1000.0, 0.0, 1e-12, 48000.0)]                    # (in range, but alpha is so large that a2 rounds to -1: the setter's check refuses the result)
    for kind, f, g, q, sr in bad:
        assert L.s2r_eq_design(kind, f, g, q, sr, _p(out)) == s2s.S2R_ERR_PATCH_RANGE, (kind, f, g, q, sr)
    assert (out == 9.0).all()
    assert L.s2r_eq_design(0, 1000.0, 0.0, 1.0, 48000.0, None) == s2s.S2R_ERR_INVALID
    for kind in range(5):                                        # the ends of the audio band and of the gain: in range, and what comes back the setter takes
        for f in (20.0, 20000.0):
            for g in (-48.0, 48.0):
                assert L.s2r_eq_design(kind, f, g, 0.7071, 48000.0, _p(out)) == s2s.S2R_OK, (kind, f, g)
                assert L.s2r_set_bus_eq(None, 0, 1, _p(out)) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        s2.eq_design(s2.EQ_PEAK, 1000.0, 0.0, 0.0, 48000.0)
    assert err.value.status == s2s.S2R_ERR_PATCH_RANGE


def _adjacent(a, b):
    """equal, or neighbours in binary32 (as ordered integers, so that the two zeros are one step apart at most)"""
    def key(v):
        u = int(bits(v).reshape(-1)[0])
        return u if u < 0x80000000 else 0x80000000 - u
    return abs(key(a) - key(b)) <= 1


@pytest.mark.parametrize("kind,f,g,q,sr", DESIGNS)
def test_design_is_the_cookbook_in_float64(kind, f, g, q, sr):
    """each coefficient equal or adjacent in binary32 to the numpy float64 formulas rounded once: the two libms may differ in the last
    place before the one rounding"""
    got = s2.eq_design(KINDS[kind], f, g, q, sr)
    want = np_design(kind, f, g, q, sr).astype(F)
    assert got.dtype == F and got.shape == (5,)
    for i in range(5):
        assert _adjacent(got[i], want[i]), (kind, "b0 b1 b2 a1 a2".split()[i], float(got[i]), float(want[i]))


def test_a_peak_of_zero_db_is_flat_exactly():
    for f, q, sr in [(1000.0, 1.0, 48000.0), (55.0, 7.0, 44100.0), (19000.0, 0.3, 96000.0)]:
        c = s2.eq_design(s2.EQ_PEAK, f, 0.0, q, sr)
        assert c[0] == F(1.0) and bits(c[1]) == bits(c[3]) and bits(c[2]) == bits(c[4]), c


def test_the_committed_bounds_are_the_measurement():
    """profiles/truth/eq_design_deviation.json lists these designs, and each bound is twice the deviation recorded beside it.  The
    deviations are binary32's: around 1e-7 in the middle of the band, up to 5e-4 for a deep cut at 40 Hz of 96 kHz, where the poles
    and zeros crowd z = 1 — far below the per cent a wrong `ideal` would show"""
    doc = json.load(open(TRUTH))
    assert [(r["kind"], r["freq_hz"], r["gain_db"], r["q"], r["sample_rate"]) for r in doc["designs"]] == DESIGNS
    for r in doc["designs"]:
        assert r["bound"] == 2.0 * r["reference_deviation"] and 0.0 <= r["reference_deviation"] < 1e-2, r


@pytest.mark.parametrize("i", range(len(DESIGNS)))
def test_design_magnitude_at_the_defining_frequency(i):
    """the library's band, at its defining frequency, is as close to the ideal magnitude — the gain at a peak's centre, half the gain in
    dB at a shelf's corner, Q at a filter's corner — as twice the numpy reference's own deviation (measured on the CPU, committed)"""
    kind, f, g, q, sr = DESIGNS[i]
    row = json.load(open(TRUTH))["designs"][i]
    d = deviation(s2.eq_design(KINDS[kind], f, g, q, sr), kind, f, g, q, sr)
    print("%s %g Hz %g dB Q %g at %g: deviation %.3e, bound %.3e" % (kind, f, g, q, sr, d, row["bound"]))
    assert d <= row["bound"], (DESIGNS[i], d, row["bound"])


def test_abi_version_stays():
    assert s2.load_library().s2r_abi_version() == 4


def check_ranges(syn):
    """the setters' range checks on a live handle, and the coefficient and state entries on a bus without an EQ (also called by
    tests/test_gpu_eq.py)"""
    L, h = syn.L, syn.h
    assert all(syn.get_bus_eq(b).shape == (0, 5) for b in range(s2.MAX_BUSES))       # a fresh handle: no EQ anywhere
    ok4 = np.ascontiguousarray(_bands(4))
    buf, n = np.zeros(32, dtype=F), C.c_uint32(9)
    for c in bad_bands():
        assert L.s2r_set_bus_eq(h, 0, 1, _p(c)) == s2s.S2R_ERR_PATCH_RANGE, c
    assert L.s2r_set_bus_eq(h, 8, 1, _p(ok4)) == s2s.S2R_ERR_PATCH_RANGE and L.s2r_set_bus_eq(h, 0, 5, _p(buf)) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_eq(h, 0, 2, None) == s2s.S2R_ERR_INVALID
    assert syn.get_bus_eq(0).shape == (0, 5)                     # a refused call changes nothing
    assert L.s2r_set_bus_eq_coeffs(h, 0, 1, _p(ok4)) == s2s.S2R_ERR_INVALID          # no EQ there
    assert L.s2r_get_bus_eq_state(h, 0, _p(buf), 32) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_eq_state(h, 0, _p(buf), 4) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_eq(h, 0, C.byref(n), None, 0) == s2s.S2R_OK and n.value == 0
    assert L.s2r_get_bus_eq(h, 0, None, None, 0) == s2s.S2R_OK
    syn.clear_bus_eq(3)                                          # removing what is not there is no error
    syn.set_bus_eq(3, ok4[:3])
    assert np.array_equal(bits(syn.get_bus_eq(3)), bits(ok4[:3])) and syn.get_bus_eq(0).shape == (0, 5)
    st = syn.bus_eq_state(3)
    assert st.shape == (3, 4) and not bits(st).any()             # +0.0 everywhere right after the EQ is set
    assert L.s2r_get_bus_eq(h, 3, C.byref(n), _p(buf), 14) == s2s.S2R_ERR_INVALID and L.s2r_get_bus_eq(h, 3, C.byref(n), _p(buf), 15) == s2s.S2R_OK
    assert n.value == 3
    for count in (0, 11, 13, 16, 4):
        assert L.s2r_set_bus_eq_state(h, 3, _p(buf), count) == s2s.S2R_ERR_INVALID, count
    assert L.s2r_set_bus_eq_state(h, 3, None, 12) == s2s.S2R_ERR_INVALID
    for cap in (0, 11):
        assert L.s2r_get_bus_eq_state(h, 3, _p(buf), cap) == s2s.S2R_ERR_INVALID, cap
    assert L.s2r_get_bus_eq_state(h, 3, None, 12) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_eq_state(h, 3, _p(buf), 32) == s2s.S2R_OK                   # a larger buffer will do
    new = np.arange(12, dtype=F).reshape(3, 4) - F(5.5)
    syn.set_bus_eq_state(3, new)
    assert np.array_equal(bits(syn.bus_eq_state(3)), bits(new))
    for c in bad_bands():
        three = ok4[:3].copy()
        three[1] = c
        assert L.s2r_set_bus_eq_coeffs(h, 3, 3, _p(three)) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_eq(h, 3, 3, _p(three)) == s2s.S2R_ERR_PATCH_RANGE
    for nb in (1, 2, 4):
        assert L.s2r_set_bus_eq_coeffs(h, 3, nb, _p(ok4)) == s2s.S2R_ERR_INVALID     # another number of bands
    assert L.s2r_set_bus_eq_coeffs(h, 3, 3, None) == s2s.S2R_ERR_INVALID
    assert np.array_equal(bits(syn.get_bus_eq(3)), bits(ok4[:3])) and np.array_equal(bits(syn.bus_eq_state(3)), bits(new))
    syn.set_bus_eq_coeffs(3, ok4[1:])
    assert np.array_equal(bits(syn.get_bus_eq(3)), bits(ok4[1:])) and np.array_equal(bits(syn.bus_eq_state(3)), bits(new))   # the state stays
    syn.set_bus_eq(3, ok4[:1])                                   # setting it again zeroes it
    assert syn.bus_eq_state(3).shape == (1, 4) and not bits(syn.bus_eq_state(3)).any()
    syn.clear_bus_eq(3)
    assert syn.get_bus_eq(3).shape == (0, 5)
    assert L.s2r_get_bus_eq_state(h, 3, _p(buf), 32) == s2s.S2R_ERR_INVALID


if __name__ == "__main__":
    os.makedirs(os.path.dirname(TRUTH), exist_ok=True)
    with open(TRUTH, "w") as fh:
        json.dump(measure(), fh, indent=1)
        fh.write("\n")
    print("wrote", TRUTH)
