"""The per-bus dynamics, the host side: s2r_dynamics_reference — the rule restated in plain C++ — held against a numpy
float32 model of the rule written here (np_dyn: a loop over frames), the table lookup at every breakpoint and at the ends of the level
range, the ballistics (y >= 0; a^n on a step of the key, inside a bound derived from the three roundings of a step; which coefficient
is taken), s2r_dynamics_curve against its formula in numpy float64 (np_curve), s2r_dynamics_coef against numpy, and the range checks
of the entry points, which answer without a device.  Comparisons of signals and gains are on bits (helpers.assert_bits_equal_finite).

Run as a program (PYTHONPATH=.:tests python tests/test_dyn_host.py, from the repository's root) this file measures how far the numpy
model's interpolated table is from the exact curve between the breakpoints, and writes that and twice that — the bound the library is
held to — into profiles/truth/dynamics_curve_deviation.json."""
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
TRUTH = os.path.join(ROOT, "profiles", "truth", "dynamics_curve_deviation.json")
F = np.float32
NAN = float("nan")
INF = float("inf")
M32 = 0xFFFFFFFF
P = s2.DYN_CURVE_POINTS
LO = 0x33800000                                                  # the bits of 2^-24
U = 2.0 ** -24                                                   # binary32's unit roundoff
# (threshold_db, ratio, knee_db, makeup_db): hard and soft knees, a gentle ratio, a limiter, makeup, thresholds on and off a breakpoint
DESIGNS = [(-20.0, 4.0, 0.0, 0.0), (-18.0, 2.0, 6.0, 3.0), (-30.0, INF, 0.0, 0.0), (-12.0, 8.0, 12.0, 6.0), (-40.0, 1.5, 3.0, -2.0),
           (20.0 * float(np.log10(0.125)), 10.0, 0.0, 0.0), (-6.0, 20.0, 1.0, 12.0), (-24.0, 1.0, 4.0, 0.0)]


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def _p(a):
    return a.ctypes.data_as(s2s._f32p)


def levels():
    """the level of every breakpoint, exact in binary32 (and in float64)"""
    j = np.arange(P)
    return np.ldexp(1.0 + (j % 16) / 16.0, -24 + j // 16)


def np_target(curve, p):
    """the rule's step 2 for one level p (np.float32): one subtraction, one product, one sum, each a float32 operation"""
    if not p >= F(2.0 ** -24):
        return curve[0]
    if p >= F(256.0):
        return curve[P - 1]
    u = int(np.array(p, dtype=F).view(np.uint32)) - LO
    i, f = u >> 19, F(u & 0x7FFFF) * F(2.0 ** -19)
    return curve[i] + f * (curve[i + 1] - curve[i])


def np_dyn(curve, a_att, a_rel, key, x, y):
    """the rule in numpy float32: a loop over frames.  curve [P], key and x [frames, 2], y the gain carried in; returns (out [frames,
    2], the gain after the call, the minimum of the gain over the call, the targets [frames], the gains [frames])"""
    curve, key, x = np.asarray(curve, dtype=F), np.asarray(key, dtype=F), np.asarray(x, dtype=F)
    a_att, a_rel, y = F(a_att), F(a_rel), F(y)
    out, ts, ys = np.empty_like(x), np.empty(x.shape[0], dtype=F), np.empty(x.shape[0], dtype=F)
    mn = F(np.inf)
    with np.errstate(under="ignore"):
        for n in range(x.shape[0]):
            l, r = np.abs(key[n, 0]), np.abs(key[n, 1])
            t = np_target(curve, l if l > r else r)
            a = a_att if t < y else a_rel
            y = t + a * (y - t)
            mn = y if y < mn else mn
            out[n] = x[n] * y
            ts[n], ys[n] = t, y
    assert out.dtype == F and type(y) is F and ys.dtype == F
    return out, y, mn, ts, ys


def exact_gain(level, threshold_db, ratio, knee_db, makeup_db):
    """s2r.h's formula at any level, in float64 (numpy arrays)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        o = 20.0 * np.log10(level) - threshold_db
        slope, W = 1.0 / ratio - 1.0, knee_db
        knee = slope * (o + W / 2.0) ** 2 / (2.0 * W) if W > 0.0 else np.zeros_like(o)
        G = np.where(2.0 * o < -W, 0.0, np.where((W > 0.0) & (2.0 * np.abs(o) <= W), knee, slope * o))
    return np.power(10.0, (G + makeup_db) / 20.0)


def np_curve(threshold_db, ratio, knee_db, makeup_db):
    """the table in float64: the formula at every breakpoint"""
    return exact_gain(levels(), threshold_db, ratio, knee_db, makeup_db)


def between():
    """levels at a quarter, a half and three quarters of every segment, exact in binary32: [512 * 3] float32"""
    u = (LO + (np.arange(P - 1, dtype=np.uint64)[:, None] << 19) + (np.arange(1, 4, dtype=np.uint64)[None, :] << 17)).astype(np.uint32)
    return u.reshape(-1).view(F)


def table_deviation(curve, design, target):
    """the largest relative distance of target(curve, level) from the exact curve over between()"""
    lv = between()
    got = np.array([float(target(curve, p)) for p in lv])
    want = exact_gain(lv.astype(np.float64), *design)
    return float(np.max(np.abs(got - want) / want))


def reference_target(curve, p):
    """the library's step 2 alone: zero coefficients make the gain the target, and x = 1 makes the output the gain"""
    one = np.ones((1, 2), dtype=F)
    out, y, _ = s2.dynamics_reference(curve, 0.0, 0.0, np.array([[p, 0.0]], dtype=F), one, curve[0])
    assert bits(out[0, 0]) == bits(y)
    return y


def measure():
    rows = []
    for d in DESIGNS:
        dev = table_deviation(np_curve(*d).astype(F), d, np_target)
        rows.append({"threshold_db": d[0], "ratio": d[1] if np.isfinite(d[1]) else "inf", "knee_db": d[2], "makeup_db": d[3], "reference_deviation": dev,
                     "bound": 2.0 * dev})
    return {"what": "largest relative deviation, at a quarter, a half and three quarters of each of the 512 segments, of the numpy float32 model's "
                    "interpolated gain (table = the formula in numpy float64 rounded to binary32) from the exact curve of s2r_dynamics_curve's "
                    "formula; bound = 2 x that; s2r_dynamics_reference over s2r_dynamics_curve's table is held to the bound (tests/test_dyn_host.py)",
            "designs": rows}


def _signal(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((n, 2)) * scale).astype(F)


def _random_curve(seed):
    """513 gains with nothing regular about them: zeros, the top of the range and values in between"""
    c = (np.random.default_rng(seed).random(P) * 2.0).astype(F)
    c[::37] = 0.0
    c[5::61] = 256.0
    return c


COMP = (-20.0, 4.0, 6.0, 3.0)


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("frames", [0, 1, 2, 5, 1000])
def test_reference_is_the_numpy_model(frames, cross):
    curve = s2.dynamics_curve(*COMP) if frames != 5 else _random_curve(3)
    x = _signal(frames, frames + 1, 0.5)
    key = _signal(frames, frames + 77, 0.25) if cross else x
    a_att, a_rel = s2.dynamics_coef(1.0, 48000.0), s2.dynamics_coef(100.0, 48000.0)
    y0 = curve[0] if frames % 2 == 0 else F(0.3)
    want, y_want, mn_want, ts, ys = np_dyn(curve, a_att, a_rel, key, x, y0)
    got, y_got, mn_got = s2.dynamics_reference(curve, a_att, a_rel, key if cross else None, x, y0)
    assert_bits_equal_finite(got, want, "%d frames: the output" % frames)
    assert bits(y_got) == bits(y_want)
    if frames:
        assert bits(mn_got) == bits(mn_want) == bits(ys.min())
    else:
        assert np.isinf(mn_got) and bits(y_got) == bits(y0)
    if frames == 1000:
        assert bits(got).any() and not np.array_equal(bits(got), bits(x))
        assert (ts < ys).sum() >= 30 and (ts > ys).sum() >= 30     # both branches of the ballistics


def test_two_calls_are_one():
    curve = s2.dynamics_curve(*COMP)
    x, key = _signal(337, 5, 0.5), _signal(337, 6, 0.5)
    a = (F(0.9), F(0.999))
    whole, y_whole, mn_whole = s2.dynamics_reference(curve, a[0], a[1], key, x, curve[0])
    for cut in (0, 1, 2, 100, 336, 337):
        o1, y1, m1 = s2.dynamics_reference(curve, a[0], a[1], key[:cut], x[:cut], curve[0])
        o2, y2, m2 = s2.dynamics_reference(curve, a[0], a[1], key[cut:], x[cut:], y1)
        assert_bits_equal_finite(np.concatenate([o1, o2]), whole, "cut at %d" % cut)
        assert bits(y2) == bits(y_whole) and bits(min(m1, m2)) == bits(mn_whole)


def test_a_level_at_a_breakpoint_returns_its_entry():
    """all 513: with zero coefficients the gain is the target, and a key exactly at breakpoint j reads curve[j] in every bit — on either
    channel and under either sign"""
    curve = _random_curve(11)
    lv = levels().astype(F)
    assert np.array_equal(lv.astype(np.float64), levels()) and np.array_equal(bits(lv), LO + (np.arange(P, dtype=np.uint32) << 19))
    key = np.zeros((P, 2), dtype=F)
    key[::2, 0], key[1::2, 1] = lv[::2], -lv[1::2]
    out, y, mn = s2.dynamics_reference(curve, 0.0, 0.0, key, np.ones((P, 2), dtype=F), curve[0])
    assert_bits_equal_finite(out[:, 0], curve, "the gain at each breakpoint")
    assert_bits_equal_finite(out[:, 1], curve, "the other channel: linked")
    assert bits(y) == bits(curve[P - 1]) and mn == curve.min()


def test_the_ends_of_the_level_range():
    curve = _random_curve(12)
    below = np.nextafter(F(2.0 ** -24), F(0.0))
    for p in (F(0.0), F(-0.0), F(1e-45), F(1e-40), below):
        assert bits(reference_target(curve, p)) == bits(curve[0]), p
    for p in (F(256.0), np.nextafter(F(256.0), F(1e9)), F(1e10), np.finfo(F).max):
        assert bits(reference_target(curve, p)) == bits(curve[P - 1]), p
    # the last level below 2^8 still interpolates inside the last segment
    p = np.nextafter(F(256.0), F(0.0))
    assert bits(reference_target(curve, p)) == bits(np_target(curve, p))
    assert bits(reference_target(curve, F(2.0 ** -24))) == bits(curve[0])


def test_zero_coefficients_make_the_output_x_times_the_target():
    curve = s2.dynamics_curve(-30.0, INF, 0.0, 0.0)
    x, key = _signal(500, 21, 0.5), _signal(500, 22, 0.3)
    out, y, mn = s2.dynamics_reference(curve, 0.0, 0.0, key, x, F(7.0))
    t = np.array([np_target(curve, max(abs(k[0]), abs(k[1]))) for k in key], dtype=F)
    assert_bits_equal_finite(out, x * t[:, None], "x * t")
    assert bits(y) == bits(t[-1]) and bits(mn) == bits(t.min()) and (t < 1.0).sum() > 100


def test_the_gain_stays_non_negative():
    """from any finite state >= 0: with t >= 0 and 0 <= a < 1, fl(a * fl(y - t)) is no larger in magnitude than fl(y - t), which is no
    larger than t when y < t — so fl(t + m) >= 0.  (No upper bound is claimed.)"""
    rng = np.random.default_rng(31)
    for y0 in (0.0, 1e-45, 1e-30, 0.5, 255.0, 1e30, float(np.finfo(F).max)):
        for a in ((0.0, 0.0), (0.5, 0.999999), (float(np.nextafter(F(1.0), F(0.0))),) * 2):
            curve = _random_curve(int(rng.integers(1 << 30)))
            key = (rng.standard_normal((400, 2)) * 10.0 ** rng.uniform(-8, 3, (400, 1))).astype(F)
            out, y, mn = s2.dynamics_reference(curve, a[0], a[1], key, np.ones((400, 2), dtype=F), F(y0))
            assert np.isfinite(out).all() and (out >= 0.0).all() and y >= 0.0 and mn >= 0.0, (y0, a)


def test_attack_and_release_follow_a_to_the_n():
    """a step in the key: 0 dB for 400 frames, then -60 dB.  With e = y - t the rule is e' = a e in exact arithmetic; computed, d = (y -
    t)(1 + d1), m = a d (1 + d2), y' = (t + m)(1 + d3) with |d| <= u = 2^-24, so e' = a e (1 + d1)(1 + d2) + (t + m) d3 and, t + m
    lying between t and y, |e' - a e| <= a |e| (2u + u^2) + max(t, y) u.  The bound below carries that through the steps."""
    curve = s2.dynamics_curve(-20.0, 4.0, 0.0, 0.0)
    a_att, a_rel = s2.dynamics_coef(1.0, 48000.0), s2.dynamics_coef(5.0, 48000.0)
    key = np.full((800, 2), 1.0, dtype=F)
    key[400:] = 0.001
    out, _, _ = s2.dynamics_reference(curve, a_att, a_rel, key, np.ones((800, 2), dtype=F), curve[0])
    ys = out[:, 0].astype(np.float64)
    t_hi, t_lo = float(reference_target(curve, F(1.0))), float(reference_target(curve, F(0.001)))
    assert t_hi < 0.2 and t_lo == 1.0 == float(curve[0])
    for t, a, y_in, seg in ((t_hi, float(a_att), 1.0, ys[:400]), (t_lo, float(a_rel), ys[399], ys[400:])):
        e, dev, big = y_in - t, 0.0, max(t, y_in)
        for n in range(400):
            dev = a * (1.0 + 2.0 * U + U * U) * dev + a * abs(e) * (2.0 * U + U * U) + big * U
            e *= a
            assert abs((seg[n] - t) - e) <= dev, (t, n, seg[n] - t, e, dev)
        assert dev < 1e-4 and abs(e) < 0.2 * abs(y_in - t)        # the bound is tight, and the segment is long enough to tell a from another a


def test_the_attack_coefficient_is_taken_exactly_when_the_target_is_below_the_gain():
    """values whose arithmetic is exact: from y = 0.5, a target of 0.25 (below: attack, 0.25) gives 0.25 + 0.25 * 0.25; a target of 1
    (above: release, 0.75) gives 1 + 0.75 * (y - 1); a target equal to the gain keeps it under either"""
    curve = np.full(P, 1.0, dtype=F)
    lv = levels().astype(F)
    curve[400], curve[410], curve[420] = 0.25, 1.0, 0.3125
    key = np.array([[lv[400], 0.0], [lv[410], 0.0], [lv[420], 0.0], [lv[420], 0.0]], dtype=F)
    one = np.ones((1, 2), dtype=F)
    o, y, _ = s2.dynamics_reference(curve, 0.25, 0.75, key[0:1], one, F(0.5))
    assert y == F(0.3125) and o[0, 0] == y
    o, y, _ = s2.dynamics_reference(curve, 0.25, 0.75, key[1:2], one, F(0.5))
    assert y == F(0.625)
    o, y, _ = s2.dynamics_reference(curve, 0.25, 0.75, key[2:3], one, F(0.3125))
    assert y == F(0.3125)
    o, y, mn = s2.dynamics_reference(curve, 0.25, 0.75, key, np.ones((4, 2), dtype=F), F(0.5))
    assert np.array_equal(o[:, 0], np.array([0.3125, 0.484375, 0.35546875, 0.3232421875], dtype=F))
    assert mn == F(0.3125)


def _adjacent(a, b):
    def key(v):
        u = int(bits(v).reshape(-1)[0])
        return u if u < 0x80000000 else 0x80000000 - u
    return abs(key(a) - key(b)) <= 1


@pytest.mark.parametrize("design", DESIGNS)
def test_curve_is_the_formula_in_float64(design):
    """each entry equal or adjacent in binary32 to the numpy float64 formula rounded once (the two libms may differ in the last place
    before the one rounding); exactly the makeup below the knee; never rising with the level"""
    got = s2.dynamics_curve(*design)
    want = np_curve(*design).astype(F)
    assert got.dtype == F and got.shape == (P,)
    for j in range(P):
        assert _adjacent(got[j], want[j]), (design, j, float(got[j]), float(want[j]))
    t, ratio, knee, makeup = design
    flat = 20.0 * np.log10(levels()) - t < -knee / 2.0 - 1e-9
    assert flat.sum() > 16 and (bits(got[flat]) == bits(F(10.0 ** (makeup / 20.0)))).all()
    assert (np.diff(got) <= 0.0).all()
    if ratio > 1.0:
        assert got[P - 1] < got[0]


def test_a_limiter_curve_holds_the_threshold():
    """ratio inf, no knee: above the threshold the gain times the level is the threshold"""
    curve = s2.dynamics_curve(-20.0, INF, 0.0, 0.0).astype(np.float64)
    lv = levels()
    above = lv > 0.1
    assert above.sum() > 100 and np.allclose(curve[above] * lv[above], 0.1, rtol=1e-6)
    assert (curve[~above] == 1.0).all()


def test_coef_is_numpy():
    for ms, sr in [(1.0, 48000.0), (100.0, 48000.0), (0.01, 44100.0), (5000.0, 96000.0), (10.0, 8000.0)]:
        got = s2.dynamics_coef(ms, sr)
        assert type(got) is F and _adjacent(got, F(np.exp(-1.0 / (ms * 0.001 * sr)))), (ms, sr)
        assert 0.0 <= got < 1.0 or ms == 5000.0
    assert bits(s2.dynamics_coef(0.0, 48000.0)) == 0
    for ms, sr in [(-1.0, 48000.0), (1.0, 0.0), (1.0, -1.0), (NAN, 48000.0), (1.0, NAN)]:
        assert np.isnan(s2.dynamics_coef(ms, sr))


def test_the_committed_bounds_are_the_measurement():
    doc = json.load(open(TRUTH))
    assert [(r["threshold_db"], float(r["ratio"]), r["knee_db"], r["makeup_db"]) for r in doc["designs"]] == DESIGNS
    for r in doc["designs"]:
        assert r["bound"] == 2.0 * r["reference_deviation"] and 0.0 <= r["reference_deviation"] < 2e-2, r


@pytest.mark.parametrize("i", range(len(DESIGNS)))
def test_interpolated_curve_between_the_breakpoints(i):
    """the library's table read by the library's rule, between the breakpoints, is as close to the exact curve as twice the numpy
    model's own deviation (measured on the CPU, committed): sixteen chords per octave of a power law, and a knee wherever it falls"""
    row = json.load(open(TRUTH))["designs"][i]
    curve = s2.dynamics_curve(*DESIGNS[i])
    lv = between()
    key = np.stack([lv, np.zeros_like(lv)], axis=1)
    out, _, _ = s2.dynamics_reference(curve, 0.0, 0.0, key, np.ones_like(key), curve[0])
    want = exact_gain(lv.astype(np.float64), *DESIGNS[i])
    d = float(np.max(np.abs(out[:, 0].astype(np.float64) - want) / want))
    print("%s: deviation %.3e, bound %.3e" % (DESIGNS[i], d, row["bound"]))
    assert d <= row["bound"], (DESIGNS[i], d, row["bound"])


def bad_curves():
    out = []
    for j in (0, 1, 255, 512):
        for v in (NAN, INF, -INF, -1e-30, -1.0, float(np.nextafter(F(256.0), F(1e9))), 1e30):
            c = np.ones(P, dtype=F)
            c[j] = v
            out.append(c)
    return out


BAD_COEFS = [NAN, INF, -INF, 1.0, -1e-30, -0.5, 2.0, float(np.nextafter(F(1.0), F(2.0)))]
GOOD_COEFS = [0.0, 0.5, float(np.nextafter(F(1.0), F(0.0)))]


def test_range_errors_without_a_handle():
    """every entry looks at the values before it looks at the handle, so the range checks answer without a device, and a refused
    reference call leaves gain and output alone; S2R_ERR_INVALID is what no handle gets for values in range"""
    L = s2.load_library()
    ok = np.ascontiguousarray(s2.dynamics_curve(*COMP))
    top = np.full(P, 256.0, dtype=F)
    top[::2] = 0.0
    for setter in (L.s2r_set_bus_dynamics, L.s2r_set_bus_dynamics_params):
        for c in bad_curves():
            assert setter(None, 0, 0, _p(c), 0.5, 0.5) == s2s.S2R_ERR_PATCH_RANGE
        for a in BAD_COEFS:
            assert setter(None, 0, 0, _p(ok), a, 0.5) == s2s.S2R_ERR_PATCH_RANGE, a
            assert setter(None, 0, 0, _p(ok), 0.5, a) == s2s.S2R_ERR_PATCH_RANGE, a
        for bus in (8, 255, M32):
            assert setter(None, bus, 0, _p(ok), 0.5, 0.5) == s2s.S2R_ERR_PATCH_RANGE
            assert setter(None, 0, bus, _p(ok), 0.5, 0.5) == s2s.S2R_ERR_PATCH_RANGE
        for a in GOOD_COEFS:
            assert setter(None, 7, 7, _p(top), a, a) == s2s.S2R_ERR_INVALID, a
        assert setter(None, 0, 0, None, 0.5, 0.5) == s2s.S2R_ERR_INVALID
    assert L.s2r_clear_bus_dynamics(None, 8) == s2s.S2R_ERR_PATCH_RANGE and L.s2r_clear_bus_dynamics(None, 0) == s2s.S2R_ERR_INVALID
    buf, n = np.zeros(P, dtype=F), C.c_uint32(5)
    assert L.s2r_get_bus_dynamics(None, 8, C.byref(n), None, _p(buf), P, None, None) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_dynamics(None, 0, C.byref(n), None, _p(buf), P, None, None) == s2s.S2R_ERR_INVALID and n.value == 5
    assert L.s2r_get_bus_dynamics_meter(None, 8, _p(buf)) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_dynamics_meter(None, 0, _p(buf)) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_dynamics_state(None, 8, _p(buf), 1) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_dynamics_state(None, 8, _p(buf), 1) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_dynamics_state(None, 0, _p(buf), 1) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_dynamics_state(None, 0, _p(buf), 1) == s2s.S2R_ERR_INVALID
    for v in (NAN, INF, -1.0, -1e-45):
        assert L.s2r_set_bus_dynamics_state(None, 0, _p(np.array([v], dtype=F)), 1) == s2s.S2R_ERR_PATCH_RANGE, v
    # the reference: a refusal changes neither the gain nor the output
    x, y, out, mn = _signal(3, 1), np.array([0.5], dtype=F), np.full((3, 2), 9.0, dtype=F), np.array([9.0], dtype=F)
    ref = L.s2r_dynamics_reference
    for c in bad_curves():
        assert ref(_p(c), 0.5, 0.5, _p(x), _p(x), 3, _p(y), _p(out), _p(mn)) == s2s.S2R_ERR_PATCH_RANGE
    for a in BAD_COEFS:
        assert ref(_p(ok), a, 0.5, _p(x), _p(x), 3, _p(y), _p(out), _p(mn)) == s2s.S2R_ERR_PATCH_RANGE
        assert ref(_p(ok), 0.5, a, _p(x), _p(x), 3, _p(y), _p(out), _p(mn)) == s2s.S2R_ERR_PATCH_RANGE
    for v in (NAN, INF, -1.0):
        assert ref(_p(ok), 0.5, 0.5, _p(x), _p(x), 3, _p(np.array([v], dtype=F)), _p(out), _p(mn)) == s2s.S2R_ERR_PATCH_RANGE
    assert ref(None, 0.5, 0.5, _p(x), _p(x), 3, _p(y), _p(out), _p(mn)) == s2s.S2R_ERR_INVALID
    assert ref(_p(ok), 0.5, 0.5, _p(x), _p(x), 3, None, _p(out), _p(mn)) == s2s.S2R_ERR_INVALID
    assert ref(_p(ok), 0.5, 0.5, _p(x), None, 3, _p(y), _p(out), _p(mn)) == s2s.S2R_ERR_INVALID
    assert y[0] == 0.5 and (out == 9.0).all() and mn[0] == 9.0
    assert ref(_p(ok), 0.5, 0.5, None, None, 0, _p(y), None, _p(mn)) == s2s.S2R_OK and y[0] == 0.5 and mn[0] == 9.0   # no frames: nothing moves
    assert ref(_p(ok), 0.5, 0.5, None, _p(x), 3, _p(y), None, None) == s2s.S2R_OK         # a NULL key: the bus keys itself; no output, no meter
    assert bits(y[0]) == bits(np_dyn(ok, 0.5, 0.5, x, x, 0.5)[1])
    with pytest.raises(ValueError):
        s2.dynamics_reference(ok[:-1], 0.5, 0.5, None, x, 0.5)
    with pytest.raises(s2.S2rError) as err:
        s2.dynamics_reference(ok, 1.0, 0.5, None, x, 0.5)
    assert err.value.status == s2s.S2R_ERR_PATCH_RANGE
    assert s2.Synth.dynamics_reference(ok, 0.5, 0.5, None, x, 0.5)[0].shape == (3, 2)
    syn = _new_or_skip(num_voices=8, max_frames=64)              # with a device the rest runs on a real handle
    if syn is not None:
        check_ranges(syn)


def test_curve_range_checks():
    L = s2.load_library()
    out = np.full(P, 9.0, dtype=F)
    bad = [(NAN, 4.0, 0.0, 0.0), (-20.0, NAN, 0.0, 0.0), (-20.0, 4.0, NAN, 0.0), (-20.0, 4.0, 0.0, NAN), (-20.0, 0.999, 0.0, 0.0), (-20.0, 0.0, 0.0, 0.0),
           (-20.0, -4.0, 0.0, 0.0), (-20.0, 4.0, -0.001, 0.0), (-20.0, 4.0, 0.0, 49.0),     # (a makeup past 2^8)
           (-20.0, 4.0, 0.0, INF), (-INF, 1.0, 0.0, 0.0), (-20.0, 4.0, INF, 0.0)]      # (entries that are not finite)
    for d in bad:
        assert L.s2r_dynamics_curve(*d, _p(out)) == s2s.S2R_ERR_PATCH_RANGE, d
    assert (out == 9.0).all()
    assert L.s2r_dynamics_curve(-20.0, 4.0, 0.0, 0.0, None) == s2s.S2R_ERR_INVALID
    for d in DESIGNS + [(INF, 4.0, 0.0, 0.0), (-150.0, INF, 0.0, 40.0), (50.0, 1.0, 0.0, 48.0), (0.0, INF, 100.0, -200.0)]:
        assert L.s2r_dynamics_curve(*d, _p(out)) == s2s.S2R_OK, d
        assert L.s2r_set_bus_dynamics(None, 0, 0, _p(out), 0.5, 0.5) == s2s.S2R_ERR_INVALID     # what comes back the setter takes
    with pytest.raises(s2.S2rError) as err:
        s2.dynamics_curve(-20.0, 0.5)
    assert err.value.status == s2s.S2R_ERR_PATCH_RANGE


def test_abi_version_stays():
    assert s2.load_library().s2r_abi_version() == 4


def check_ranges(syn):
    """the setters' range checks on a live handle, and the parameter, state and meter entries on a bus without dynamics (also called by
    tests/test_gpu_dyn.py)"""
    L, h = syn.L, syn.h
    assert all(syn.get_bus_dynamics(b) is None for b in range(s2.MAX_BUSES))      # a fresh handle: no dynamics anywhere
    ok, other = np.ascontiguousarray(s2.dynamics_curve(*COMP)), _random_curve(8)
    buf = np.zeros(P + 4, dtype=F)
    for c in bad_curves()[:6]:
        assert L.s2r_set_bus_dynamics(h, 0, 0, _p(c), 0.5, 0.5) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_dynamics(h, 8, 0, _p(ok), 0.5, 0.5) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_dynamics(h, 0, 8, _p(ok), 0.5, 0.5) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_dynamics(h, 0, 0, _p(ok), 1.0, 0.5) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_dynamics(h, 0, 0, None, 0.5, 0.5) == s2s.S2R_ERR_INVALID
    assert syn.get_bus_dynamics(0) is None                       # a refused call changes nothing
    assert L.s2r_set_bus_dynamics_params(h, 0, 0, _p(ok), 0.5, 0.5) == s2s.S2R_ERR_INVALID          # none there
    assert L.s2r_get_bus_dynamics_state(h, 0, _p(buf), 4) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_dynamics_state(h, 0, _p(buf), 1) == s2s.S2R_ERR_INVALID
    assert syn.bus_dynamics_meter(0) == 1.0
    syn.clear_bus_dynamics(3)                                    # removing what is not there is no error
    syn.set_bus_dynamics(3, 5, other, 0.25, 0.75)
    key, curve, a_att, a_rel = syn.get_bus_dynamics(3)
    assert key == 5 and np.array_equal(bits(curve), bits(other)) and (a_att, a_rel) == (F(0.25), F(0.75)) and syn.get_bus_dynamics(0) is None
    assert bits(syn.bus_dynamics_state(3)) == bits(other[0])     # the gain at silence right after a set
    assert syn.bus_dynamics_meter(3) == 1.0                      # no call yet
    n = C.c_uint32(0)
    assert L.s2r_get_bus_dynamics(h, 3, C.byref(n), None, _p(buf), P - 1, None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_dynamics(h, 3, C.byref(n), None, None, 0, None, None) == s2s.S2R_OK and n.value == 1
    for count in (0, 2, 4):
        assert L.s2r_set_bus_dynamics_state(h, 3, _p(buf), count) == s2s.S2R_ERR_INVALID, count
    assert L.s2r_set_bus_dynamics_state(h, 3, None, 1) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_dynamics_state(h, 3, _p(buf), 0) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_dynamics_state(h, 3, None, 1) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_dynamics_state(h, 3, _p(buf), 4) == s2s.S2R_OK                 # a larger buffer will do
    for v in (NAN, INF, -1.0):
        with pytest.raises(s2.S2rError) as err:
            syn.set_bus_dynamics_state(3, v)
        assert err.value.status == s2s.S2R_ERR_PATCH_RANGE
    syn.set_bus_dynamics_state(3, 0.125)
    assert syn.bus_dynamics_state(3) == F(0.125)
    for c in bad_curves()[:6]:
        assert L.s2r_set_bus_dynamics_params(h, 3, 5, _p(c), 0.25, 0.75) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_dynamics_params(h, 3, 5, None, 0.25, 0.75) == s2s.S2R_ERR_INVALID
    assert np.array_equal(bits(syn.get_bus_dynamics(3)[1]), bits(other)) and syn.bus_dynamics_state(3) == F(0.125)
    syn.set_bus_dynamics_params(3, 2, ok, 0.5, 0.0)
    key, curve, a_att, a_rel = syn.get_bus_dynamics(3)
    assert key == 2 and np.array_equal(bits(curve), bits(ok)) and (a_att, a_rel) == (F(0.5), F(0.0))
    assert syn.bus_dynamics_state(3) == F(0.125)                 # the gain stays
    syn.set_bus_dynamics(3, 3, ok, 0.5, 0.5)                     # setting them again resets it
    assert bits(syn.bus_dynamics_state(3)) == bits(ok[0])
    syn.clear_bus_dynamics(3)
    assert syn.get_bus_dynamics(3) is None
    assert L.s2r_get_bus_dynamics_state(h, 3, _p(buf), 4) == s2s.S2R_ERR_INVALID


if __name__ == "__main__":
    os.makedirs(os.path.dirname(TRUTH), exist_ok=True)
    with open(TRUTH, "w") as fh:
        json.dump(measure(), fh, indent=1)
        fh.write("\n")
    print("wrote", TRUTH)
