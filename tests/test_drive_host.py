"""The per-bus drive's rule on the host (s2r.h: s2r_set_bus_drive), no device needed: s2r_drive_reference against a
numpy float32 model that walks the rule — up to four times the rate through g = 4 h, the table by sign and magnitude, back down
through h, every product and sum rounded on its own and every sum from +0.0 in index order —, fed the taps the library reports; the
rule's consequences (the 16 frames of latency, concatenation, the clamp, the grid, the history's layout); the designed curves against
their formulas in binary64; every range check without a handle; and what the stage is for: the aliasing it avoids.

Run as a program it measures how far the float32 model is from a binary64 run of the same rule on a signal of magnitude 1e-6 and
what the oversampling buys on a clipped 5 kHz sine, and writes both to profiles/truth/drive_deviation.json, and the designed curves'
distance from numpy's to profiles/truth/drive_curve_deviation.json."""
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
TRUTH = os.path.join(ROOT, "profiles", "truth", "drive_deviation.json")
CURVE_TRUTH = os.path.join(ROOT, "profiles", "truth", "drive_curve_deviation.json")
F = np.float32
NAN, INF = float("nan"), float("inf")
M32 = 0xffffffff
H, LAT, TAPS, POINTS = s2.DRIVE_HISTORY, s2.DRIVE_LATENCY, s2.DRIVE_TAPS, s2.DRIVE_CURVE_POINTS
KINDS = [("linear", s2.DRIVE_LINEAR, 1.0), ("tanh", s2.DRIVE_TANH, 3.0), ("hard", s2.DRIVE_HARD, 2.0), ("cubic", s2.DRIVE_CUBIC, 1.5),
         ("fold", s2.DRIVE_FOLD, 3.5)]
FRAMES = [0, 1, 2, 5, 15, 16, 17, 31, 32, 33, 1000]
SMALL = dict(frames=2000, seed=21, magnitude=1e-6)               # the small-signal case of drive_deviation.json
ALIAS = dict(rate=48000, tone=5000, frames=4800, lead=64, pre=8.0)


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f(v):
    return C.c_float(float(F(v)))


def _signal(frames, seed, scale=0.5):
    return (np.random.default_rng(seed).standard_normal((frames, 2)) * scale).astype(F)


def random_table(seed=5):
    """finite, asymmetric, nothing regular about it"""
    r = np.random.default_rng(seed)
    return (np.cumsum(r.standard_normal(POINTS)) * 0.05 + r.standard_normal(POINTS) * 0.01).astype(F)


def np_drive(T, h32, curve, pre, dry, wet, x, hist):
    """the rule in numpy at precision T, a loop over its indices: one array operation is one rounded operation per frame.  h32: the
    taps as the library reports them; returns (out [frames, 2], the history after the call)"""
    h = np.asarray(h32, dtype=F).astype(T)
    g = (F(4.0) * np.asarray(h32, dtype=F)).astype(T)            # exact in binary32
    curve = np.asarray(curve, dtype=F).astype(T)
    pre, dry, wet = T(F(pre)), T(F(dry)), T(F(wet))
    x = np.asarray(x, dtype=F).astype(T)
    n = x.shape[0]
    out = np.zeros((n, 2), dtype=T)
    new = np.zeros((H, 2), dtype=T)
    nf = n + LAT                                                  # frames q = -16 .. n - 1 whose four phases the call needs
    for c in range(2):
        xs = np.concatenate([np.asarray(hist, dtype=F)[:, c].astype(T), x[:, c]])         # frame q at H + q
        w = np.zeros((nf, 4), dtype=T)
        for p in range(4):
            u = np.zeros(nf, dtype=T)
            j = 0
            while p + 4 * j <= 64:
                u = u + g[p + 4 * j] * xs[LAT - j:LAT - j + nf]                           # x[q - j], q = f - 16, sits at f + 16 - j
                j += 1
            t = pre * u
            at = np.abs(t)
            m = np.where(at < T(1.0), at, T(1.0))
            a = m * T(512.0)
            i = np.minimum(a.astype(np.uint32), 511).astype(np.int64)
            fr = a - i.astype(T)
            neg = t < T(0.0)
            c0 = curve[np.where(neg, 512 - i, 512 + i)]
            c1 = curve[np.where(neg, 511 - i, 513 + i)]
            w[:, p] = c0 + fr * (c1 - c0)
        wf = w.reshape(-1)                                        # w[m] at m + 64
        v = np.zeros(n, dtype=T)
        for k in range(TAPS):
            v = v + h[k] * wf[64 - k::4][:n]                      # w[4 n - k]
        out[:, c] = dry * xs[LAT:LAT + n] + wet * v               # x[n - 16]
        new[:, c] = xs[n:n + H]
    return out, new


def taps():
    return s2.drive_taps()


def table(kind_row):
    return s2.drive_curve(kind_row[1], kind_row[2])


def ref(curve, pre, dry, wet, x, hist=None):
    return s2.drive_reference(curve, pre, dry, wet, x, hist)


def deviation(out, want):
    """the largest distance from the binary64 evaluation, as a fraction of its peak"""
    return float(np.max(np.abs(np.asarray(out, dtype=np.float64) - want)) / np.max(np.abs(want)))


def small_signal():
    r = np.random.default_rng(SMALL["seed"])
    return (r.standard_normal((SMALL["frames"], 2)) * SMALL["magnitude"]).astype(F)


def inharmonic_db(y, strict):
    """the energy of a Hann-windowed 4800-frame FFT at the bins that are not multiples of 5 kHz, in dB re the whole spectrum's.  Bins are
    10 Hz apart.  strict: the two bins beside each multiple are left out too — a Hann window puts a whole-period partial on exactly
    those three bins, so they hold the harmonics' energy and nothing aliased."""
    n = ALIAS["frames"]
    sp = np.abs(np.fft.rfft(np.asarray(y, dtype=np.float64) * np.hanning(n + 1)[:n])) ** 2
    k = np.arange(sp.size) % (ALIAS["tone"] * n // ALIAS["rate"])
    keep = (k != 0) if not strict else ((k > 1) & (k < ALIAS["tone"] * n // ALIAS["rate"] - 1))
    return float(10.0 * np.log10(sp[keep].sum() / sp.sum()))


def alias_figures(T):
    """(naive, through the rule at precision T or the library's reference for T None), each (plain, strict) in dB: a 5 kHz sine of
    amplitude 1 at 48 kHz through the hard clip at pre 8, against clipping the same sine at the bus rate"""
    n, lead = ALIAS["frames"], ALIAS["lead"]
    t = np.arange(n + lead, dtype=np.float64)
    s = np.sin(2.0 * np.pi * ALIAS["tone"] / ALIAS["rate"] * t).astype(F)
    x = np.stack([s, s], axis=1)
    curve = s2.drive_curve(s2.DRIVE_HARD, 1.0)
    zero = np.zeros((H, 2), dtype=F)
    if T is None:
        y = ref(curve, ALIAS["pre"], 0.0, 1.0, x)[0][lead:, 0]
    else:
        y = np_drive(T, taps(), curve, ALIAS["pre"], 0.0, 1.0, x, zero)[0][lead:, 0]
    naive = np.clip(F(ALIAS["pre"]) * s, F(-1.0), F(1.0))[lead:]
    return tuple(inharmonic_db(naive, st) for st in (False, True)), tuple(inharmonic_db(y, st) for st in (False, True))


def measure():
    x = small_signal()
    lin = s2.drive_curve(s2.DRIVE_LINEAR, 1.0)
    zero = np.zeros((H, 2), dtype=F)
    got, _ = np_drive(F, taps(), lin, 1.0, 0.0, 1.0, x, zero)
    want, _ = np_drive(np.float64, taps(), lin, 1.0, 0.0, 1.0, x, zero)
    dev = deviation(got, want)
    naive, rule64 = alias_figures(np.float64)
    _, rule32 = alias_figures(F)
    return {"what": "tests/test_drive_host.py.  small_signal: the largest distance of the numpy float32 model of the drive's rule (np_drive) from the "
                    "same rule in binary64, as a fraction of the binary64 output's peak, for noise of magnitude 1e-6 through the linear curve "
                    "(pre 1, dry 0, wet 1); bound = 2 x that; s2r_drive_reference is held to the bound on the same input.  aliasing: a 5 kHz "
                    "sine of amplitude 1 at 48 kHz through the hard clip at pre 8: the energy of a Hann-windowed 4800-frame FFT at the bins "
                    "that are not multiples of 5 kHz, in dB re the whole spectrum (strict: nor beside one: the window's own three bins per "
                    "partial), for clipping at the bus rate in numpy and for the rule in binary64 and in the float32 model; gain = naive - "
                    "rule64; the reference must be lower than the naive figure by the gain less 1 dB",
            "small_signal": dict(SMALL, reference_deviation=dev, bound=2.0 * dev),
            "aliasing": {"naive_db": naive[0], "rule64_db": rule64[0], "model32_db": rule32[0], "gain_db": naive[0] - rule64[0],
                         "strict_naive_db": naive[1], "strict_rule64_db": rule64[1], "strict_model32_db": rule32[1], "strict_gain_db": naive[1] - rule64[1]}}


# ---- the designed curves in numpy float64 ----
def np_curve(kind, a):
    u = np.arange(POINTS, dtype=np.float64) / 512.0 - 1.0
    z = a * u
    if kind == s2.DRIVE_LINEAR:
        y = u
    elif kind == s2.DRIVE_TANH:
        y = np.tanh(z) / np.tanh(a)
    elif kind == s2.DRIVE_HARD:
        y = np.clip(z, -1.0, 1.0)
    elif kind == s2.DRIVE_CUBIC:
        v = np.clip(z, -1.0, 1.0)
        y = 1.5 * v - 0.5 * (v * v * v)
    else:
        r = np.mod(z + 1.0, 4.0)
        y = np.where(r < 2.0, r - 1.0, 3.0 - r)
    return y.astype(F)


CURVE_CASES = [(name, kind, a) for (name, kind, _) in KINDS for a in (1.0 / 64.0, 0.5, 1.0, 2.75, 10.0, 64.0)]
# tanh is the host's libm here and numpy's there: two binary64 values an ulp or so apart round to binary32 values at most one ulp
# apart, 2^-23 of the value; the other kinds are the same binary64 operations in the same order, and fmod is exact
TANH_BOUND_ULP = 1


def measure_curves():
    from helpers import ulp_diff
    rows = []
    for name, kind, a in CURVE_CASES:
        rows.append({"kind": name, "amount": a, "ulps": ulp_diff(s2.drive_curve(kind, a), np_curve(kind, a))})
    return {"what": "tests/test_drive_host.py: the largest distance, in binary32 ulps, of s2r_drive_curve's table from the same formula in numpy "
                    "float64 rounded once.  bound_ulp: what the test allows: 0 for the kinds made of exact or identically ordered binary64 "
                    "operations, 1 for tanh, which is the host's libm on one side and numpy's on the other",
            "bound_ulp": {name: (TANH_BOUND_ULP if kind == s2.DRIVE_TANH else 0) for name, kind, _ in KINDS}, "cases": rows}


# ---- the rule ----
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("which", ["random"] + [k[0] for k in KINDS])
def test_reference_is_the_numpy_model(frames, which):
    """from a history with nothing regular about it, so that all 32 frames are read from the first frame on; pre puts a good part of
    the oversampled samples on either side of the clamp"""
    curve = random_table() if which == "random" else table([k for k in KINDS if k[0] == which][0])
    x = _signal(frames, 100 + frames)
    hist = _signal(H, 7)
    want, wh = np_drive(F, taps(), curve, 2.5, 0.25, 0.75, x, hist)
    got, gh = ref(curve, 2.5, 0.25, 0.75, x, hist)
    assert_bits_equal_finite(got, want, "%s, %d frames" % (which, frames))
    assert_bits_equal_finite(gh, wh, "%s, %d frames: the history" % (which, frames))


@pytest.mark.parametrize("cuts", [(1,), (15, 16, 17), (31, 32, 33, 64), (5, 200, 201, 232, 233, 600)])
def test_calls_of_any_lengths_concatenate(cuts):
    curve = random_table()
    x = _signal(700, 3)
    want, wh = ref(curve, 3.0, 0.5, 0.5, x)
    hist, parts = None, []
    for a, b in zip((0,) + cuts, cuts + (700,)):
        o, hist = ref(curve, 3.0, 0.5, 0.5, x[a:b], hist)
        parts.append(o)
    assert_bits_equal_finite(np.concatenate(parts), want, "cut at %r" % (cuts,))
    assert_bits_equal_finite(hist, wh, "the history")


def test_an_impulse_peaks_at_the_latency_and_is_symmetric_about_it():
    """through the linear curve w is u exactly (every step of the interpolation is exact below 1), so v[n] = sum h[k] g[4 n - k]: the
    two filters in a row, whose delays add up to 64 oversampled samples.  v[16 + d] and v[16 - d] add the same 17 or so products in
    opposite orders: they agree within (17 + 65) * 2^-24 * sum |g h| over those products"""
    h = taps().astype(np.float64)
    g = 4.0 * h
    x = np.zeros((48, 2), dtype=F); x[0] = 1.0
    out, _ = ref(s2.drive_curve(s2.DRIVE_LINEAR), 1.0, 0.0, 1.0, x)
    v = out[:, 0].astype(np.float64)
    assert int(np.argmax(np.abs(v))) == LAT and np.array_equal(out[:, 0], out[:, 1])
    for d in range(1, LAT + 1):
        s = sum(abs(h[k] * g[4 * (LAT + d) - k]) for k in range(TAPS) if 0 <= 4 * (LAT + d) - k <= 64)
        bound = (17 + 65) * 2.0 ** -24 * s
        assert abs(v[LAT + d] - v[LAT - d]) <= bound, (d, v[LAT + d], v[LAT - d], bound)
    assert np.all(out[2 * LAT + 1:] == 0.0)


def test_dry_alone_is_the_input_sixteen_frames_late():
    x = _signal(300, 9)
    hist = _signal(H, 10)
    out, _ = ref(random_table(), 4.0, 1.0, 0.0, x, hist)
    want = np.concatenate([hist, x])[H - LAT:H - LAT + 300]
    assert np.array_equal(out, want)                             # (0 * v is a zero of either sign: -0.0 comes out as +0.0)
    nz = want != 0.0
    assert np.array_equal(out[nz].view(np.uint32), want[nz].view(np.uint32))


@pytest.mark.parametrize("kind", [k[0] for k in KINDS])
def test_past_the_clamp_the_table_s_end_values_come_out(kind):
    """|pre * u| > 1 reads the last interval at fr = 1: c0 + (c1 - c0), which is c1 on bits where the two entries are within a factor
    of two of each other (Sterbenz), as they are at the ends of every designed curve"""
    curve = table([k for k in KINDS if k[0] == kind][0])
    h = taps()
    for sign, end in ((1.0, curve[POINTS - 1]), (-1.0, curve[0])):
        x = np.full((H + 8, 2), sign, dtype=F)
        out, _ = ref(curve, 1024.0, 0.0, 1.0, x, x[:H])
        v = F(0.0)
        for k in range(TAPS):
            v = F(v + F(h[k] * end))
        assert_bits_equal_finite(out, np.full((H + 8, 2), v, dtype=F), "%s, %+g" % (kind, sign))


def test_a_sample_on_a_grid_point_returns_that_entry():
    """an impulse of amplitude A with fl(A * g[32]) = i / 512 on bits, through a table that is 1 at entry 512 + i and 0 elsewhere: only
    the centre tap's sample reaches that interval (the next taps are 9 % lower), and on the grid point fr is 0, so w is 1 there and 0
    elsewhere and the output is h itself, every fourth tap, on bits.  Off the grid by one ulp w would be below 1.  And pre = 0 puts
    every sample on entry 512."""
    h = taps()
    g32 = F(4.0) * h[32]
    found = None
    for i in range(256, 200, -1):
        a0 = F(F(i / 512.0) / g32)
        for step in range(-8, 9):
            a = a0
            for _ in range(abs(step)):
                a = np.nextafter(a, F(INF if step > 0 else -INF))
            if F(a * g32) == F(i / 512.0):
                found = (i, a)
                break
        if found:
            break
    assert found, "no amplitude puts the centre tap on a grid point"
    i, a = found
    assert F(a * F(4.0) * h[31]) < F((i - 1) / 512.0)
    curve = np.zeros(POINTS, dtype=F); curve[512 + i] = 1.0
    x = np.zeros((40, 2), dtype=F); x[0] = a
    out, _ = ref(curve, 1.0, 0.0, 1.0, x)
    want = np.zeros((40, 2), dtype=F)
    for n in range(8, 25):
        want[n] = h[4 * n - 32]
    assert_bits_equal_finite(out, want, "entry %d at amplitude %r" % (512 + i, a))
    curve = random_table()
    out, _ = ref(curve, 0.0, 0.0, 1.0, _signal(20, 4), _signal(H, 5))
    v = F(0.0)
    for k in range(TAPS):
        v = F(v + F(h[k] * curve[512]))
    assert_bits_equal_finite(out, np.full((20, 2), v, dtype=F), "pre 0")


def test_the_history_s_layout():
    """[32][2], oldest first, L then R: a 1.0 at entry k of channel c comes out of the dry path at frame k - 16 of that channel alone,
    and after a call the history is the last 32 frames of history ++ call"""
    lin = s2.drive_curve(s2.DRIVE_LINEAR)
    for k, c in ((16, 0), (31, 1), (20, 1)):
        hist = np.zeros((H, 2), dtype=F); hist[k, c] = 1.0
        out, _ = ref(lin, 1.0, 1.0, 0.0, np.zeros((20, 2), dtype=F), hist)
        want = np.zeros((20, 2), dtype=F); want[k - LAT, c] = 1.0
        assert np.array_equal(out, want), (k, c)
    hist = np.zeros((H, 2), dtype=F); hist[0, 1] = 1.0             # the oldest frame: the wet path alone reaches it, at frame 0, through g[64] and h[64]
    out, _ = ref(lin, 1.0, 0.0, 1.0, np.zeros((3, 2), dtype=F), hist)
    assert out[0, 1] != 0.0 and out[0, 0] == 0.0 and np.all(out[1:] == 0.0)
    x, hist = _signal(5, 1), _signal(H, 2)
    _, new = ref(lin, 1.0, 1.0, 0.0, x, hist)
    assert_bits_equal_finite(new, np.concatenate([hist, x])[5:], "5 frames")
    x = _signal(40, 3)
    _, new = ref(lin, 1.0, 1.0, 0.0, x, hist)
    assert_bits_equal_finite(new, x[8:], "40 frames")
    raw = hist.copy()
    assert s2.load_library().s2r_drive_reference(_p(lin), _f(1.0), _f(1.0), _f(0.0), _p(x), 5, _p(raw), None) == s2s.S2R_OK
    assert_bits_equal_finite(raw, np.concatenate([hist, x[:5]])[5:], "in place")


def test_the_taps():
    h = taps()
    assert h.shape == (TAPS,) and h.dtype == F
    assert np.array_equal(h.view(np.uint32), h[::-1].view(np.uint32))       # symmetric on bits
    assert abs(float(h.astype(np.float64).sum()) - 1.0) <= 65 * 2.0 ** -24
    assert int(np.argmax(h)) == 32 and np.array_equal(taps(), h)
    assert s2.Synth.drive_taps().shape == (TAPS,)
    assert s2.load_library().s2r_drive_taps(None) == s2s.S2R_ERR_INVALID


# ---- the designed curves ----
@pytest.mark.parametrize("case", CURVE_CASES, ids=["%s-%g" % (c[0], c[2]) for c in CURVE_CASES])
def test_designed_curves_are_the_formulas_in_float64(case):
    from helpers import ulp_diff
    name, kind, a = case
    got, want = s2.drive_curve(kind, a), np_curve(kind, a)
    assert got.shape == (POINTS,) and np.isfinite(got).all()
    bound = json.load(open(CURVE_TRUTH))["bound_ulp"][name]
    d = ulp_diff(got, want)
    print("%s at %g: %d ulp, bound %d" % (name, a, d, bound))
    assert d <= bound, (name, a, d)
    if kind == s2.DRIVE_LINEAR:
        assert np.array_equal(got, (np.arange(POINTS) / 512.0 - 1.0).astype(F)) and got[512] == 0.0


def test_the_committed_curve_bounds():
    doc = json.load(open(CURVE_TRUTH))
    assert doc["bound_ulp"] == {name: (TANH_BOUND_ULP if kind == s2.DRIVE_TANH else 0) for name, kind, _ in KINDS}
    assert [(r["kind"], r["amount"]) for r in doc["cases"]] == [(c[0], c[2]) for c in CURVE_CASES]
    for r in doc["cases"]:
        assert r["ulps"] <= doc["bound_ulp"][r["kind"]], r


def test_curve_range_checks():
    L = s2.load_library()
    t = np.full(POINTS, 9.0, dtype=F)
    for kind in (5, 6, M32):
        assert L.s2r_drive_curve(kind, 1.0, _p(t)) == s2s.S2R_ERR_PATCH_RANGE
    for kind in (s2.DRIVE_TANH, s2.DRIVE_HARD, s2.DRIVE_CUBIC, s2.DRIVE_FOLD):
        for a in (NAN, INF, -1.0, 0.0, 0.015, 64.5):
            assert L.s2r_drive_curve(kind, a, _p(t)) == s2s.S2R_ERR_PATCH_RANGE, (kind, a)
        assert L.s2r_drive_curve(kind, 1.0, None) == s2s.S2R_ERR_INVALID
    assert (t == 9.0).all()
    assert L.s2r_drive_curve(s2.DRIVE_LINEAR, NAN, _p(t)) == s2s.S2R_OK and t[0] == -1.0 and t[1024] == 1.0     # the linear kind has no amount
    with pytest.raises(s2.S2rError) as err:
        s2.drive_curve(s2.DRIVE_TANH, 100.0)
    assert err.value.status == s2s.S2R_ERR_PATCH_RANGE


# ---- precision, and what the stage is for ----
def test_the_committed_bounds_are_the_measurement():
    doc = json.load(open(TRUTH))
    r = doc["small_signal"]
    assert {k: r[k] for k in SMALL} == SMALL
    # relative precision kept: indexing the table by t + 1 would quantise this signal to 2^-24 / 1e-6, six per cent of it
    assert r["bound"] == 2.0 * r["reference_deviation"] and 0.0 < r["reference_deviation"] < 1e-5, r
    a = doc["aliasing"]
    assert a["gain_db"] == a["naive_db"] - a["rule64_db"] and a["strict_gain_db"] == a["strict_naive_db"] - a["strict_rule64_db"]
    # The reason for the stage.  The clipped sine is nearly a square wave: odd harmonics k at amplitude 1 / k.  Those from the 7th up
    # (35 kHz and more) lie in the decimator's stop band (past 0.157 cycles per oversampled sample, 30 kHz) and no longer fold; the
    # 5th, at 25 kHz, lies in its transition band and folds to 23 kHz only partly attenuated.  Were it not attenuated at all, the
    # folded energy would still fall from sum over odd k >= 5 of 1 / k^2 = 0.1226 to 1 / 25: 4.9 dB.
    assert a["strict_gain_db"] > 4.9, a


def test_a_small_signal_keeps_its_relative_precision():
    """the library's rule is as close to the rule in binary64 as twice the numpy float32 model's own deviation on the same input
    (measured on the CPU, committed)"""
    row = json.load(open(TRUTH))["small_signal"]
    x = small_signal()
    lin = s2.drive_curve(s2.DRIVE_LINEAR)
    got, _ = ref(lin, 1.0, 0.0, 1.0, x)
    want, _ = np_drive(np.float64, taps(), lin, 1.0, 0.0, 1.0, x, np.zeros((H, 2), dtype=F))
    dev = deviation(got, want)
    print("deviation %.3e, bound %.3e" % (dev, row["bound"]))
    assert dev <= row["bound"], (dev, row["bound"])


def test_oversampling_keeps_the_clipper_s_harmonics_from_folding_back():
    """a 5 kHz sine at 48 kHz through the hard clip at pre 8: the harmonics past 24 kHz of a clip at the bus rate fold back to 23, 13,
    3, 7 kHz and so on.  The reference's energy off the multiples of 5 kHz is below the naive clip's by what the rule in binary64
    shows, less 1 dB for the float32 rounding — counting every bin that is no multiple, and counting only those outside the window's
    three bins per partial.  Figures (profiles/truth/drive_deviation.json): naive -4.2 dB and rule -4.8 dB on every bin off the
    multiples, which the window's own leakage dominates on both sides; strict: naive -11.9 dB, rule -30.6 dB, where what is left is
    the 5th harmonic, 25 kHz, in the decimator's transition band."""
    a = json.load(open(TRUTH))["aliasing"]
    naive, got = alias_figures(None)
    print("naive %.2f dB, reference %.2f dB, binary64 gain %.2f dB; strict: naive %.2f dB, reference %.2f dB, binary64 gain %.2f dB"
          % (naive[0], got[0], a["gain_db"], naive[1], got[1], a["strict_gain_db"]))
    assert naive[0] - got[0] >= a["gain_db"] - 1.0
    assert naive[1] - got[1] >= a["strict_gain_db"] - 1.0


# ---- the range checks ----
GOOD = (1.0, 0.5, 0.5)
# (index into pre, dry, wet; values out of its range)
BAD_LEVELS = [(0, [NAN, INF, -INF, -1e-30, float(np.nextafter(F(1024.0), F(2048.0))), 2048.0]), (1, [NAN, -1e-30, 1.5, INF]), (2, [NAN, -1e-30, 1.5, -INF])]
EDGE_LEVELS = [(0.0, 0.0, 0.0), (1024.0, 1.0, 1.0)]


def bad_tables():
    out = []
    for k in (0, 1, 512, 1023, 1024):
        for v in (NAN, INF, -INF):
            t = s2.drive_curve(s2.DRIVE_LINEAR); t[k] = v
            out.append(t)
    return out


def test_range_errors_without_a_handle():
    """every entry looks at the values before it looks at the handle, so the range checks answer without a device, and a refused
    reference call leaves history and output alone; S2R_ERR_INVALID is what no handle gets for values in range"""
    L = s2.load_library()
    lin = s2.drive_curve(s2.DRIVE_LINEAR)
    big = np.full(POINTS, 3.0e38, dtype=F); big[::2] = -3.0e38    # any finite table is in range
    for t in bad_tables():
        assert L.s2r_set_bus_drive(None, 0, _p(t), *map(_f, GOOD)) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_drive_params(None, 0, _p(t), *map(_f, GOOD)) == s2s.S2R_ERR_PATCH_RANGE
    for k, vals in BAD_LEVELS:
        for v in vals:
            lv = list(GOOD); lv[k] = v
            assert L.s2r_set_bus_drive(None, 0, _p(lin), *map(_f, lv)) == s2s.S2R_ERR_PATCH_RANGE, (k, v)
            assert L.s2r_set_bus_drive_params(None, 0, _p(lin), *map(_f, lv)) == s2s.S2R_ERR_PATCH_RANGE, (k, v)
            assert L.s2r_set_bus_drive_params(None, 0, None, *map(_f, lv)) == s2s.S2R_ERR_PATCH_RANGE, (k, v)
    for bus in (8, 255, M32):
        assert L.s2r_set_bus_drive(None, bus, _p(lin), *map(_f, GOOD)) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_drive_params(None, bus, None, *map(_f, GOOD)) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_clear_bus_drive(None, bus) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_get_bus_drive(None, bus, None, None, 0, None, None, None) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_get_bus_drive_history(None, bus, None, 0) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_drive_history(None, bus, None, 0) == s2s.S2R_ERR_PATCH_RANGE
    for lv in EDGE_LEVELS:
        assert L.s2r_set_bus_drive(None, 7, _p(big), *map(_f, lv)) == s2s.S2R_ERR_INVALID, lv
        assert L.s2r_set_bus_drive_params(None, 7, None, *map(_f, lv)) == s2s.S2R_ERR_INVALID, lv
    assert L.s2r_set_bus_drive(None, 0, None, *map(_f, GOOD)) == s2s.S2R_ERR_INVALID
    assert L.s2r_clear_bus_drive(None, 0) == s2s.S2R_ERR_INVALID
    n = C.c_uint32(5)
    assert L.s2r_get_bus_drive(None, 0, C.byref(n), None, 0, None, None, None) == s2s.S2R_ERR_INVALID and n.value == 5
    buf = np.zeros(2 * H, dtype=F)
    assert L.s2r_get_bus_drive_history(None, 0, _p(buf), buf.size) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_drive_history(None, 0, _p(buf), buf.size) == s2s.S2R_ERR_INVALID
    # the reference: a refusal changes neither the history nor the output
    rf = L.s2r_drive_reference
    x, out = _signal(3, 1), np.full((3, 2), 9.0, dtype=F)
    hist = np.full((H, 2), 0.5, dtype=F)
    for t in bad_tables():
        assert rf(_p(t), *map(_f, GOOD), _p(x), 3, _p(hist), _p(out)) == s2s.S2R_ERR_PATCH_RANGE
    for k, vals in BAD_LEVELS:
        for v in vals:
            lv = list(GOOD); lv[k] = v
            assert rf(_p(lin), *map(_f, lv), _p(x), 3, _p(hist), _p(out)) == s2s.S2R_ERR_PATCH_RANGE, (k, v)
    for v in (NAN, INF, -INF):
        for at in ((0, 0), (H - 1, 1)):
            bad = hist.copy(); bad[at] = v
            assert rf(_p(lin), *map(_f, GOOD), _p(x), 3, _p(bad), _p(out)) == s2s.S2R_ERR_PATCH_RANGE
    assert rf(None, *map(_f, GOOD), _p(x), 3, _p(hist), _p(out)) == s2s.S2R_ERR_INVALID
    assert rf(_p(lin), *map(_f, GOOD), _p(x), 3, None, _p(out)) == s2s.S2R_ERR_INVALID
    assert rf(_p(lin), *map(_f, GOOD), None, 3, _p(hist), _p(out)) == s2s.S2R_ERR_INVALID
    assert (hist == 0.5).all() and (out == 9.0).all()
    assert rf(_p(lin), *map(_f, GOOD), None, 0, _p(hist), None) == s2s.S2R_OK and (hist == 0.5).all()       # no frames: nothing moves
    assert rf(_p(lin), *map(_f, GOOD), _p(x), 3, _p(hist), None) == s2s.S2R_OK and not (hist == 0.5).all()  # no output: the history alone
    for lv in EDGE_LEVELS:
        assert rf(_p(big), *map(_f, lv), _p(x), 3, _p(np.zeros((H, 2), dtype=F)), _p(out)) == s2s.S2R_OK
    with pytest.raises(ValueError):
        s2.drive_reference(lin[:-1], 1.0, 0.0, 1.0, x)
    with pytest.raises(ValueError):
        s2.drive_reference(lin, 1.0, 0.0, 1.0, x, np.zeros((H - 1, 2), dtype=F))
    with pytest.raises(s2.S2rError) as err:
        s2.drive_reference(lin, 1025.0, 0.0, 1.0, x)
    assert err.value.status == s2s.S2R_ERR_PATCH_RANGE
    assert s2.Synth.drive_reference(lin, 1.0, 0.0, 1.0, x)[0].shape == (3, 2)
    syn = _new_or_skip(num_voices=8, max_frames=64)              # with a device the rest runs on a real handle
    if syn is not None:
        check_ranges(syn)


def test_abi_version_stays():
    assert s2.load_library().s2r_abi_version() == 4


def check_ranges(syn):
    """the setters' range checks on a live handle, and the parameter and history entries on a bus without a drive (also called by
    tests/test_gpu_drive.py)"""
    L, h = syn.L, syn.h
    lin = s2.drive_curve(s2.DRIVE_LINEAR)
    for t in bad_tables()[::4]:
        assert L.s2r_set_bus_drive(h, 0, _p(t), *map(_f, GOOD)) == s2s.S2R_ERR_PATCH_RANGE
    for k, vals in BAD_LEVELS:
        lv = list(GOOD); lv[k] = vals[0]
        assert L.s2r_set_bus_drive(h, 0, _p(lin), *map(_f, lv)) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_drive(h, 8, _p(lin), *map(_f, GOOD)) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_drive(h, 0, None, *map(_f, GOOD)) == s2s.S2R_ERR_INVALID
    assert syn.get_bus_drive(0) is None
    assert L.s2r_set_bus_drive_params(h, 0, None, *map(_f, GOOD)) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_drive_params(h, 0, _p(lin), *map(_f, GOOD)) == s2s.S2R_ERR_INVALID
    buf = np.zeros(2 * H, dtype=F)
    assert L.s2r_get_bus_drive_history(h, 0, _p(buf), buf.size) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_drive_history(h, 0, _p(buf), buf.size) == s2s.S2R_ERR_INVALID
    assert L.s2r_clear_bus_drive(h, 0) == s2s.S2R_OK


if __name__ == "__main__":
    os.makedirs(os.path.dirname(TRUTH), exist_ok=True)
    for path, doc in ((TRUTH, measure()), (CURVE_TRUTH, measure_curves())):
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(json.dumps(doc, indent=1))
