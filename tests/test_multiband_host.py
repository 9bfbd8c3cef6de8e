"""The master multiband compressor's host rule (s2r_multiband_reference, s2r_multiband_design) against the independent
restatement of tests/multiband_model.py: a binary32 frame loop in numpy for the bits, binary64 for what the crossover adds up to.  No
device."""
import json
import os

import numpy as np
import pytest
from scipy.signal import butter

import multiband_model as mm
import synth2_amd as s2
from synth2_amd import synth as s2s

F = np.float32
SR = 48000.0
SPLITS = [200.0, 1500.0, 6000.0]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUTH = json.load(open(os.path.join(ROOT, "profiles", "truth", "multiband_deviation.json")))


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _coeffs(B, splits=SPLITS):
    return s2.multiband_design(SR, splits[:B - 1]) if B > 1 else None


def _rows(coeffs):
    return coeffs if coeffs is not None else (np.zeros((0, 5), F), np.zeros((0, 5), F), np.zeros((0, 5), F))


def _signal(n, seed):
    """a chord over three octaves with noise under it, so that every band of splits at 200 / 1500 / 6000 Hz carries signal that
    rises and falls: stereo, the right channel another mixture"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    env = 0.5 + 0.5 * np.sin(2.0 * np.pi * 37.0 * t)
    tones = sum(np.sin(2.0 * np.pi * f * t + k) for k, f in enumerate((82.4, 164.8, 329.6, 659.3, 2637.0, 7040.0, 9000.0)))
    l = 0.2 * env * tones + 0.05 * rng.standard_normal(n)
    r = 0.15 * (1.0 - env) * tones + 0.05 * rng.standard_normal(n)
    return np.stack([l, r], axis=1).astype(F)


def _curves(B, x):
    bands = s2.multiband_reference(_coeffs(B), np.ones((B, mm.POINTS), F), [0.0] * B, [0.0] * B, x, want_bands=True)[3]
    return np.stack([s2.dynamics_curve(20.0 * np.log10(float(np.abs(bands[j]).max()) / 2.0), (4.0, 2.0, 8.0, float("inf"))[j], (6.0, 0.0, 12.0, 3.0)[j], 1.5 * j)
                     for j in range(B)])


def _coef(ms):
    """s2r_dynamics_coef's value (computed here: nothing loads the library while the suite is collected)"""
    return float(F(np.exp(-1.0 / (ms * 0.001 * SR)))) if ms else 0.0


ATT = [_coef(ms) for ms in (1.0, 0.0, 5.0, 0.3)]
REL = [_coef(ms) for ms in (50.0, 20.0, 0.0, 100.0)]


def _initial(B, curves):
    st = np.zeros(s2.multiband_state_floats(B), dtype=F)
    st[-B:] = curves[:, 0]
    return st


@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_the_reference_is_the_numpy_frame_loop(B):
    """output, state, minima and band signals, bit for bit, from the initial state and from a carried one; every band works: its gain
    falls below its start and moves both ways"""
    x = _signal(700, 3)
    coeffs, curves = _coeffs(B), _curves(B, _signal(700, 3))
    lp, hp, ap = _rows(coeffs)
    st = _initial(B, curves)
    for part in (x[:450], x[450:]):
        got = s2.multiband_reference(coeffs, curves, ATT[:B], REL[:B], part, st, want_bands=True)
        want = mm.np32(B, lp, hp, ap, curves, ATT[:B], REL[:B], part, st)
        for g, w, name in zip(got, want, ("output", "state", "minima", "bands")):
            assert np.isfinite(g).all() and np.array_equal(bits(g), bits(w)), "%d bands: %s" % (B, name)
        assert not np.array_equal(bits(st), bits(got[1]))
        st = got[1]
        assert (got[2] < curves[:, 0]).all(), got[2]
    assert s2.multiband_sections(B) == (0, 4, 9, 15)[B - 1] and st.size == 4 * s2.multiband_sections(B) + B


def test_one_band_is_the_dynamics_reference():
    x = _signal(900, 5)
    curve = _curves(1, x)[0]
    out, st, mn = s2.multiband_reference(None, curve[None], ATT[:1], REL[:1], x)
    want, y, wmn = s2.dynamics_reference(curve, ATT[0], REL[0], None, x, curve[0])
    assert np.array_equal(bits(out), bits(want)) and bits(st)[0] == bits(y) and bits(mn)[0] == bits(wmn)
    assert wmn < curve[0]


@pytest.mark.parametrize("B", [2, 4])
def test_a_stream_cut_into_calls_is_one_call(B):
    x = _signal(1300, 7)
    coeffs, curves = _coeffs(B), _curves(B, x)
    whole = s2.multiband_reference(coeffs, curves, ATT[:B], REL[:B], x)
    for step in (1, 7, 300):
        st, outs, mn = _initial(B, curves), [], np.full(B, np.inf, dtype=F)
        for at in range(0, x.shape[0], step):
            o, st, m = s2.multiband_reference(coeffs, curves, ATT[:B], REL[:B], x[at:at + step], st)
            outs.append(o)
            mn = np.minimum(mn, m)
        assert np.array_equal(bits(np.concatenate(outs)), bits(whole[0])), "calls of %d: output" % step
        assert np.array_equal(bits(st), bits(whole[1])), "calls of %d: state" % step
        assert np.array_equal(bits(mn), bits(whole[2])), "calls of %d: minima" % step
    o, st, m = s2.multiband_reference(coeffs, curves, ATT[:B], REL[:B], x[:0], whole[1])
    assert o.shape == (0, 2) and np.array_equal(bits(st), bits(whole[1])) and np.isinf(m).all()


@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_unit_curves_leave_the_ordered_band_sum(B):
    x = _signal(600, 9)
    out, st, mn, bands = s2.multiband_reference(_coeffs(B), np.ones((B, mm.POINTS), F), [0.0] * B, [0.0] * B, x, want_bands=True)
    assert np.array_equal(bits(mn), bits(np.ones(B, F))) and np.array_equal(bits(st[-B:]), bits(np.ones(B, F)))
    acc = bands[0].copy()
    for j in range(1, B):
        acc = acc + bands[j]
    assert np.array_equal(bits(out), bits(acc))
    if B == 1:
        assert np.array_equal(bits(out), bits(x))


@pytest.mark.parametrize("B", [2, 3, 4])
@pytest.mark.parametrize("splits", ["200/1500/6000", "120/1000/6000"])
def test_the_unit_gain_sum_is_the_allpass_cascade(B, splits):
    """the library's band sum with unit curves against the binary64 allpass cascade AP_{B-2}( ... AP_0(x)) with binary64 coefficients,
    within the bound tools/multiband_truth.py measured on the restatement and doubled (profiles/truth/multiband_deviation.json), on
    noise of another seed than the tool's and on the tool's sweep"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("multiband_truth", os.path.join(ROOT, "tools", "multiband_truth.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    f = tool.SPLIT_SETS[splits][:B - 1]
    bound = float(TRUTH["bound"][str(B)])
    assert 0.0 < bound < 2e-3
    ap_all = mm.design64(SR, f)[2]
    x_noise, x_sweep = tool.signals(seed=77)["noise"], tool.signals()["sweep"]
    for name, x in (("noise", x_noise), ("sweep", x_sweep)):
        out = s2.multiband_reference(_coeffs(B, f), np.ones((B, mm.POINTS), F), [0.0] * B, [0.0] * B, x)[0]
        dev = float(np.abs(out.astype(np.float64) - mm.allpass64(ap_all, x)).max()) / float(np.abs(x).max())
        print("%d bands at %s Hz, %s: %.3e of the peak, bound %.3e" % (B, splits, name, dev, bound))
        assert dev <= bound, (name, dev, bound)


def test_the_truth_file_is_what_the_tool_writes(tmp_path, monkeypatch):
    """profiles/truth/multiband_deviation.json is the tool's output, not a hand-written number"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("multiband_truth", os.path.join(ROOT, "tools", "multiband_truth.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    r = tool.measure(3, tool.SPLIT_SETS["200/1500/6000"], tool.signals()["noise"])
    rec = TRUTH["cases"]["3 bands, 200/1500 Hz, noise"]
    for k in ("rounded64", "rule32", "sum32"):
        assert abs(r[k] - rec[k]) <= 2e-3 * rec[k], (k, r[k], rec[k])
    assert r["identity64"] < 1e-12


def test_the_design_is_scipys_butterworth():
    """every row within 1 ulp of float32 of butter(2, f, fs=sr); the allpass row is the denominator reversed over itself"""
    for sr, splits in ((48000.0, SPLITS), (44100.0, [120.0, 1000.0, 6000.0]), (96000.0, [50.0, 20000.0])):
        lp, hp, ap = s2.multiband_design(sr, splits)
        assert lp.shape == hp.shape == (len(splits), 5) and ap.shape == (len(splits) - 1, 5)
        for k, f in enumerate(splits):
            for got, kind in ((lp[k], "low"), (hp[k], "high")):
                b, a = butter(2, f, btype=kind, fs=sr)
                want = np.array([b[0], b[1], b[2], a[1], a[2]]).astype(F)
                assert (np.abs(bits(got).astype(np.int64) - bits(want).astype(np.int64)) <= 1).all(), (sr, f, kind, got, want)
            if k:
                _, a = butter(2, f, fs=sr)
                want = np.array([a[2], a[1], 1.0, a[1], a[2]]).astype(F)
                assert (np.abs(bits(ap[k - 1]).astype(np.int64) - bits(want).astype(np.int64)) <= 1).all(), (sr, f, ap[k - 1], want)
    assert all(c.shape[0] == 0 for c in s2.multiband_design(SR, []))
    for bad in ([0.0], [24000.0], [500.0, 500.0], [900.0, 300.0], [float("nan")], [100.0, 200.0, 300.0, 400.0]):
        with pytest.raises(s2.S2rError):
            s2.multiband_design(SR, bad)


def test_every_refusal_changes_nothing():
    """ranges first (S2R_ERR_PATCH_RANGE), then null arrays (S2R_ERR_INVALID); state, output and minima keep what they held"""
    L = s2.load_library()
    B = 3
    x = _signal(64, 11)
    lp, hp, ap = _coeffs(B)
    curves = _curves(B, _signal(700, 3))
    att, rel = np.array(ATT[:B], dtype=F), np.array(REL[:B], dtype=F)
    st0 = _initial(B, curves)
    st0[:4] = (0.25, -0.5, 0.125, 1.0)
    p = lambda v: v.ctypes.data_as(s2s._f32p) if v is not None else None

    def call(n_bands=B, lp_=lp, hp_=hp, ap_=ap, cv=curves, at=att, rl=rel, state=st0, xs=x):
        st, out, mn = (None if state is None else state.copy()), np.full((64, 2), 7.0, dtype=F), np.full(4, 9.0, dtype=F)
        rc = L.s2r_multiband_reference(n_bands, p(lp_), p(hp_), p(ap_), p(cv), p(at), p(rl), p(xs), 64, p(st), p(out), None, p(mn))
        if rc != s2s.S2R_OK:
            assert state is None or np.array_equal(bits(st), bits(state)), "a refusal moved the state"
            assert (out == 7.0).all() and (mn == 9.0).all(), "a refusal wrote an output"
        return rc

    assert call() == s2s.S2R_OK
    edit = lambda v, idx, val: (lambda c: (c.__setitem__(idx, val), c)[1])(v.copy())
    for name, rc, want in (
            ("no band", call(n_bands=0), s2s.S2R_ERR_PATCH_RANGE), ("five bands", call(n_bands=5), s2s.S2R_ERR_PATCH_RANGE),
            ("a NaN in lp", call(lp_=edit(lp, (1, 0), np.nan)), s2s.S2R_ERR_PATCH_RANGE), ("an infinity in hp", call(hp_=edit(hp, (0, 1), np.inf)), s2s.S2R_ERR_PATCH_RANGE),
            ("a2 = 1 in ap", call(ap_=edit(ap, (0, 4), 1.0)), s2s.S2R_ERR_PATCH_RANGE), ("|a1| = 1 + a2 in lp", call(lp_=edit(edit(lp, (0, 4), 0.5), (0, 3), 1.5)), s2s.S2R_ERR_PATCH_RANGE),
            ("a curve entry below 0", call(cv=edit(curves, (2, 7), -0.5)), s2s.S2R_ERR_PATCH_RANGE), ("a curve entry of 257", call(cv=edit(curves, (0, 512), 257.0)), s2s.S2R_ERR_PATCH_RANGE),
            ("an attack of 1", call(at=edit(att, 1, 1.0)), s2s.S2R_ERR_PATCH_RANGE), ("a release below 0", call(rl=edit(rel, 2, -0.1)), s2s.S2R_ERR_PATCH_RANGE),
            ("a NaN filter state", call(state=edit(st0, 5, np.nan)), s2s.S2R_ERR_PATCH_RANGE), ("a gain below 0", call(state=edit(st0, st0.size - 1, -1.0)), s2s.S2R_ERR_PATCH_RANGE),
            ("null lp", call(lp_=None), s2s.S2R_ERR_INVALID), ("null ap at three bands", call(ap_=None), s2s.S2R_ERR_INVALID), ("null curves", call(cv=None), s2s.S2R_ERR_INVALID),
            ("null coefficients of retention", call(at=None), s2s.S2R_ERR_INVALID), ("a null state", call(state=None), s2s.S2R_ERR_INVALID),
            ("a null input", call(xs=None), s2s.S2R_ERR_INVALID)):
        assert rc == want, "%s: %d, not %d" % (name, rc, want)
    # null arrays of no rows are accepted: ap at two bands, all three at one
    two = L.s2r_multiband_reference(2, p(lp), p(hp), None, p(curves), p(att), p(rel), p(x), 64, p(_initial(2, curves[:2])), None, None, None)
    one = L.s2r_multiband_reference(1, None, None, None, p(curves), p(att), p(rel), p(x), 64, p(_initial(1, curves[:1])), None, None, None)
    assert two == s2s.S2R_OK and one == s2s.S2R_OK
    # the design leaves its outputs alone when it refuses
    f = np.array([500.0, 400.0])
    keep = np.full((2, 5), 3.0, dtype=F)
    rc = L.s2r_multiband_design(SR, f.ctypes.data_as(s2s.C.POINTER(s2s.C.c_double)), 2, p(keep), p(keep), p(keep))
    assert rc == s2s.S2R_ERR_PATCH_RANGE and (keep == 3.0).all()
