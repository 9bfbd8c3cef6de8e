"""The master limiter's true-peak detector, the host side: s2r_limiter_tp_reference — the rule restated in plain C++
loops — held on bits against a numpy float32 model of the rule written here (np_limiter_tp, which tests/test_gpu_limiter_tp.py holds
the device against too), the properties the rule promises with no model in the loop, what the detector is for — the project's own
true-peak meter reads the output near the ceiling, where the sample-peak rule leaves it decibels above —, and the range checks of the
entry points, which answer without a device."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view
import pytest

import synth2_amd as s2
from synth2_amd import synth as s2s
from test_limiter_host import BAD, CUTS, GOOD, PAIRS, bits, noise, _new_or_skip, _p
from test_loudness_host import np_taps

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAT, HIST = 8, 16
SHORT_CALLS = [1, 2, 7, 8, 9, 15, 16, 17]
TRUTH = os.path.join(ROOT, "profiles", "truth", "limiter_tp_deviation.json")


def truth_tool():
    spec = importlib.util.spec_from_file_location("limiter_tp_truth", os.path.join(ROOT, "tools", "limiter_tp_truth.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def np_detector(xe, N, g):
    """step 1' in numpy float32: xe [16 + N, 2] — the 16 frames in front, then the call's —, g the 65 taps; d [N].  One array
    operation is one rounded operation per frame; the sums run from +0.0 in ascending j."""
    d = np.abs(xe[HIST - LAT:HIST - LAT + N]).max(axis=1)
    with np.errstate(under="ignore"):
        for c in range(2):
            for p in range(4):
                u = np.zeros(N, F)
                for j in range(HIST + 1):
                    if p + 4 * j < len(g):
                        t = (g[p + 4 * j] * xe[HIST - j:HIST - j + N, c]).astype(F)
                        u = (u + t).astype(F)
                d = np.maximum(d, np.abs(u))
    assert d.dtype == F
    return d


def np_limiter_tp(x, C, L, H, xh=None, gh=None, detail=False):
    """The rule in numpy float32: x [N, 2]; returns (y, s', xh, gh) with the state the call leaves — xh [L + 16, 2] —, and with
    detail also d [N] and the sample magnitude max |x_c[n - 8]| it replaces."""
    N = len(x); C = F(C); W = L + 1; G = 2 * L + H; X = L + HIST
    xh = np.zeros((X, 2), F) if xh is None else xh
    gh = np.ones(G, F) if gh is None else gh
    assert xh.shape == (X, 2) and gh.shape == (G,) and x.dtype == F
    xe = np.concatenate([xh, x])                                 # frame n of the call at X + n
    d = np_detector(xe[L:], N, np_taps())
    with np.errstate(divide="ignore", invalid="ignore", under="ignore", over="ignore"):
        g = np.where(d > C, C / d, F(1)).astype(F)
    ge = np.concatenate([gh, g])
    m = sliding_window_view(ge, L + H + 1).min(axis=1)           # m[j] is m[n = j - L]
    acc = np.zeros(N, F)
    with np.errstate(under="ignore"):
        for k in range(W):
            acc = (acc + m[L - k:L - k + N]).astype(F)
        s = (acc / F(W)).astype(F)
        sp = np.minimum(s, ge[G - L:G - L + N])
        y = np.minimum(np.maximum((xe[LAT:LAT + N] * sp[:, None]).astype(F), -C), C)       # x[n - L - 8] at X + n - L - 8
    assert y.dtype == F and sp.dtype == F
    out = (y, sp, xe[N:], ge[N:])
    return out + (d, np.abs(xe[X - LAT:X - LAT + N]).max(axis=1)) if detail else out


def half_peak(x):
    return F(0.5) * np.abs(x).max()


def _both(x, c, L, H, xh, gh, what):
    """one call through the model and the reference from the same state; everything on bits; returns the model's"""
    want = np_limiter_tp(x, c, L, H, xh, gh)
    got = s2.limiter_tp_reference(x, c, L, H, xh, gh)
    for g, w, name in zip(got, want, ("y", "gain", "xh", "gh")):
        assert g.shape == w.shape, (what, name)
        assert np.isfinite(g).all() and np.array_equal(bits(g), bits(w)), (what, name)
    return want


def check_model_bites(sp, d, mag):
    """at least a quarter of the frames limited, and in at least a quarter the detector's magnitude is not the sample's"""
    assert (sp < 1.0).mean() >= 0.25, (sp < 1.0).mean()
    assert (bits(d) != bits(mag)).mean() >= 0.25, (bits(d) != bits(mag)).mean()


@pytest.mark.parametrize("L,H", PAIRS)
def test_reference_is_the_rule(L, H):
    """noise of 3000 frames under a ceiling of half its peak: one call, the same stream cut into calls of 7, 293, 1, 1699 and 1000
    frames, and again into runs of 1, 2, 7, 8, 9, 15, 16 and 17 frames — around the latency of 8 and the history of 16 — with the
    state carried: every call equal to the model on bits, and the pieces equal to the one call"""
    x = noise(scale=0.5)
    c = half_peak(x)
    y, sp, xh, gh, d, mag = np_limiter_tp(x, c, L, H, detail=True)
    check_model_bites(sp, d, mag)
    _both(x, c, L, H, None, None, "one call")
    for cuts, whole in ((CUTS, True), (SHORT_CALLS * 8, False)):      # (the short calls: the stream's first 600 frames)
        at, ys, sps, xh2, gh2 = 0, [], [], None, None
        for n in cuts:
            yy, ss, xh2, gh2 = _both(x[at:at + n], c, L, H, xh2, gh2, "cut at %d" % at)
            ys.append(yy), sps.append(ss)
            at += n
        assert at == (len(x) if whole else 600)
        assert np.array_equal(bits(np.concatenate(ys)), bits(y[:at])) and np.array_equal(bits(np.concatenate(sps)), bits(sp[:at]))
        if whole:
            assert np.array_equal(bits(xh2), bits(xh)) and np.array_equal(bits(gh2), bits(gh))
    assert np.array_equal(bits(xh), bits(np.concatenate([np.zeros((L + HIST, 2), F), x])[-(L + HIST):]))


@pytest.mark.parametrize("L,H", PAIRS)
def test_delay_and_ceiling_without_a_model(L, H):
    """the reference alone: no output sample exceeds the ceiling; under a ceiling above the largest interpolated magnitude the
    output is the input delayed by L + 8 frames in every bit, behind L + 8 frames of +0.0, with a gain of exactly 1"""
    x = noise(scale=0.5)
    c = half_peak(x)
    y, gain, _, _ = s2.limiter_tp_reference(x, c, L, H)
    assert np.abs(y).max() <= c and (gain > 0.0).all() and (gain <= 1.0).all() and gain.min() < 1.0
    D = L + LAT
    for ceiling in (4.0 * float(np.abs(x).max()), 1000.0):     # (the interpolator's gain is below 2: the sum of a phase's |taps|)
        y, gain, xh, gh = s2.limiter_tp_reference(x, ceiling, L, H)
        assert np.array_equal(bits(y[D:]), bits(x[:len(x) - D])) and not bits(y[:D]).any()
        assert np.array_equal(bits(gain), bits(np.ones(len(x), F))) and np.array_equal(bits(gh), bits(np.ones(2 * L + H, F)))
        assert np.array_equal(bits(xh), bits(x[len(x) - (L + HIST):]))
    assert max(float(np.abs(np_taps()[p::4]).sum()) for p in range(4)) < 2.0


def meter_true_peak(y):
    """the project's meter over y [N, 2] from its initial state: the larger channel's true peak"""
    return float(s2.loudness_reference(s2.loudness_design(48000.0), 4800, None, y)[3].max())


@pytest.mark.parametrize("L,H", [(48, 0), (16, 8)])
def test_the_true_peak_of_the_output_is_held(L, H):
    """what the detector is for.  An fs/4 sine at 45 degrees, seeded noise and a naive square at 1661.2 Hz, 6000 frames each, the
    ceiling half the sample peak: behind the sample-peak rule the project's meter reads at least 1.1 ceilings (the float64 model:
    1.24 to 1.43); behind the true-peak detector at most 1 + 2 e, e the largest excess of the float64 evaluation of
    tools/limiter_tp_truth.py over these signals and pairs (committed: profiles/truth/limiter_tp_deviation.json), 2 the project's
    margin for binary32 against binary64."""
    e = json.load(open(TRUTH))["e"]
    assert 0.0 < e < 0.05
    for name, x in truth_tool().signals().items():
        assert x.shape == (6000, 2) and x.dtype == F
        c = half_peak(x)
        sample = meter_true_peak(s2.limiter_reference(x, c, L, H)[0]) / float(c)
        held = meter_true_peak(s2.limiter_tp_reference(x, c, L, H)[0]) / float(c)
        print("%s (%d, %d): sample-peak rule %.6f C, true-peak detector %.6f C, bound %.6f C" % (name, L, H, sample, held, 1.0 + 2.0 * e))
        assert sample >= 1.1, (name, sample)
        assert held <= 1.0 + 2.0 * e, (name, held)


def test_the_committed_e_is_the_tools():
    """the committed figure is what tools/limiter_tp_truth.py computes now (float64 numpy alone, never the library)"""
    t = truth_tool()
    g, e = t.taps64(), 0.0
    assert np.array_equal(bits(g.astype(F)), bits(np_taps()))    # the tool's own design of the taps is the library's, on bits
    for x in t.signals().values():
        c = 0.5 * float(np.abs(x).max())
        for L, H in t.PAIRS:
            e = max(e, t.true_peak64(t.limiter64(x, c, L, H, True, g), g) / c - 1.0)
    assert t.PAIRS == [(48, 0), (16, 8)] and abs(e - json.load(open(TRUTH))["e"]) < 2e-6


def test_range_errors_without_a_handle():
    """the setter looks at the detector with the other values, before the handle: S2R_ERR_PATCH_RANGE for a detector above 1 and for
    every bad triple beside detector 1, S2R_ERR_INVALID is what no handle gets for values in range; the reference's refusals.  With
    a device the rest runs on a real handle (check_ranges_tp, also called by tests/test_gpu_limiter_tp.py)."""
    L = s2.load_library()
    assert (s2.LIMITER_SAMPLE_PEAK, s2.LIMITER_TRUE_PEAK, s2.LIMITER_TP_LATENCY, s2.LIMITER_TP_HISTORY) == (0, 1, LAT, HIST)
    x, y, gain = np.zeros((4, 2), dtype=F), np.zeros((4, 2), dtype=F), np.zeros(4, dtype=F)
    for det in (2, 0xffffffff):
        assert L.s2r_set_master_limiter_ex(None, 0.25, 48, 0, det) == s2s.S2R_ERR_PATCH_RANGE, det
    for c, la, hold in BAD:
        assert L.s2r_set_master_limiter_ex(None, c, la, hold, 1) == s2s.S2R_ERR_PATCH_RANGE, (c, la, hold)
        assert L.s2r_limiter_tp_reference(_p(x), 4, c, la, hold, None, None, _p(y), _p(gain)) == s2s.S2R_ERR_PATCH_RANGE, (c, la, hold)
    for c, la, hold in GOOD:
        for det in (0, 1):
            assert L.s2r_set_master_limiter_ex(None, c, la, hold, det) == s2s.S2R_ERR_INVALID, (c, la, hold)
        xh, gh = np.zeros((la + HIST, 2), dtype=F), np.ones(2 * la + hold, dtype=F)
        assert L.s2r_limiter_tp_reference(_p(x), 4, c, la, hold, None, _p(gh), _p(y), _p(gain)) == s2s.S2R_ERR_INVALID
        assert L.s2r_limiter_tp_reference(_p(x), 4, c, la, hold, _p(xh), None, _p(y), _p(gain)) == s2s.S2R_ERR_INVALID
        assert L.s2r_limiter_tp_reference(None, 4, c, la, hold, _p(xh), _p(gh), _p(y), _p(gain)) == s2s.S2R_ERR_INVALID
        assert L.s2r_limiter_tp_reference(None, 0, c, la, hold, _p(xh), _p(gh), None, None) == s2s.S2R_OK     # no frames: nothing moves
        assert not bits(xh).any() and (gh == 1.0).all()
        assert L.s2r_limiter_tp_reference(_p(x), 4, c, la, hold, _p(xh), _p(gh), None, None) == s2s.S2R_OK    # the outputs may be null
    n = C.c_uint32()
    assert L.s2r_get_master_limiter_detector(None, C.byref(n)) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        s2.limiter_tp_reference(x, 0.25, 0, 0)
    assert err.value.status == s2s.S2R_ERR_PATCH_RANGE
    with pytest.raises(ValueError):
        s2.limiter_tp_reference(np.zeros((4, 3), dtype=F), 0.25, 4, 0)
    with pytest.raises(ValueError):
        s2.limiter_tp_reference(x, 0.25, 4, 0, xh=np.zeros((4, 2), dtype=F))     # the sample-peak rule's shape
    xh, gh = np.zeros((4 + HIST, 2), dtype=F), np.ones(9, dtype=F)
    s2.Synth.limiter_tp_reference(np.ones((6, 2), dtype=F), 0.25, 4, 1, xh, gh)   # the arguments are not modified
    assert not bits(xh).any() and (gh == 1.0).all()
    assert L.s2r_abi_version() == 4
    syn = _new_or_skip(num_voices=8, max_frames=64)
    if syn is not None:
        check_ranges_tp(syn)


def check_ranges_tp(syn):
    """the entries on a real handle that makes no fill: the sizes of the state pair follow the detector, a mismatch is refused in
    either mode, another detector resets the state, another ceiling keeps it"""
    L, h = syn.L, syn.h
    buf, gbuf = np.zeros(64, dtype=F), np.zeros(64, dtype=F)
    assert syn.get_master_limiter() == (0.0, 0, 0) and syn.get_master_limiter_detector() == 0
    for det in (2, 0xffffffff):
        assert L.s2r_set_master_limiter_ex(h, 0.5, 4, 3, det) == s2s.S2R_ERR_PATCH_RANGE
    for c, la, hold in BAD:
        assert L.s2r_set_master_limiter_ex(h, c, la, hold, 1) == s2s.S2R_ERR_PATCH_RANGE, (c, la, hold)
    assert syn.get_master_limiter() == (0.0, 0, 0) and syn.get_master_limiter_detector() == 0       # a refused call changes nothing
    assert L.s2r_get_master_limiter_detector(h, None) == s2s.S2R_ERR_INVALID
    syn.set_master_limiter(0.5, 4, 3, true_peak=True)
    assert syn.get_master_limiter() == (0.5, 4, 3) and syn.get_master_limiter_detector() == s2.LIMITER_TRUE_PEAK
    xh, gh = syn.limiter_state()
    assert xh.shape == (20, 2) and gh.shape == (11,) and not bits(xh).any() and (gh == 1.0).all()
    for n_x, n_g in ((8, 11), (39, 11), (41, 11), (40, 10), (40, 12), (0, 0)):       # (8, 11) is the sample-peak rule's pair
        assert L.s2r_set_limiter_state(h, _p(buf), n_x, _p(gbuf), n_g) == s2s.S2R_ERR_INVALID, (n_x, n_g)
    for n_x, n_g in ((8, 11), (39, 11), (40, 10), (0, 0)):
        assert L.s2r_get_limiter_state(h, _p(buf), n_x, _p(gbuf), n_g) == s2s.S2R_ERR_INVALID, (n_x, n_g)
    assert L.s2r_get_limiter_state(h, _p(buf), 64, _p(gbuf), 64) == s2s.S2R_OK            # larger buffers will do
    new_x, new_g = np.arange(40, dtype=F).reshape(20, 2) - F(19.5), np.linspace(0.25, 1.0, 11, dtype=F)
    syn.set_limiter_state(new_x, new_g)
    xh, gh = syn.limiter_state()
    assert np.array_equal(bits(xh), bits(new_x)) and np.array_equal(bits(gh), bits(new_g))
    syn.set_master_limiter(0.25, 4, 3, true_peak=True)           # the ceiling alone: the state stays
    xh, gh = syn.limiter_state()
    assert np.array_equal(bits(xh), bits(new_x)) and np.array_equal(bits(gh), bits(new_g))
    syn.set_master_limiter(0.25, 4, 3)                           # the other detector: the initial state, the sample-peak rule's shapes
    assert syn.get_master_limiter() == (0.25, 4, 3) and syn.get_master_limiter_detector() == s2.LIMITER_SAMPLE_PEAK
    xh, gh = syn.limiter_state()
    assert xh.shape == (4, 2) and gh.shape == (11,) and not bits(xh).any() and (gh == 1.0).all()
    for n_x, n_g in ((40, 11), (7, 11), (8, 10)):                # (40, 11) is the true-peak detector's pair
        assert L.s2r_set_limiter_state(h, _p(buf), n_x, _p(gbuf), n_g) == s2s.S2R_ERR_INVALID, (n_x, n_g)
    syn.set_limiter_state(new_x[:4], new_g)
    assert L.s2r_set_master_limiter_ex(h, 0.25, 4, 3, 1) == s2s.S2R_OK      # and back: the initial state again
    xh, gh = syn.limiter_state()
    assert xh.shape == (20, 2) and not bits(xh).any() and (gh == 1.0).all()
    syn.set_limiter_state(new_x, new_g)
    syn.set_master_limiter(0.25, 5, 3, true_peak=True)           # another lookahead resets as before
    xh, gh = syn.limiter_state()
    assert xh.shape == (21, 2) and gh.shape == (13,) and not bits(xh).any() and (gh == 1.0).all()
    syn.clear_master_limiter()
    assert syn.get_master_limiter() == (0.0, 0, 0) and syn.get_master_limiter_detector() == 0
    assert L.s2r_get_limiter_state(h, _p(buf), 64, _p(gbuf), 64) == s2s.S2R_ERR_INVALID
