"""The blocks whose only definition is the oracle — the dsp_filters.rs filters, the SVF outputs, the DPW shapes, the 4x
decimator — held to the independent binary64 models of tests/truth_model.py, on the CPU: (a) the models themselves against the
textbook (scipy's bilinear transform of the prewarped analog prototypes, and the headline gains), (b) the oracle against the
models on the same case table tests/test_gpu_truth_blocks.py runs on the GPU's own rows, within the bounds committed in
profiles/truth/blocks_deviation.json (tools/truth_blocks.py writes it; twice the oracle's own deviation per case)."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

import truth_model as tm
from oracle import s2o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "profiles", "truth", "blocks_deviation.json")


def _tool():
    spec = importlib.util.spec_from_file_location("truth_blocks", os.path.join(ROOT, "tools", "truth_blocks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool():
    return _tool()


@pytest.fixture(scope="module")
def measured(tool):
    return tool.measure()


@pytest.fixture(scope="module")
def committed():
    return json.load(open(TABLE))


# ------------------------------------------------------------------------------------------ (a) the truth and the textbook

GRID = [(sr, fc, p) for sr in tm.RATES for fc in tm.CUTOFFS[sr] for p in tm.PARAMS]


def _gain(b, a, theta):
    z = np.exp(-1j * theta * np.arange(3))
    return abs(np.dot(b, z) / np.dot(a, z))


def test_coefficients_are_the_bilinear_transform_of_the_analog_prototypes():
    signal = pytest.importorskip("scipy.signal")
    for sr, fc, p in GRID:
        w = 2.0 * sr * np.tan(np.pi * fc / sr)                 # prewarped: the digital filter meets the prototype at fc
        for Q, kinds in ((1.0 / p, (tm.LP2, tm.HP2, None)), (p, (tm.SVF_LP, tm.SVF_HP, tm.SVF_BP))):
            den = [1.0 / w ** 2, 1.0 / (Q * w), 1.0]
            for kind, num in zip(kinds, ([1.0], [1.0 / w ** 2, 0.0, 0.0], [1.0 / w, 0.0])):
                if kind is None:
                    continue
                want_b, want_a = signal.bilinear(num, den, fs=sr)
                b, a = tm.coefficients(kind, fc, p, sr)
                assert np.allclose(b, want_b, rtol=0, atol=1e-12) and np.allclose(a, want_a, rtol=0, atol=1e-12), (kind, sr, fc, p)
        for kind, num in ((tm.LP1, [1.0]), (tm.HP1, [1.0 / w, 0.0])):
            want_b, want_a = signal.bilinear(num, [1.0 / w, 1.0], fs=sr)
            b, a = tm.coefficients(kind, fc, 0.0, sr)
            assert np.allclose(b[:2], want_b, rtol=0, atol=1e-12) and np.allclose(a[:2], want_a, rtol=0, atol=1e-12), (kind, sr, fc)
            assert b[2] == 0.0 and a[2] == 0.0


def test_headline_gains_of_the_truth():
    optimize = pytest.importorskip("scipy.optimize")
    for sr, fc, p in GRID:
        th = 2.0 * np.pi * fc / sr
        for kind, want in ((tm.LP2, 1.0 / p), (tm.HP2, 1.0 / p), (tm.SVF_LP, p), (tm.SVF_HP, p), (tm.SVF_BP, p),
                           (tm.LP1, np.sqrt(0.5)), (tm.HP1, np.sqrt(0.5))):
            assert abs(_gain(*tm.coefficients(kind, fc, p, sr), th) / want - 1.0) < 1e-12, (kind, sr, fc, p)
        for kind, dc, nyquist in ((tm.LP1, 1, 0), (tm.HP1, 0, 1), (tm.LP2, 1, 0), (tm.HP2, 0, 1), (tm.SVF_LP, 1, 0), (tm.SVF_HP, 0, 1),
                                  (tm.SVF_BP, 0, 0), (tm.BP2, 0, 0), (tm.ONEPOLE, 1, None)):
            if kind == tm.BP2 and th / (2.0 * p) >= np.pi / 4.0:
                continue
            b, a = tm.coefficients(kind, fc, p, sr)
            assert abs(_gain(b, a, 0.0) - dc) < 1e-12, (kind, sr, fc, p)
            assert nyquist is None or abs(_gain(b, a, np.pi) - nyquist) < 1e-12, (kind, sr, fc, p)
        if th / (2.0 * p) < np.pi / 4.0:
            # BP2: 0 dB at the centre; the two -3 dB points lie d_theta apart, tan(d_theta / 2) = t, t = tan(theta / (2 q))
            b, a = tm.coefficients(tm.BP2, fc, p, sr)
            assert abs(_gain(b, a, th) - 1.0) < 1e-12, (sr, fc, p)
            half = lambda x: _gain(b, a, x) ** 2 - 0.5
            lo, hi = optimize.brentq(half, 1e-9, th, xtol=1e-14), optimize.brentq(half, th, np.pi - 1e-9, xtol=1e-14)
            assert abs(np.tan((hi - lo) / 2.0) / np.tan(th / (2.0 * p)) - 1.0) < 1e-9, (sr, fc, p)
    # the SVF's cutoff stops at f32(0.49) sr
    for kind in (tm.SVF_LP, tm.SVF_BP, tm.SVF_HP):
        for got, want in zip(tm.coefficients(kind, 30000.0, 3.0, 48000), tm.coefficients(kind, float(np.float32(0.49)) * 48000, 3.0, 48000)):
            assert np.array_equal(got, want)
    # the one-pole: y = (1 - x) in + x y_-1, x = exp(-theta)
    b, a = tm.coefficients(tm.ONEPOLE, 1000.0, 0.0, 48000)
    assert b[0] == 1.0 - np.exp(-2.0 * np.pi * 1000.0 / 48000) and a[1] == -np.exp(-2.0 * np.pi * 1000.0 / 48000)


def test_decimator_truth_is_the_windowed_sinc():
    h = tm.decimator_taps()
    assert h.size == 63 and abs(h.sum() - 1.0) < 1e-15 and np.allclose(h, h[::-1], rtol=0, atol=1e-17)
    k = np.arange(63) - 31
    ideal = np.where(k == 0, 2 * 0.115, np.sin(2 * np.pi * 0.115 * k) / (np.pi * np.where(k == 0, 1, k)))
    w = 0.42 - 0.5 * np.cos(2 * np.pi * np.arange(63) / 62) + 0.08 * np.cos(4 * np.pi * np.arange(63) / 62)
    assert np.allclose(h, ideal * w / (ideal * w).sum(), rtol=0, atol=1e-16)
    # a DC input comes out as itself, an impulse at new sample 4 n comes out as h[62], h[58], ... from output n on
    out, _ = tm.decimate4(np.ones(62 + 40))
    assert np.allclose(out, 1.0, rtol=0, atol=1e-15)
    x = np.zeros(62 + 80); x[62] = 1.0
    out, _ = tm.decimate4(x)
    assert np.array_equal(out[:16], h[62::-4])


def test_case_table_shape():
    for sr in tm.RATES:
        cases = tm.filter_cases(sr)
        assert 110 <= len(cases) <= 255                         # one bank: program 0 is the pass-through
        assert {c.kind for c in cases} == set(range(9))
        assert sum(1 for c in cases if c.amount != 0.0) == 6 and {c.amount for c in cases} == {0.0, 4.0, -6.0}
        assert len(tm.reciprocal_pairs(cases)) == 8
        assert not any(c.kind == tm.BP2 and np.tan(np.pi * c.lpf_freq / sr / c.p) >= 1.0 for c in cases)
    assert tm.Case(tm.SVF_LP, 30000.0, 3.0, 0.0) in tm.filter_cases(48000)


# ------------------------------------------------------------------------------------------ (b) the oracle against the truth

def test_twin_rows_premises_hold_on_the_oracle(tool):
    """what makes the comparison oracle-free: the amplitude envelope at attack 0, decay 0 is its sustain from frame 0 (the row
    at sustain 1 is exactly twice the row at sustain 0.5), and a one-pole at 1e9 Hz is the identity whatever its state"""
    case = tm.Case(tm.SVF_BP, 1000.0, 3.0, 0.0)
    full = tm.patch_fields(case, tm.OSC_SAW)
    half = dict(full, **{"amp_env.sustain": 0.5})
    rows = tool.oracle_layer_rows([tool.oracle_cfg(full), tool.oracle_cfg(half)], 440.0, 48000, calls=1)
    assert np.array_equal(rows[0], 2.0 * rows[1]) and rows[0, 0] != 0.0
    cfg = tool.oracle_cfg(tm.patch_fields(tm.PASS_THROUGH, tm.OSC_SAW))
    L = s2o.lib()
    out = np.zeros((2, 256), dtype=np.float32)
    for i, last in enumerate((0.0, 123.0)):
        st = s2o.LayerState()
        st.has_phase = 1; st.lpf_last = last
        assert L.s2o_process_layer_buf_simd(C.byref(cfg), C.byref(st), 440.0, 48000, 0, 0, 0, s2o._fp(out[i]), 256) == 0
    assert np.array_equal(out[0], out[1]) and np.ptp(out[0]) > 1.0


def test_oracle_filters_stay_within_the_committed_bounds(measured, committed):
    for form in ("bank", "single"):
        assert sorted(measured[form]) == sorted(committed[form]), "the case table and %s differ: run tools/truth_blocks.py" % TABLE
        keys = sorted(committed[form])
        bounds = tm.bounds_for(committed[form], keys)           # (asserts the ceiling)
        got = np.array([measured[form][k] for k in keys])
        over = [(k, g, b) for k, g, b in zip(keys, got, bounds) if not g <= b]
        assert not over, over[:5]
    want = {tm.case_key(sr, name, c) for sr in tm.RATES for name, _, _ in tm.INPUTS for c in tm.filter_cases(sr)}
    assert set(committed["bank"]) == want and set(committed["single"]) == set(tm.KIND_NAMES)


def test_committed_deviations_reproduce(measured, committed):
    for form in ("bank", "single"):
        for k, have in committed[form].items():
            assert abs(have - measured[form][k]) <= 1e-6 * have, (k, have, measured[form][k])


def test_oracle_reciprocal_pairs_are_one_filter(tool, committed):
    """SVF_LP(q) and LP2(d = 1 / q) are one truth (likewise the high-passes): the two rows agree within the sum of their bounds"""
    for sr in tm.RATES:
        cases = tm.filter_cases(sr)
        for name, osc, pitch in tm.INPUTS:
            rows = tool.oracle_layer_rows([tool.oracle_cfg(tm.patch_fields(c, osc)) for c in [tm.PASS_THROUGH] + cases], pitch, sr)
            truth = tm.truth_rows(cases, sr, rows[0])
            bounds = tm.bounds_for(committed["bank"], [tm.case_key(sr, name, c) for c in cases])
            for i, j in tm.reciprocal_pairs(cases):
                assert np.array_equal(truth[i], truth[j])
                peak = np.maximum.accumulate(np.maximum(np.abs(truth[i]), 1e-30))
                assert np.max(np.abs(rows[1 + i].astype(np.float64) - rows[1 + j]) / peak) <= bounds[i] + bounds[j], (sr, name, cases[i])


@pytest.mark.parametrize("sr", tm.RATES)
def test_oracle_dpw_rows_are_the_naive_rows_plus_the_closed_form(tool, sr):
    for naive, dpw in tm.DPW_PAIRS:
        for pitch in tm.DPW_PITCHES[sr]:
            cfgs = [tool.oracle_cfg(tm.patch_fields(tm.PASS_THROUGH, k)) for k in (dpw, naive)]
            rows = tool.oracle_layer_rows(cfgs, pitch, sr)
            worst, first, kept = tm.dpw_compare(rows[0], rows[1], naive, pitch, sr)
            assert kept >= 0.90, (naive, pitch, kept)
            assert worst <= 1.0 and first <= 1.0, (naive, pitch, worst, first)


def test_oracle_decimator_against_the_f64_convolution():
    rng = np.random.RandomState(5)
    x = np.concatenate([np.zeros(62), rng.uniform(-4.0, 4.0, 4 * 532)]).astype(np.float32)
    truth, scale = tm.decimate4(x)
    got = s2o.decimate4(x, 532)
    assert np.all(np.abs(got - truth) <= tm.DECIM_BOUND_ULPS * scale)
    # the worst relative rounding of a tap is below 2^-24 (part of the bound's derivation)
    assert np.max(np.abs(s2o.decim4_taps().astype(np.float64) / tm.decimator_taps() - 1.0)) < 2.0 ** -24
    # and the bound notices one sample of misalignment
    shifted = s2o.decimate4(np.concatenate([x[1:], x[:1]]), 532)
    assert np.any(np.abs(shifted - truth) > tm.DECIM_BOUND_ULPS * scale)
