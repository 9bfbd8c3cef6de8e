"""The GPU's own rows against the independent binary64 models of tests/truth_model.py — no oracle in the loop.  For the
dsp_filters.rs filters, the SVF outputs, the DPW shapes and the 4x decimator the oracle is the only definition and was
written together with the kernels, so bit parity with it (tests/test_gpu_parity.py) cannot see a mistake the two share: a Q
read from the wrong field, a swapped SVF output, a decimator one tap out of line, a DPW scale of `period` for `period / 2`.

Twin rows make the filter's input visible: every case is rendered next to a layer with the same oscillator, pitch, phase, seed
and offset whose filter is a one-pole at 1e9 Hz (x = expf(-huge) = 0, y = fma(1, input, +-0) = input) and whose amplitude
envelope is 1 from frame 0.  That row is the exact f32 sequence the case's filter consumed; the model filters it in binary64.
The bound of a case is twice the ORACLE's deviation from the same model (profiles/truth/blocks_deviation.json, measured on
the CPU by tools/truth_blocks.py and re-checked by tests/test_truth_blocks.py); nothing in it comes from the GPU."""
import json
import os

import numpy as np
import pytest

import synth2_amd as s2
import truth_model as tm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def committed():
    return json.load(open(os.path.join(ROOT, "profiles", "truth", "blocks_deviation.json")))


def _patch(fields):
    p = s2.default_patch()
    for k, v in fields.items():
        if "." in k:
            a, b = k.split(".")
            setattr(getattr(p, a), b, v)
        else:
            setattr(p, k, v)
    return p


def _bank_rows(ws, programs, pitch_hz, sr, calls=tm.CALLS, frames=tm.CALL_FRAMES):
    """one fresh layer per program (phase 0, seed 0, filter state 0, no DPW memory) through s2r_process_layers, `calls` calls
    continuing the states"""
    layers = np.zeros(len(programs), dtype=s2.LAYER_CALL_DTYPE)
    layers["pitch_hz"] = np.broadcast_to(np.asarray(pitch_hz, dtype=np.float32), layers.shape)
    layers["program"] = programs
    layers["osc_z"] = np.float32(np.nan)
    out = []
    for _ in range(calls):
        out.append(ws.process_layers(layers, frames, sr))
        layers["offset"] += frames
    return np.concatenate(out, axis=1)


def _assert_within(dev, bounds, keys, what):
    ratio = dev / bounds
    worst = int(np.argmax(ratio))
    print("%s: %d cases, worst deviation / bound %.3f at %s (%.3g of the running peak)" % (what, len(keys), ratio[worst], keys[worst], dev[worst]))
    over = [(k, float(d), float(b)) for k, d, b in zip(keys, dev, bounds) if not d <= b]
    assert not over, "%s: %d of %d cases beyond their bound, first %s" % (what, len(over), len(keys), over[:3])


@pytest.mark.parametrize("coeff_stream", [1, 0])
@pytest.mark.parametrize("input_name,osc,pitch", tm.INPUTS)
@pytest.mark.parametrize("sr", tm.RATES)
def test_bank_filters_against_the_f64_truth(committed, sr, input_name, osc, pitch, coeff_stream):
    """all nine filter kinds over the case table, the six constant-modulation cases included, through the bank kernel; with
    the coefficients read from the patch's tables (1) and computed in-lane (0)"""
    cases = tm.filter_cases(sr)
    keys = [tm.case_key(sr, input_name, c) for c in cases]
    bounds = tm.bounds_for(committed["bank"], keys)
    ws = s2.Synth(256, max_frames=tm.CALL_FRAMES)
    ws.set_patch_bank([_patch(tm.patch_fields(c, osc)) for c in [tm.PASS_THROUGH] + cases])
    ws.set_coeff_stream(coeff_stream)
    rows = _bank_rows(ws, np.arange(1 + len(cases)), pitch, sr)
    ws.close()
    assert np.all(np.isfinite(rows)) and np.ptp(rows[0]) > 1.0
    truth = tm.truth_rows(cases, sr, rows[0])
    _assert_within(tm.deviation(rows[1:], truth), bounds, keys, "bank, %d Hz, %s, coeff_stream %d" % (sr, input_name, coeff_stream))
    # SVF_LP(q) and LP2(d = 1 / q) are one and the same truth, and so are the two high-passes
    for i, j in tm.reciprocal_pairs(cases):
        assert np.array_equal(truth[i], truth[j])
        peak = np.maximum.accumulate(np.maximum(np.abs(truth[i]), 1e-30))
        assert np.max(np.abs(rows[1 + i].astype(np.float64) - rows[1 + j]) / peak) <= bounds[i] + bounds[j], (keys[i], keys[j])


def _single_rows(fields, notes, sr, calls, frames=tm.CALL_FRAMES):
    syn = s2.Synth(tm.SINGLE_VOICES, max_frames=frames)
    syn.set_patch(_patch(fields))
    voices = [syn.note_on(n) for n in notes]
    pitches = syn.export_state()["pitch_hz"][voices]
    rows = np.concatenate([syn.render_voices(frames, sr) for _ in range(calls)], axis=1)
    syn.close()
    return rows, voices, pitches


@pytest.mark.parametrize("kind", range(9), ids=tm.KIND_NAMES)
def test_single_patch_filters_against_the_f64_truth(committed, kind):
    """the per-oscillator render kernels of a handle with ONE patch, which the bank kernel's cases do not reach: 64 voices, a
    note each, pass-through handle against filter handle, voice by voice"""
    case = tm.Case(kind, tm.SINGLE_FC, tm.SINGLE_P, 0.0)
    osc = tm.SINGLE_OSCS[kind % 4]
    a, va, _ = _single_rows(tm.patch_fields(tm.PASS_THROUGH, osc), tm.SINGLE_NOTES, 48000, tm.SINGLE_CALLS)
    b, vb, _ = _single_rows(tm.patch_fields(case, osc), tm.SINGLE_NOTES, 48000, tm.SINGLE_CALLS)
    assert va == vb and sorted(va) == list(range(tm.SINGLE_VOICES))
    assert np.all(np.isfinite(b)) and np.all(np.ptp(a, axis=1) > 1.0)
    bq, aq = tm.coefficients(kind, tm.case_cutoff(case), tm.F32(case.p), 48000)
    truth = tm.run_biquads(np.tile(bq, (len(a), 1)), np.tile(aq, (len(a), 1)), a)
    bound = tm.bounds_for(committed["single"], [tm.KIND_NAMES[kind]])[0]
    dev = tm.deviation(b, truth)
    _assert_within(dev, np.full(len(dev), bound), ["%s, voice %d" % (tm.KIND_NAMES[kind], v) for v in range(len(dev))], "single patch")


def _assert_dpw(dpw_row, naive_row, naive, pitch, sr, what):
    worst, first, kept = tm.dpw_compare(dpw_row, naive_row, naive, pitch, sr)
    print("%s: worst %.3f and frame 0 %.3f of the tolerance, %.1f %% of frames compared" % (what, worst, first, 100.0 * kept))
    assert kept >= 0.90, (what, kept)                  # a mask that hid more could hide a failure
    assert worst <= 1.0, (what, worst)
    assert first <= 1.0, (what, first)


@pytest.mark.parametrize("sr", tm.RATES)
def test_bank_dpw_rows_are_the_naive_rows_plus_the_closed_form(sr):
    """DPW saw = naive saw + 1 / period, DPW square = naive square, DPW triangle = naive triangle +- 2 / period away from the
    naive shape's discontinuities; frame 0 is 0.  The twins share their phase sequence bit for bit, so drift cancels."""
    ws = s2.Synth(256, max_frames=tm.CALL_FRAMES)
    kinds = [k for pair in tm.DPW_PAIRS for k in pair]
    ws.set_patch_bank([_patch(tm.patch_fields(tm.PASS_THROUGH, k)) for k in kinds])
    pitches = tm.DPW_PITCHES[sr]
    programs = np.tile(np.arange(len(kinds)), len(pitches))
    rows = _bank_rows(ws, programs, np.repeat(pitches, len(kinds)), sr, calls=tm.DPW_FRAMES // tm.CALL_FRAMES)
    ws.close()
    for ip, pitch in enumerate(pitches):
        for ik, (naive, dpw) in enumerate(tm.DPW_PAIRS):
            base = ip * len(kinds) + 2 * ik
            _assert_dpw(rows[base + 1], rows[base], naive, pitch, sr, "bank, %d Hz, shape %d at %g Hz" % (sr, naive, pitch))


@pytest.mark.parametrize("sr", tm.RATES)
@pytest.mark.parametrize("naive,dpw", tm.DPW_PAIRS)
def test_single_patch_dpw_rows_are_the_naive_rows_plus_the_closed_form(naive, dpw, sr):
    pitches = tm.DPW_PITCHES[sr]
    notes = [tm.DPW_NOTES[p] for p in pitches]
    calls = tm.DPW_FRAMES // tm.CALL_FRAMES
    a, va, pa = _single_rows(tm.patch_fields(tm.PASS_THROUGH, dpw), notes, sr, calls)
    b, vb, pb = _single_rows(tm.patch_fields(tm.PASS_THROUGH, naive), notes, sr, calls)
    assert va == vb and list(pa) == list(pitches) and list(pb) == list(pitches)      # the A notes' pitches are exact
    for v, pitch in zip(va, pitches):
        _assert_dpw(a[v], b[v], naive, pitch, sr, "single patch, %d Hz, shape %d at %g Hz" % (sr, naive, pitch))


@pytest.mark.parametrize("patch_name", ["dpw_saw_svf", "default"])
def test_decimator_against_the_f64_convolution(patch_name):
    """s2r_fill_oversampled at 48 kHz against the binary64 63-tap convolution of what a twin handle's s2r_fill returns at
    192 kHz, history carried across calls of 256, 1, 3, 17 and 255 frames; every sample within the first-order rounding bound
    of 63 sequentially accumulated f32 products and the f32 rounding of the taps"""
    patch = s2.default_patch() if patch_name == "default" else _patch(
        {"osc_kind": tm.OSC_DPW_SAW, "lpf_kind": tm.SVF_LP, "lpf_freq": 4000.0, "lpf_q": 1.2, "mod_env_to_lpf_freq": 2.0})
    over, plain = (s2.Synth(tm.SINGLE_VOICES, max_frames=1024) for _ in range(2))
    for syn in (over, plain):
        syn.set_patch(patch)
        for note in range(40, 88, 3):
            syn.note_on(note)
    got, x = [], [np.zeros(tm.DECIM_TAPS - 1, dtype=np.float32)]
    for k, n in enumerate(tm.DECIM_CALLS):
        got.append(over.sample_oversampled(n, 48000))
        x.append(plain.sample(4 * n, 192000))
        for syn in (over, plain):                               # events between the calls
            syn.note_off(40 + 3 * k)
            syn.note_on(90 + k)
    over.close(); plain.close()
    got, x = np.concatenate(got), np.concatenate(x)
    truth, scale = tm.decimate4(x)
    assert np.ptp(x) > 1.0 and np.all(np.isfinite(got))
    err = np.abs(got - truth)
    print("decimator, %s: worst error %.3f of the bound over %d samples" % (patch_name, np.max(err / np.maximum(scale * tm.DECIM_BOUND_ULPS, 1e-300)), got.size))
    assert np.all(err <= tm.DECIM_BOUND_ULPS * scale), int(np.argmax(err - tm.DECIM_BOUND_ULPS * scale))
