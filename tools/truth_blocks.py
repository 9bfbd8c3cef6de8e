#!/usr/bin/env python3
"""How far the oracle's dsp_filters.rs filters, SVF outputs and one-pole are from a binary64 model of the same filters
(tests/truth_model.py, written from the textbook and not from the oracle), case by case, on the input the filter really saw.

The filter's input is not visible from outside, so every case is rendered twice with the same oscillator, pitch, phase, seed
and offset: once through a one-pole at 1e9 Hz (x = expf(-huge) = 0: the filter returns its input, exactly) and once through
the filter under test.  The first row is the exact f32 sequence the second row's filter consumed; the model filters it in
binary64 and the distance is reported as max |row - truth| / running peak of |truth|.

CPU only; nothing here comes from the GPU.  tests/test_truth_blocks.py recomputes these figures and holds them against the
committed file; tests/test_gpu_truth_blocks.py holds the GPU's own rows to twice each figure, with no oracle in the loop.

    python tools/truth_blocks.py [profiles/truth/blocks_deviation.json]
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import s2o          # noqa: E402   (test infrastructure)
import truth_model as tm        # noqa: E402

OUT = os.path.join(ROOT, "profiles", "truth", "blocks_deviation.json")


def oracle_cfg(fields):
    c = s2o.lib().s2o_default_config()
    for k, v in fields.items():
        if "." in k:
            a, b = k.split(".")
            setattr(getattr(c, a), b, v)
        else:
            setattr(c, k, v)
    return c


def oracle_layer_rows(cfgs, pitch_hz, sr, calls=tm.CALLS, frames=tm.CALL_FRAMES):
    """process_layer_buf_simd per config from a fresh state (phase 0, seed 0, no DPW memory), `calls` calls continuing it"""
    L = s2o.lib()
    rows = np.zeros((len(cfgs), calls * frames), dtype=np.float32)
    for i, cfg in enumerate(cfgs):
        st = s2o.LayerState()
        st.has_phase = 1
        for k in range(calls):
            rc = L.s2o_process_layer_buf_simd(C.byref(cfg), C.byref(st), pitch_hz, sr, k * frames, 0, 0,
                                              s2o._fp(rows[i, k * frames:]), frames)
            assert rc == 0
    return rows


def bank_deviations(sr, input_name, osc_kind, pitch_hz):
    cases = tm.filter_cases(sr)
    cfgs = [oracle_cfg(tm.patch_fields(c, osc_kind)) for c in [tm.PASS_THROUGH] + cases]
    rows = oracle_layer_rows(cfgs, pitch_hz, sr)
    dev = tm.deviation(rows[1:], tm.truth_rows(cases, sr, rows[0]))
    return {tm.case_key(sr, input_name, c): float(d) for c, d in zip(cases, dev)}


def single_rows(case, osc_kind, sr=48000):
    """the single-patch form: 64 voices, one note each, per-voice rows"""
    syn = s2o.OracleSynth(tm.SINGLE_VOICES)
    syn.config = oracle_cfg(tm.patch_fields(case, osc_kind))
    for note in tm.SINGLE_NOTES:
        syn.note_on(note)
    return np.concatenate([syn.render_voices(tm.CALL_FRAMES, sr) for _ in range(tm.SINGLE_CALLS)], axis=1)


def single_deviation(kind, sr=48000):
    case = tm.Case(kind, tm.SINGLE_FC, tm.SINGLE_P, 0.0)
    osc = tm.SINGLE_OSCS[kind % 4]
    a, b = single_rows(tm.PASS_THROUGH, osc, sr), single_rows(case, osc, sr)
    bq, aq = tm.coefficients(kind, tm.case_cutoff(case), tm.F32(case.p), sr)
    truth = tm.run_biquads(np.tile(bq, (a.shape[0], 1)), np.tile(aq, (a.shape[0], 1)), a)
    return float(tm.deviation(b, truth).max())


def measure():
    bank = {}
    for sr in tm.RATES:
        for name, osc, pitch in tm.INPUTS:
            bank.update(bank_deviations(sr, name, osc, pitch))
    single = {tm.KIND_NAMES[k]: single_deviation(k) for k in range(9)}
    return {"what": "oracle vs the binary64 model of tests/truth_model.py: max |row - truth| / running peak of |truth| per case; "
                    "a case's bound is max(%g x this, 2^-24), never above %g" % (tm.BOUND_FACTOR, tm.BOUND_CEILING),
            "frames": tm.CALLS * tm.CALL_FRAMES, "bank": bank, "single": single}


if __name__ == "__main__":
    r = measure()
    worst = max(r["bank"], key=r["bank"].get)
    print("%d bank cases, worst %s: %.3g; single-patch form: %s" % (
        len(r["bank"]), worst, r["bank"][worst], ", ".join("%s %.3g" % kv for kv in r["single"].items())))
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(r, indent=1) + "\n")
