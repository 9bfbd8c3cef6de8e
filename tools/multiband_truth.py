"""Measures what the master multiband compressor's crossover deviates by, on the restatement of the rule in
tests/multiband_model.py — never the library —, and writes profiles/truth/multiband_deviation.json.  Signals: 4096 frames of white
noise (seed 2031, peak 0.5) and a logarithmic sine sweep from 20 Hz to 20 kHz (peak 0.5), stereo with the right channel negated and
halved.  Splits at 200 / 1500 / 6000 Hz (the tests') and at 120 / 1000 / 6000 Hz, 48 kHz.  All figures are maxima of absolute
differences over both channels, divided by the input's peak:

  identity64   the unit-gain band sum of the binary64 tree with binary64 coefficients against the allpass cascade
               AP_{B-2}( ... AP_0(x)), also in binary64: that the tree is sound
  rounded64    the same sum with the coefficients rounded to binary32, evaluated in binary64, against that cascade: what the rounding
               of the fifteen coefficient rows costs
  rule32       the rule's binary32 frame loop (numpy, unit curves) against the binary64 evaluation with the same binary32 coefficients:
               what binary32 arithmetic costs
  sum32        the rule's binary32 frame loop against the binary64 allpass cascade with binary64 coefficients: both together

tests/test_multiband_host.py holds the LIBRARY's unit-gain sum, on noise of another seed and the same sweep, to `bound`: twice the
largest sum32 of the band count.  No device needed.

    python tools/multiband_truth.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multiband_model as m  # noqa: E402

SR = 48000.0
N = 4096
SPLIT_SETS = {"200/1500/6000": [200.0, 1500.0, 6000.0], "120/1000/6000": [120.0, 1000.0, 6000.0]}


def signals(seed=2031, n=N):
    rng = np.random.default_rng(seed)
    noise = rng.uniform(-0.5, 0.5, n)
    t = np.arange(n) / SR
    dur = n / SR
    sweep = 0.5 * np.sin(2.0 * np.pi * 20.0 * dur / np.log(1000.0) * (np.exp(t / dur * np.log(1000.0)) - 1.0))
    return {name: np.stack([v, -0.5 * v], axis=1).astype(np.float32) for name, v in (("noise", noise), ("sweep", sweep))}


def measure(B, splits, x):
    lp64, hp64, ap64 = m.design64(SR, splits[:B - 1])
    lp32, hp32, ap32 = (c.astype(np.float32) for c in (lp64, hp64, ap64))
    peak = float(np.abs(x).max())
    cascade = m.allpass64(ap64, x)
    exact = m.tree64(B, lp64, hp64, ap64[1:], x).sum(axis=0)
    rounded = m.tree64(B, lp32, hp32, ap32[1:], x).sum(axis=0)
    unit = np.ones((B, m.POINTS), dtype=np.float32)
    state = np.zeros(4 * m.sections(B) + B, dtype=np.float32)
    state[-B:] = 1.0
    rule = m.np32(B, lp32, hp32, ap32[1:], unit, np.zeros(B), np.zeros(B), x, state)[0].astype(np.float64)
    d = lambda a, b: float(np.abs(a - b).max()) / peak
    return {"identity64": d(exact, cascade), "rounded64": d(rounded, cascade), "rule32": d(rule, rounded), "sum32": d(rule, cascade)}


def main():
    cases, bound = {}, {}
    for B in (2, 3, 4):
        worst = 0.0
        for set_name, splits in SPLIT_SETS.items():
            for sig_name, x in signals().items():
                r = measure(B, splits, x)
                cases["%d bands, %s Hz, %s" % (B, "/".join(set_name.split("/")[:B - 1]), sig_name)] = {k: float("%.3e" % v) for k, v in r.items()}
                worst = max(worst, r["sum32"])
                print("%d bands %-14s %-6s identity64 %.2e  rounded64 %.2e  rule32 %.2e  sum32 %.2e" % (B, set_name, sig_name, r["identity64"], r["rounded64"], r["rule32"], r["sum32"]))
        bound[str(B)] = float("%.3e" % (2.0 * worst))
    doc = {"what": "the master multiband compressor's crossover on the restatement of tests/multiband_model.py (never the library), 4096 frames at 48 kHz, "
                   "maxima of absolute differences over the input's peak: identity64 the binary64 band sum against the binary64 allpass cascade; rounded64 "
                   "the same with the coefficients rounded to binary32; rule32 the rule's binary32 loop against binary64 arithmetic on the same "
                   "coefficients; sum32 the binary32 loop against the binary64 cascade.  bound[B] = twice the largest sum32 at B bands: what "
                   "tests/test_multiband_host.py holds the library's unit-gain sum to, on noise of another seed and the same sweep",
           "bound": bound, "cases": cases}
    with open(os.path.join(ROOT, "profiles", "truth", "multiband_deviation.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
