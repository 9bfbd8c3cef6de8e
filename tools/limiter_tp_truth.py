"""Measures how far the true peak of the master limiter's output exceeds the ceiling under the true-peak detector, on a
float64 numpy evaluation of the rule written here — never the library —, and writes the largest excess e into
profiles/truth/limiter_tp_deviation.json.  The gain moves inside the interpolator's span, so the interpolation of the limited signal
is not the limited interpolation: the rule bounds the samples exactly and the true peak nearly.  Signals of 6000 frames: an fs/4 sine
at a phase of 45 degrees (its samples miss every crest by 3 dB), seeded noise, a naive square at 1661.2 Hz and 48 kHz; pairs
(lookahead, hold) = (48, 0) and (16, 8); the ceiling half of each signal's sample peak; the true peak read as the loudness meter reads
it (4.26: the samples and the four phases of g = 4 h), in float64.  The sample-peak rule's reading on the same signals is recorded
beside it.  tests/test_limiter_tp_host.py holds the library's binary32 rule to 1 + 2 e.  No device needed.

    python tools/limiter_tp_truth.py
"""
import json
import os

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS, LATENCY, HISTORY = 65, 8, 16
FRAMES = 6000
PAIRS = [(48, 0), (16, 8)]
SHORT = [(5, 3)]                                                  # recorded beside them, not part of e: a lookahead shorter than the interpolator's span


def taps64():
    """g = 4 h of the drive's prototype: a Blackman-windowed sinc, cutoff 0.115, unit DC gain, each tap rounded to
    binary32 once — the rule's constants —, as float64"""
    k = np.arange(TAPS)
    at = (k - (TAPS - 1) // 2).astype(np.float64)
    safe = np.where(at == 0.0, 1.0, at)
    ideal = np.where(at == 0.0, 2.0 * 0.115, np.sin(2.0 * np.pi * 0.115 * at) / (np.pi * safe))
    w = 0.42 - 0.5 * np.cos(2.0 * np.pi * k / (TAPS - 1)) + 0.08 * np.cos(4.0 * np.pi * k / (TAPS - 1))
    d = ideal * w
    d[TAPS // 2 + 1:] = d[:TAPS // 2][::-1]                       # the second half mirrors the first, on bits
    h = (d / d.sum()).astype(np.float32)
    return (np.float32(4.0) * h).astype(np.float64)


def signals(frames=FRAMES):
    """{name: x [frames, 2] float32}; the right channel is the left at half the level, the noise's its own"""
    n = np.arange(frames)
    sine = 0.5 * np.sin(2.0 * np.pi * n / 4.0 + np.pi / 4.0)
    square = 0.5 * np.where(np.sin(2.0 * np.pi * 1661.2 * n / 48000.0) >= 0.0, 1.0, -1.0)
    noise = np.random.default_rng(30).standard_normal((frames, 2)) * 0.3
    return {"sine fs/4 at 45 degrees": np.stack([sine, 0.5 * sine], axis=1).astype(np.float32),
            "noise": noise.astype(np.float32),
            "square 1661.2 Hz": np.stack([square, 0.5 * square], axis=1).astype(np.float32)}


def phases64(x, g):
    """u [4, N, 2]: the four phases of the interpolator over x [N, 2] behind 16 frames of silence"""
    xe = np.concatenate([np.zeros((HISTORY, 2)), x.astype(np.float64)])
    N = len(x)
    u = np.zeros((4, N, 2))
    for p in range(4):
        for j in range(HISTORY + 1):
            if p + 4 * j < TAPS:
                u[p] += g[p + 4 * j] * xe[HISTORY - j:HISTORY - j + N]
    return u


def true_peak64(y, g):
    """the meter's reading of y [N, 2], both channels together"""
    return max(float(np.abs(y).max()), float(np.abs(phases64(y, g)).max()))


def limiter64(x, C, L, H, true_peak, g):
    """the rule (4.18; 4.30 with true_peak) in float64 from the initial state: y [N, 2]"""
    x = x.astype(np.float64)
    N, W, G = len(x), L + 1, 2 * L + H
    delay = L + (LATENCY if true_peak else 0)
    xe = np.concatenate([np.zeros((delay, 2)), x])
    if true_peak:
        d = np.maximum(np.abs(xe[L:L + N]).max(axis=1), np.abs(phases64(x, g)).max(axis=(0, 2)))      # |x[n - 8]| and the phases
    else:
        d = np.abs(x).max(axis=1)
    gain = np.where(d > C, C / np.maximum(d, 1e-300), 1.0)
    ge = np.concatenate([np.ones(G), gain])
    m = sliding_window_view(ge, L + H + 1).min(axis=1)           # m[j] is m[n = j - L]
    s = np.convolve(m, np.ones(W))[W - 1:W - 1 + N] / W
    sp = np.minimum(s, ge[G - L:G - L + N])
    return np.clip(xe[:N] * sp[:, None], -C, C)


def main():
    g = taps64()
    rows, e = {}, 0.0
    for name, x in signals().items():
        C = 0.5 * float(np.abs(x).max())
        for L, H in PAIRS + SHORT:
            tp = true_peak64(limiter64(x, C, L, H, True, g), g) / C
            sample = true_peak64(limiter64(x, C, L, H, False, g), g) / C
            rows["%s (%d, %d)" % (name, L, H)] = {"true_peak_over_ceiling": round(tp, 6), "sample_peak_rule_over_ceiling": round(sample, 6)}
            print("%-24s (%2d, %d): true-peak detector %.6f C, sample-peak rule %.6f C" % (name, L, H, tp, sample))
            if (L, H) in PAIRS:
                e = max(e, tp - 1.0)
    doc = {"what": "the loudness meter's true peak (DESIGN.md 4.26) of the master limiter's output over its ceiling, by a float64 numpy evaluation of the "
                   "rule with the true-peak detector (4.30) and with the sample-peak rule (4.18), 6000 frames, the ceiling half the sample peak; e is "
                   "the largest excess of the true-peak detector at (48, 0) and (16, 8) — (5, 3) is recorded, not counted —; the library's binary32 rule is held to 1 + 2 e (tests/test_limiter_tp_host.py, "
                   "tests/test_gpu_limiter_tp.py)",
           "e": round(e + 5e-7, 6), "cases": rows}
    with open(os.path.join(ROOT, "profiles", "truth", "limiter_tp_deviation.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("e = %.6f" % doc["e"])


if __name__ == "__main__":
    main()
