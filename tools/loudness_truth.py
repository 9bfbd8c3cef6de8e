"""Measures how far the loudness meters' binary32 rule (s2r_loudness_reference, s2r_loudness_readings) lies from a binary64 model of the
same rule on the signals of tests/test_loudness_host.py — a 997 Hz sine at full scale, the fs/4 sine at 45 degrees, a 50 Hz tone at
-40 dB, noise — and writes the deviations and twice each, the bound the tests hold the library to, into
profiles/truth/loudness_deviation.json (the convention of profiles/truth/blocks_deviation.json).  No device needed.

    python tools/loudness_truth.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_loudness_host as t  # noqa: E402


def main():
    signals = []
    for name, sr, frames in t.SIGNALS:
        m = t.measure(name, sr, frames)
        m["bound_lu"] = 2.0 * m["reference_deviation_lu"]
        m["bound_true_peak"] = 2.0 * m["reference_deviation_true_peak"]
        signals.append(m)
        print("%-26s deviation %.3e LU, true peak %.3e; integrated %.4f LKFS, true peak %s" % (
            name, m["reference_deviation_lu"], m["reference_deviation_true_peak"], m["readings"][2], m["true_peak"]))
    doc = {"what": "deviation of the loudness meters' binary32 rule (s2r_loudness_reference + s2r_loudness_readings on the master of a stream in one "
                   "call, hop = sample_rate / 10) from the same rule in numpy float64 over the binary32 coefficients and taps: the largest of the "
                   "momentary, short-term and integrated readings' in LU, and the true peak's relative to the model's; bound = 2 x that; the library "
                   "is held to the bounds (tests/test_loudness_host.py)",
           "signals": signals}
    with open(t.TRUTH, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
