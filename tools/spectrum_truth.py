"""Measures how far the spectrum meter's binary32 rule (s2r_spectrum_reference) lies from numpy's float64 FFT of the same windowed
frames, on the cases of tests/test_spectrum_host.py — seeded noise through Hann and Blackman-Harris windows at N = 256, 2048 and 8192 —
and writes the largest |p - truth| / max(truth) of each case into profiles/truth/spectrum_deviation.json.  The test allows twice the
committed figure (the convention of profiles/truth/loudness_deviation.json).  No device needed.

    python tools/spectrum_truth.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_spectrum_host as t  # noqa: E402


def main():
    cases = {}
    for name, n, hop, kind in t.deviation_cases():
        cases[name] = t.measure_deviation(n, hop, kind)
        print("%-28s deviation %.3e of the row's largest bin" % (name, cases[name]))
    doc = {"what": "deviation of the spectrum meter's binary32 rule (s2r_spectrum_reference over seeded noise, one bus and the master, hop = N / 2) "
                   "from numpy.fft.fft in float64 of the same windowed frames: the largest |p[k] - truth[k]| over the rows, relative to the row's "
                   "largest truth[k]; the library is held to twice each figure (tests/test_spectrum_host.py)",
           "cases": cases}
    with open(t.DEVIATION, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
