"""Measures the response of the sample-rate converter's designs on the float64 restatement of s2r_resampler_design
(tests/resampler_model.py: np.kaiser, np.sinc — never the library) on the cases of tests/test_resampler_host.py, and writes the worst
passband and stopband figures of each into profiles/truth/resampler_deviation.json: the response of the interleaved prototype from a
2^18-point FFT, the passband up to 0.8 of the lower Nyquist, the stopband from 1.2 of it.  The test holds the library's tables to
these figures plus 0.05 dB and 3 dB (the FFT grid's own resolution).  No device needed.

    python tools/resampler_truth.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import resampler_model as m  # noqa: E402

DESIGNS = [(147, 160, 32, 10.0, 0.9), (160, 147, 32, 10.0, 0.9), (1, 2, 64, 10.0, 0.9), (2, 1, 32, 10.0, 0.9), (2, 3, 48, 10.0, 0.9), (147, 320, 64, 10.0, 0.9),
           (147, 160, 48, 12.0, 0.92)]


def main():
    designs = {}
    for L, M, T, beta, rolloff in DESIGNS:
        _, h = m.design64(L, M, T, beta, rolloff)
        hi, lo, stop = m.response_db(h.astype(np.float32), L, M)
        name = "%d/%d T%d beta%g rolloff%g" % (L, M, T, beta, rolloff)
        designs[name] = {"passband_high_db": round(hi, 5), "passband_low_db": round(lo, 5), "stopband_db": round(stop, 2)}
        print("%-34s passband %+.5f / %+.5f dB, stopband %.2f dB" % (name, hi, lo, stop))
    doc = {"what": "response of the float64 restatement of s2r_resampler_design (np.kaiser, np.sinc, rows normalised, rounded to binary32): the "
                   "interleaved prototype's magnitude from a 2^18-point FFT, gain L taken out; passband up to 0.8 of the lower Nyquist, stopband "
                   "from 1.2 of it; the library's tables are held to these plus 0.05 dB and 3 dB (tests/test_resampler_host.py)",
           "designs": designs}
    with open(os.path.join(ROOT, "profiles", "truth", "resampler_deviation.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
