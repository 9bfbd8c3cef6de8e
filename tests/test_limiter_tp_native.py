"""ASan + UBSan over the host side of the master limiter's true-peak detector, which needs neither a handle nor HIP:
s2r_limiter_tp_reference (csrc/s2r_rules.cpp) beside tests/native/san_limiter_tp.cpp, compiled by plain g++ and run as a child process,
with no preload of any kind — as tests/test_resampler_native.py does."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_limiter_tp_reference_under_asan_ubsan(tmp_path):
    """the pairs (1, 0), (48, 0) and (1024, 4096) with calls of 0, 1, 9 and 1000 frames on buffers of exactly the stated sizes: the
    calls in a row equal one call on bits, the ceiling holds, the delay of L + 8 in every bit, null outputs and y == x, and refusals
    that touch nothing"""
    exe = str(tmp_path / "san_limiter_tp")
    subprocess.check_call(SAN + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                                 os.path.join(ROOT, "tests", "native", "san_limiter_tp.cpp"),
                                 os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "limiter tp ok" in out.stdout
