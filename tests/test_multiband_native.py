"""ASan + UBSan over the host side of the master multiband compressor, which needs neither a handle nor HIP:
s2r_multiband_reference and s2r_multiband_design (csrc/s2r_rules.cpp) beside tests/native/san_multiband.cpp, compiled by plain g++ and
run as a child process, with no preload of any kind — as tests/test_limiter_tp_native.py does."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_multiband_reference_and_design_under_asan_ubsan(tmp_path):
    """1 .. 4 bands with calls of 0, 1, 9 and 500 frames on buffers of exactly the stated sizes, arrays of no rows as NULL: the calls in
    a row equal one call on bits, unit curves leave gains of exactly 1, null optional outputs, and refusals that touch nothing"""
    exe = str(tmp_path / "san_multiband")
    subprocess.check_call(SAN + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                                 os.path.join(ROOT, "tests", "native", "san_multiband.cpp"),
                                 os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "multiband ok" in out.stdout
