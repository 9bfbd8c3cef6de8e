"""ASan + UBSan over the sample-rate converter's host side, which needs neither a handle nor HIP:
s2r_resampler_reference, s2r_resampler_count and s2r_resampler_design (csrc/s2r_rules.cpp) beside tests/native/san_resampler.cpp,
compiled by plain g++ and run as a child process, with no preload of any kind — as tests/test_pcm_native.py does."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_resampler_host_functions_under_asan_ubsan(tmp_path):
    """the three functions at the edges of their shapes — the ratios 1/1 to 147/320 and both ends of the table budget; T 4; calls of
    0, 1, T - 2, T - 1, T and 1000 frames; 0, 3 and 8 buses; ph at 0 and M - 1 — on buffers of exactly the stated sizes, a stream in
    one call and in two, the answers that need no model, and refusals that touch nothing"""
    exe = str(tmp_path / "san_resampler")
    subprocess.check_call(SAN + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                                 os.path.join(ROOT, "tests", "native", "san_resampler.cpp"),
                                 os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "resampler ok" in out.stdout
