"""ASan + UBSan over the PCM stage's host side, which needs neither a handle nor HIP: s2r_pcm_reference,
s2r_pcm_dither, s2r_pcm_pack and s2r_pcm_shaper (csrc/s2r_rules.cpp) beside tests/native/san_pcm.cpp, compiled by plain g++ and run
as a child process, with no preload of any kind — as tests/test_spectrum_native.py does."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_pcm_host_functions_under_asan_ubsan(tmp_path):
    """the four functions at the edges of their shapes — 0, 1, 2, 5 and 9 taps; 8, 16 and 24 bits; the three dither kinds; calls of 0,
    1, K - 1, K, K + 1 and 1000 frames; 0, 2 and 8 buses; t across the wrap — on buffers of exactly the stated sizes, a stream in one
    call and in two, the answers that need no model, and refusals that touch nothing"""
    exe = str(tmp_path / "san_pcm")
    subprocess.check_call(SAN + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                                 os.path.join(ROOT, "tests", "native", "san_pcm.cpp"),
                                 os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "pcm ok" in out.stdout
