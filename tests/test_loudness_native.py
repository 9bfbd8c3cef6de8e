"""ASan + UBSan over the loudness meters' host side, which needs neither a handle nor HIP: s2r_loudness_reference,
s2r_loudness_readings and s2r_loudness_design (csrc/s2r_rules.cpp) beside tests/native/san_loudness.cpp, compiled by plain g++ and run
as a child process, with no preload of any kind — as tests/test_flanger_native.py does."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_loudness_host_functions_under_asan_ubsan(tmp_path):
    """the three functions at the edges of their shapes — hops 16, 17, 48 and 4800; calls of 0, 1, 15, 16, 17 frames and of many hops,
    from the start of a hop and from its last frame; 0, 2 and 8 buses; fewer than 4 and fewer than 30 hop rows — on buffers of exactly
    the stated sizes, a stream in one call and in two, the answers that need no model, and refusals that touch nothing"""
    exe = str(tmp_path / "san_loudness")
    subprocess.check_call(SAN + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                                 os.path.join(ROOT, "tests", "native", "san_loudness.cpp"),
                                 os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "loudness ok" in out.stdout
