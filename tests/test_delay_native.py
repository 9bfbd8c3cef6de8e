"""ASan + UBSan over s2r_delay_reference (csrc/s2r_rules.cpp: the bus delay's rule on the host), which needs neither a
handle nor HIP: the file is compiled by plain g++ beside a small program of its own (tests/native/san_delay.cpp) and run as a child
process, with no preload of any kind — as tests/test_rules_native.py does for the other references."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_delay_reference_under_asan_ubsan(tmp_path):
    """the reference at the edges of its shapes — D = 1 and S2R_MAX_DELAY_FRAMES; no frames, one, D - 1, D, D + 1 and a count that is
    no multiple of D; a null output — on buffers of exactly the stated sizes, and the answers that need no model: with feedback 0,
    cross 0, dry 0 and wet 1 the output is the stream D frames late and the history its last D frames"""
    exe = str(tmp_path / "san_delay")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "san_delay.cpp"),
                           os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "delay ok" in out.stdout
