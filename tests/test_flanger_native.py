"""ASan + UBSan over the bus flanger's host side, which needs neither a handle nor HIP: s2r_flanger_reference and
s2r_flanger_history_frames (csrc/s2r_rules.cpp) beside tests/native/san_flanger.cpp, compiled by plain g++ and run as a child process,
with no preload of any kind — as tests/test_drive_native.py does.  (The flanger's place in the post-mix chain's route is checked with
every other stage's by tests/native/post_route.cpp, tests/test_rules_native.py.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_flanger_reference_under_asan_ubsan(tmp_path):
    """the reference at the edges of its shapes — H = 33 and 4096; no frames, one, 31, 32, 33, H - 1, H, H + 1; a null output — on
    buffers of exactly the stated sizes, the answers that need no model (depth 0 at a whole base is the line that many frames late,
    and with feedback 1 the plain comb) and refusals that touch nothing"""
    exe = str(tmp_path / "san_flanger")
    subprocess.check_call(SAN + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                                 os.path.join(ROOT, "tests", "native", "san_flanger.cpp"),
                                 os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "flanger ok" in out.stdout
