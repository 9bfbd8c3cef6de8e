"""ASan + UBSan over the bus drive's host side, which needs neither a handle nor HIP: s2r_drive_reference,
s2r_drive_taps and s2r_drive_curve (csrc/s2r_rules.cpp) beside tests/native/san_drive.cpp, compiled by plain g++ and run as a child
process, with no preload of any kind — as tests/test_room_native.py does.  (The drive's place in the post-mix chain's route is checked
with every other stage's by tests/native/post_route.cpp, tests/test_rules_native.py.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_drive_reference_under_asan_ubsan(tmp_path):
    """the reference at the edges of its shapes — no frames, one, 31, 32, 33, a thousand; every designed curve and a table of huge
    entries; pre 0 and 1024; a null output; in place; one call against two — on buffers of exactly the stated sizes, the answers that
    need no model (dry alone is the input 16 frames late, the history is the last 32 frames, the taps are symmetric) and refusals that
    touch nothing"""
    exe = str(tmp_path / "san_drive")
    subprocess.check_call(SAN + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                                 os.path.join(ROOT, "tests", "native", "san_drive.cpp"),
                                 os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "drive ok" in out.stdout
