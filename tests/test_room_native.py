"""ASan + UBSan over the bus room's host side, which needs neither a handle nor HIP: s2r_room_reference,
s2r_room_state_floats and s2r_room_design (csrc/s2r_rules.cpp) beside tests/native/san_room.cpp, compiled by plain g++ and run as a
child process, with no preload of any kind — as tests/test_dyn_native.py does.  (The room's place in the post-mix chain's route is
checked with every other stage's by tests/native/post_route.cpp, tests/test_rules_native.py.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_room_reference_under_asan_ubsan(tmp_path):
    """the reference at the edges of its shapes — no frames, one, two, five, a thousand; every line at 64 frames, at 8192, and the
    spread at its end; a null output; in place; one call against two — on buffers of exactly the stated sizes, the answers that need
    no model (the first 64 frames are dry, gain 0 passes the input) and refusals that touch nothing; the count and the design"""
    exe = str(tmp_path / "san_room")
    subprocess.check_call(SAN + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                                 os.path.join(ROOT, "tests", "native", "san_room.cpp"),
                                 os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "room ok" in out.stdout
