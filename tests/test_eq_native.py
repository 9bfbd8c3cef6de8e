"""ASan + UBSan over the bus EQ's host side, which needs neither a handle nor HIP: s2r_eq_reference and s2r_eq_design
(csrc/s2r_rules.cpp) beside tests/native/san_eq.cpp, compiled by plain g++ and run as a child process, with no preload of any kind —
as tests/test_chorus_native.py and tests/test_rules_native.py do.  (The EQ's place in the post-mix chain's route is checked with
every other stage's by tests/native/post_route.cpp, tests/test_rules_native.py.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_eq_reference_under_asan_ubsan(tmp_path):
    """the reference at the edges of its shapes — 1 to 4 bands; no frames, one, two, five, a thousand; a null output; one call against
    two — on buffers of exactly the stated sizes, the answers that need no model (a gain, two gains, a two-frame delay and the state it
    leaves), and refusals that touch nothing"""
    exe = str(tmp_path / "san_eq")
    subprocess.check_call(SAN + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                                 os.path.join(ROOT, "tests", "native", "san_eq.cpp"),
                                 os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "eq ok" in out.stdout
