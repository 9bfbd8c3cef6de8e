"""ASan + UBSan over the bus dynamics' host side, which needs neither a handle nor HIP: s2r_dynamics_reference,
s2r_dynamics_curve and s2r_dynamics_coef (csrc/s2r_rules.cpp) beside tests/native/san_dyn.cpp, compiled by plain g++ and run as a
child process, with no preload of any kind — as tests/test_eq_native.py does.  (The dynamics' place in the post-mix chain's route is
checked with every other stage's by tests/native/post_route.cpp, tests/test_rules_native.py.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_dynamics_reference_under_asan_ubsan(tmp_path):
    """the reference at the edges of its shapes — no frames, one, two, five, a thousand; keyed by itself and by another buffer; null
    output and meter; in place; one call against two — on buffers of exactly the stated sizes, the answers that need no model (a
    constant curve is a gain, a key at a breakpoint reads its entry) and refusals that touch nothing; the curve and coefficient functions"""
    exe = str(tmp_path / "san_dyn")
    subprocess.check_call(SAN + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                                 os.path.join(ROOT, "tests", "native", "san_dyn.cpp"),
                                 os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "dyn ok" in out.stdout
