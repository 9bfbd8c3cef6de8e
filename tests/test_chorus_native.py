"""ASan + UBSan over s2r_chorus_reference (csrc/s2r_rules.cpp: the bus chorus's rule on the host), which needs neither
a handle nor HIP: the file is compiled by plain g++ beside a small program of its own (tests/native/san_chorus.cpp) and run as a child
process, with no preload of any kind — as tests/test_delay_native.py does for the delay's reference."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_chorus_reference_under_asan_ubsan(tmp_path):
    """the reference at the edges of its shapes — H = 2 and 4096; no frames, one, H - 1, H and H + 1; a null output; the top of the
    triangle, where the oldest frame of the history is read — on buffers of exactly the stated sizes, and the answer that needs no
    model: with one voice, depth 0, a whole base B, dry 0 and wet 1 the output is the stream B frames late, as values"""
    exe = str(tmp_path / "san_chorus")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "san_chorus.cpp"),
                           os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "chorus ok" in out.stdout
