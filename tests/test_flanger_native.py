"""ASan + UBSan over the bus flanger's host side, which needs neither a handle nor HIP: s2r_flanger_reference and
s2r_flanger_history_frames (csrc/s2r_rules.cpp) beside tests/native/san_flanger.cpp, and the flanger's insert into the post-mix chain's
route (s2r_post_route_flanger, csrc/s2r_post_route.h) with tests/native/post_route_flanger.cpp.  Each is compiled by plain g++ and run
as a child process, with no preload of any kind — as tests/test_drive_native.py does."""
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


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_post_route_with_the_flanger_under_asan_ubsan(tmp_path):
    """the 24 routes x EQ, dynamics, room, drive and flanger off / on, in bus and master fills: every buffer is written before it is
    read, the combine writes first, the last writer hits the call's destination, no kernel reads a pinned output, and a call without a
    flanger is pointer for pointer the drive's route"""
    exe = str(tmp_path / "post_route_flanger")
    subprocess.check_call(SAN + ["-I", os.path.join(ROOT, "synth2_amd", "csrc"), os.path.join(ROOT, "tests", "native", "post_route_flanger.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "route flanger ok" in out.stdout
