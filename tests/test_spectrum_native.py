"""ASan + UBSan over the spectrum meter's host side, which needs neither a handle nor HIP: s2r_spectrum_reference,
s2r_spectrum_readings, s2r_spectrum_band_readings, s2r_spectrum_window and s2r_spectrum_twiddles (csrc/s2r_rules.cpp) beside
tests/native/san_spectrum.cpp, compiled by plain g++ and run as a child process, with no preload of any kind — as
tests/test_loudness_native.py does."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_spectrum_host_functions_under_asan_ubsan(tmp_path):
    """the five functions at the edges of their shapes — sizes 256, 512 and 8192; hops of N / 8, N and N + 5; calls of 0, 1, hop - 1,
    hop and 2 hop + 3 frames, from the start of a hop and from its last frame; 0, 2 and 8 buses — on buffers of exactly the stated
    sizes, a stream in one call and in two, the answers that need no model, and refusals that touch nothing"""
    exe = str(tmp_path / "san_spectrum")
    subprocess.check_call(SAN + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                                 os.path.join(ROOT, "tests", "native", "san_spectrum.cpp"),
                                 os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "spectrum ok" in out.stdout
