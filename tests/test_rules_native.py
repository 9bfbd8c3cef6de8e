"""ASan + UBSan over the handle-free rule functions (csrc/s2r_rules.cpp: the reverb, master and limiter references and the mixer's
gain rules), which need neither a handle nor HIP: the file is compiled by plain g++ beside a small program of its own
(tests/native/san_rules.cpp) and run as a child process, with no preload of any kind.  The post-mix chain's route (csrc/s2r_post_route.h)
goes the same way with tests/native/post_route.cpp, what its master stages keep on the host (csrc/s2r_post_keep.h) with
tests/native/post_keep.cpp, and the voice mixer's bookkeeping (csrc/s2r_mixer_keep.h) with tests/native/mixer_keep.cpp."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_rule_functions_under_asan_ubsan(tmp_path):
    """the three references at their edges — frames 0 and 1; K = 1, S2R_IR_SEGMENT and S2R_IR_SEGMENT + 1; 1 and S2R_MAX_BUSES buses;
    lookahead 1 and the maximum, hold 0 and the maximum; null optional outputs — on buffers of exactly the stated sizes, and the
    answers that need no model: a one-tap response of 1.0 with dry 0 and wet 1 returns its input, a limiter input under the ceiling
    comes out L frames late and otherwise unchanged, returns and fader at 1 make the master the in-order sum"""
    exe = str(tmp_path / "san_rules")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "san_rules.cpp"),
                           os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "rules ok" in out.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_post_route_under_asan_ubsan(tmp_path):
    """who reads and writes what behind the bus mixdown (s2r_post_route, csrc/s2r_post_route.h, a header without HIP): a panned call,
    bus fills x the 256 subsets of running bus stages, master fills x 256 subsets x the 64 subsets of {multiband, limiter, loudness,
    spectrum, resampler, PCM} set (and the PCM stage idle behind a resampler that makes no frame) x stems wanted or not, each route
    against the 24 routes of the bus stages and the 12 of the master stages written out by hand (the tables of
    tests/native/post_route.cpp) where they name the call, against the rule walked in launch order without them — every buffer is
    written once before it is read, the combine writes first, the last writer hits the call's destination, no kernel reads a pinned
    output, exactly one stage writes the pinned master in a master fill, every reader reads what the last writer wrote, a stage that
    does not run has null pointers — and against the route of the same call with one more stage on: a bus stage or a master writer
    takes over exactly one pointer, a master reader moves at most the copy-out pointer and, if it is the only one, the last writer's
    destination"""
    exe = str(tmp_path / "post_route")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "synth2_amd", "csrc"), os.path.join(ROOT, "tests", "native", "post_route.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "route ok" in out.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_post_keep_under_asan_ubsan(tmp_path):
    """what the stages behind the master fader keep on the host (csrc/s2r_post_keep.h, a header without HIP): the row store against a
    std::deque of the last max_rows rows — count and every float after each step — at row widths 1, 18 and S2R_SPECTRUM_ROW(256),
    max_rows 1, 2 and 5, appends of 0 .. 3 max_rows + 1 rows, runs of single rows across more than one compaction, assign and clear
    followed by appends; the position step against quotient and remainder in 64 bits, past 2^32; and each transition of a mirrored
    state's host side — set, zero, committed, off, set after committed — on its own"""
    exe = str(tmp_path / "post_keep")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "post_keep.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "keep ok" in out.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_mixer_keep_under_asan_ubsan(tmp_path):
    """the voice mixer's bookkeeping (S2rMixerKeep, csrc/s2r_mixer_keep.h, a header without HIP) against a naive model — per-voice
    arrays updated in place, gains recomputed voice by voice with the rule_* functions — over 320 seeded walks of 48 steps: program
    pan / mix / send / fader sets, the first use of each attribute in every order, note_ons at frame 0 and inside a fill, fills
    that settle late, panned and bus fills split at their event frames, snap, bank shrink and regrow with voices on a program that
    fell off, checkpoint programs with the queue filtered.  After a step both staging buffers are filled, in allocations of exactly
    2 * padded_voices floats and padded_voices * kBusGainBytes bytes, and compared in BITS: every byte the layout defines, zeros past
    the shard, the per-voice getters, and the dirty bits against the model's.  Shard voices 1, 63, 64 and 65; sends never used and
    used; ramps over 1 and 48 frames; one program and eight"""
    exe = str(tmp_path / "mixer_keep")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "synth2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "mixer_keep.cpp"),
                           os.path.join(ROOT, "synth2_amd", "csrc", "s2r_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "mixer ok" in out.stdout
