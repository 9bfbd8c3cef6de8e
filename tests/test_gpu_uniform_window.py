"""The uniform window of the one-pole render kernel: a wavefront whose 64 voices were started together reads
its chunks' filter coefficients, 1 - x, amplitudes and noise from a window in LDS that it fills once per run.  Every case here
compares bit for bit against the CPU oracle (per-voice rows where the fill has no timed events, and the mix), and against the
same fills with the window switched off (s2r_set_uniform_window), and states what the handle's counter of window chunks
(s2r_uniform_window_chunks) must say: that the path was taken, or was not.

256 voices — one workgroup, the cohort in its first wavefront — unless a case says otherwise."""
import numpy as np
import pytest

from helpers import assert_bits_equal, make_patch, oracle_cfg_from_patch
from oracle import s2o
import synth2_amd as s2

pytestmark = pytest.mark.gpu

SR = 48000
NOTES = [30 + k for k in range(64)]          # 64 different notes: every lane its own pitch, every note-off its own voice

# amp: attack to frame 960, decay to 2400, then sustain; mod: attack to 480, decay to 3360 (48 kHz).  Both envelopes move
# — and the amplitude is per frame — up to frame 2400; from there the amplitude is flat and the wave takes the flat-amplitude variant.
ENV = {"amp_env.attack_ms": 20.0, "amp_env.decay_ms": 30.0, "amp_env.sustain": 0.5, "amp_env.release_ms": 25.0,
       "mod_env.attack_ms": 10.0, "mod_env.decay_ms": 60.0, "mod_env.sustain": 0.2, "mod_env.release_ms": 50.0}


def _events(items):
    ev = np.zeros(len(items), dtype=s2.NOTE_EVENT_DTYPE)
    for i, (kind, note, frame) in enumerate(items):
        ev[i] = (kind, note, frame, 1.0)
    return ev


def _oracle(voices, patch, fills, events, sr, seeds):
    """the oracle's per-voice rows of every fill, driven 16 frames at a time with the fill's events applied in between
    (main.rs:138-143), computed once per case"""
    cpu = s2o.OracleSynth(voices)
    cpu.config = oracle_cfg_from_patch(patch)

    def apply(kind, note):
        if kind:
            v = cpu.next_voice_index()
            cpu.note_on(note)
            if seeds is not None:                                # (the reference resets the seed on a note-on; the variant keeps it)
                cpu.set_seed(v, int(seeds[v]))
        else:
            cpu.note_off(note)

    rows = []
    for b, frames in enumerate(fills):
        ev = events.get(b, [])
        pv = np.zeros((voices, frames), dtype=np.float32)
        if not any(f for _k, _n, f in ev):
            for kind, note, _f in ev:
                apply(kind, note)
            pv[:, :] = cpu.render_voices(frames, sr)
        else:
            k = 0
            for c in range(0, frames, 16):
                while k < len(ev) and ev[k][2] == c:
                    apply(ev[k][0], ev[k][1])
                    k += 1
                n = min(16, frames - c)
                pv[:, c:c + n] = cpu.render_voices(n, sr)
            assert k == len(ev)
        rows.append(pv)
    return rows


def _gpu(voices, patch, fills, events, sr, window, rows, seeds=None, flat=True, max_frames=1024):
    """one GPU handle through the case: its outputs per fill (per-voice rows, or the mix) and the counter after every fill"""
    g = s2.Synth(voices, max_frames=max_frames)
    try:
        if not flat:
            g.set_flat_shortcut(False)
        g.set_patch(patch)
        if seeds is not None:
            for v, sd in enumerate(seeds):
                if sd:
                    g.set_noise_seed(v, int(sd))
        if not window:
            g.set_uniform_window(False)
        outs, counts = [], []
        for b, frames in enumerate(fills):
            if events.get(b):
                g.note_events(_events(events[b]))
            outs.append(g.render_voices(frames, sr) if rows else g.sample(np.empty(frames, dtype=np.float32), sr).copy())
            counts.append(g.uniform_window_chunks())
        return outs, counts, g.block_voices
    finally:
        g.close()


def _case(patch, fills, events, voices=256, sr=SR, seeds=None, flat=True, max_frames=1024):
    """Runs the case on the oracle once and on the GPU with the window on (rows where the case has no timed events, and the
    mix) and off (the mix); asserts the bits; returns the window-on mix run's counter after every fill."""
    want = _oracle(voices, patch, fills, events, sr, seeds)
    timed = any(f for evs in events.values() for _k, _n, f in evs)
    mix_on, counts, bv = _gpu(voices, patch, fills, events, sr, True, False, seeds, flat, max_frames)
    mix_off, counts_off, _ = _gpu(voices, patch, fills, events, sr, False, False, seeds, flat, max_frames)
    assert counts_off == [0] * len(fills), counts_off
    for b in range(len(fills)):
        assert_bits_equal(mix_on[b], s2o.mix_tree(want[b], bv, 1), "mix against the oracle, fill %d" % b)
        assert_bits_equal(mix_on[b], mix_off[b], "window on against off, fill %d" % b)
    if not timed:
        rows_on, counts_rows, _ = _gpu(voices, patch, fills, events, sr, True, True, seeds, flat, max_frames)
        for b in range(len(fills)):
            assert_bits_equal(rows_on[b], want[b], "per-voice rows against the oracle, fill %d" % b)
        assert counts_rows == counts, (counts_rows, counts)
    return counts


def _cohort(n=64):
    return [(1, NOTES[k], 0) for k in range(n)]


# ---- the path is taken ----

@pytest.mark.parametrize("osc", [s2.OSC_SQUARE, s2.OSC_SAW, s2.OSC_TRIANGLE, s2.OSC_SINE])
def test_cohort_through_attack_decay_and_sustain(osc):
    """a 64-voice cohort on different notes through attack, the attack -> decay turn inside a buffer (frame 960), decay, and
    decay -> sustain (frame 2400): every chunk up to frame 2400 goes through the window — the runs between the envelopes'
    turns at 480, 960 and 2400 all have three chunks or more — and none from there on, where the amplitude is flat"""
    counts = _case(make_patch(osc_kind=osc, **ENV), [1024, 1024, 1024, 1024], {0: _cohort()})
    assert counts == [64, 128, 150, 150], counts


@pytest.mark.parametrize("frames", [1000, 48])
def test_cohort_with_ragged_and_short_fills(frames):
    """Fills of 48 frames: three chunks, the shortest run that takes the window.  Fills of 1000: 62 chunks and a scalar tail of
    8 frames.  The first fill's runs are 30 chunks to frame 480, 30 to 960 and two to 992, which is too short; the second
    starts at offset 1000, no multiple of 16, and is not aligned at all; the third starts at 2000 = 16 * 125 and takes the
    window up to the amplitude's sustain at 2400: 25 chunks."""
    counts = _case(make_patch(**ENV), [frames, frames, frames], {0: _cohort()})
    assert counts == ([3, 6, 9] if frames == 48 else [60, 60, 85]), counts


def test_timed_note_offs_on_a_few_lanes():
    """note-offs at frames 512 and 528 of the first fill on three lanes: booked ahead, they change nothing before the voices'
    amplitude decay ends (the release offset is clamped to attack + decay, simdtest.rs:283) — the wave stays on the window up
    to there — and from frame 2400 on those three lanes release while the others sustain"""
    ev = {0: _cohort() + [(0, NOTES[3], 512), (0, NOTES[40], 512), (0, NOTES[17], 528)]}
    counts = _case(make_patch(**ENV), [1024, 1024, 1024, 1024], ev)
    assert counts[0] > 0 and counts[1] > counts[0], counts


def test_restart_of_one_lane_mid_fill():
    """64 voices in a pool of 64: a note-on at frame 640 of the first fill takes the oldest voice, lane 0.  The wave leaves the
    window at that boundary — 40 chunks — and never comes back: lane 0's offset differs from then on."""
    ev = {0: _cohort() + [(1, 99, 640)]}
    counts = _case(make_patch(**ENV), [1024, 1024], ev, voices=64)
    assert counts == [40, 40], counts


# ---- the path is refused ----

def test_refused_one_lane_started_a_buffer_later():
    counts = _case(make_patch(**ENV), [1024, 1024], {0: _cohort(63), 1: [(1, NOTES[63], 0)]})
    assert counts == [0, 0], counts


def test_refused_one_lane_never_started():
    counts = _case(make_patch(**ENV), [1024, 1024], {0: _cohort(63)})
    assert counts == [0, 0], counts


def test_refused_one_lane_with_another_seed():
    """(a seed whose rotation keeps a zero low nibble: the wave stays on the aligned variant, and only the window's own
    comparison of the seeds turns it away)"""
    seeds = np.zeros(256, dtype=np.uint32)
    seeds[5] = 1024
    counts = _case(make_patch(**ENV), [1024, 1024], {0: _cohort()}, seeds=seeds)
    assert counts == [0, 0], counts


def test_refused_without_tables():
    counts = _case(make_patch(**ENV), [1024], {0: _cohort()}, flat=False)
    assert counts == [0], counts


def test_refused_fm_patch():
    counts = _case(make_patch(mod_env_to_osc_freq=2.0, **ENV), [1024], {0: _cohort()})
    assert counts == [0], counts


def test_refused_svf_patch():
    counts = _case(make_patch(lpf_kind=s2.FILT_SVF_LP, **ENV), [1024], {0: _cohort()})
    assert counts == [0], counts


def test_refused_16_frame_fills():
    """one chunk per fill, two per fill: below the run threshold of three"""
    counts = _case(make_patch(**ENV), [16, 16, 32, 16], {0: _cohort()})
    assert counts == [0, 0, 0, 0], counts


# ---- no window ----

def test_no_window_beyond_1024_frames():
    """a handle with max_frames 2048 filling 2048 frames: 256-frame super-chunks in two buffers, no room for a window"""
    counts = _case(make_patch(**ENV), [2048], {0: _cohort()}, max_frames=2048)
    assert counts == [0], counts


def test_no_window_with_two_workgroups_per_compute_unit():
    """a pool of twice the device's compute units of 256-voice workgroups at 256 frames: the 256-frame super-chunk form"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    voices = 2 * n_cu * 256
    patch = make_patch(**ENV)
    outs = {}
    for window in (True, False):
        g = s2.Synth(voices, max_frames=256)
        g.set_patch(patch)
        g.set_uniform_window(window)
        g.note_events(_events(_cohort()))
        outs[window] = g.sample(np.empty(256, dtype=np.float32), SR).copy()
        assert g.uniform_window_chunks() == 0
    # the oracle on the cohort's own workgroup: the other workgroups' rows are +0.0 and the tree adds them to a sum that
    # is not -0.0 (checked), which changes no bit
    want = s2o.mix_tree(_oracle(256, patch, [256], {0: _cohort()}, SR, None)[0], 256, 1)
    assert not np.any((want == 0.0) & np.signbit(want))
    assert_bits_equal(outs[True], want, "mix against the oracle")
    assert_bits_equal(outs[True], outs[False], "window on against off")


# ---- envelope times that are, and are not, whole frames ----

@pytest.mark.parametrize("whole", [True, False])
def test_envelope_times_whole_and_fractional_frames(whole):
    """44 100 Hz.  Whole: 10 ms = 441 frames, 20 ms = 882.  Fractional: 10.3 ms = 454.23 frames, 21.7 ms = 956.97 — the decay's
    base and the stages' ends are no integers, so its turns fall inside chunks, which the general path renders"""
    env = dict(ENV)
    if whole:
        env.update({"amp_env.attack_ms": 10.0, "amp_env.decay_ms": 20.0, "mod_env.attack_ms": 10.0, "mod_env.decay_ms": 40.0})
    else:
        env.update({"amp_env.attack_ms": 10.3, "amp_env.decay_ms": 21.7, "mod_env.attack_ms": 3.3, "mod_env.decay_ms": 47.9})
    counts = _case(make_patch(**env), [1024, 1024], {0: _cohort()}, sr=44100)
    assert counts[0] > 0, counts
