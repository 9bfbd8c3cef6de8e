"""True stereo on the device: s2r_fill_panned bit for bit against the oracle's rows, a Python model of the
note_on rule for the pans and s2o.mix_tree per channel — and, without any oracle, against the product's own mono mix.

Every mix is non-degenerate: seeds[v] = v, noise > 0, notes 36 + v % 61.  Every comparison is on bits with no NaN
allowance (helpers.assert_bits_equal_finite)."""
import os

import numpy as np
import pytest

from helpers import assert_bits_equal_finite, make_patch, oracle_cfg_from_patch
from oracle import s2o
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_pan_host import check_ranges, np_voice_pan

pytestmark = pytest.mark.gpu
SR = 48000
F = np.float32
ON, OFF, PROGRAM = 1, 0, 2


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def np_gains(p):
    """(gL, gR) of an array of pans: sqrtf((1 -/+ p) * 0.5f), every operation rounded to binary32"""
    p = np.asarray(p, dtype=F)
    return np.sqrt((F(1.0) - p) * F(0.5), dtype=F), np.sqrt((F(1.0) + p) * F(0.5), dtype=F)


def _onepole():
    return make_patch(noise=0.25)                               # the default patch (one-pole, saw) with audible noise


def _bank2():
    return [_onepole(), make_patch(osc_kind=s2.OSC_SINE, lpf_kind=s2.FILT_LP2, lpf_freq=900.0, noise=0.2)]


def _bank_mixed():
    """one-pole, LP2 and SVF with a DPW shape side by side: the general kernel (oscillator and filter per lane) feeds the rows"""
    return [_onepole(), make_patch(osc_kind=s2.OSC_SINE, lpf_kind=s2.FILT_LP2, lpf_freq=900.0, noise=0.2),
            make_patch(osc_kind=s2.OSC_DPW_SAW, lpf_kind=s2.FILT_SVF_LP, lpf_q=1.3, noise=0.1)]


class Twin:
    """An oracle synth over the whole pool, one or more GPU handles (each the pool or a shard of it) and the model of the
    voices' pans, driven in lockstep."""

    def __init__(self, voices, max_frames=1024, block=0, groups=0, patch=None, bank=None, shards=None):
        self.V = voices
        self.cpu = s2o.OracleSynth(voices)
        self.gpus = [s2.Synth(voices, max_frames=max_frames, block_voices=block, mix_groups=groups, **kw) for kw in (shards or [{}])]
        self.idx = []                                            # pool indices of every handle's voices, local order
        for kw in (shards or [{}]):
            if kw.get("shard_interleave"):
                self.idx.append(s2.shard_pool_indices(voices, kw["shard_index"], kw["shard_count"], kw["shard_interleave"]))
            else:
                b = kw.get("shard_begin", 0)
                self.idx.append(np.arange(b, b + (kw.get("shard_voices") or voices)))
        self.block, self.groups = self.gpus[0].block_voices, groups or 1
        if bank is not None:
            for g in self.gpus:
                g.set_patch_bank(bank)
            self.cpu.set_bank([oracle_cfg_from_patch(p) for p in bank])
        else:
            patch = patch if patch is not None else _onepole()
            for g in self.gpus:
                g.set_patch(patch)
            self.cpu.config = oracle_cfg_from_patch(patch)
        for v in range(voices):
            for g in self.gpus:
                g.set_noise_seed(v, v)
        self.program = 0
        self.prog = {}                                           # program -> (pan, key_spread)
        self.pans = np.zeros(voices, dtype=F)                    # the model: pool order

    # --- the note_on rule, restated ---
    def set_program_pan(self, program, pan, spread):
        self.prog[program] = (pan, spread)
        for g in self.gpus:
            g.set_program_pan(program, pan, spread)

    def program_change(self, program):
        self.program = program
        self.cpu.program_change(program)
        for g in self.gpus:
            g.program_change(program)

    def _cpu_on(self, note):
        v = self.cpu.next_voice_index()
        self.cpu.note_on(note, 1.0)
        self.cpu.set_seed(v, v)                                  # (the reference resets the seed; the handles keep theirs)
        pan, spread = self.prog.get(self.program, (0.0, 0.0))
        self.pans[v] = np_voice_pan(pan, spread, note)
        return v

    def note_on(self, note):
        v = self._cpu_on(note)
        for g in self.gpus:
            assert g.note_on(note, 1.0) == v
        return v

    def note_off(self, note):
        self.cpu.note_off(note)
        for g in self.gpus:
            g.note_off(note)

    def cpu_event(self, kind, note):
        if kind == ON:
            self._cpu_on(note)
        elif kind == OFF:
            self.cpu.note_off(note)
        else:
            self.program = note
            self.cpu.program_change(note)

    # --- expectations ---
    def rows(self, frames):
        with np.errstate(all="ignore"):
            return self.cpu.render_voices(frames, SR, threads=_threads())

    def want(self, pv, k=0):
        """[frames, 2]: handle k's panned mix of the oracle's rows under the model's pans"""
        idx = self.idx[k]
        gl, gr = np_gains(self.pans[idx])
        rows = pv[idx]
        left = s2o.mix_tree(rows * gl[:, None], self.block, self.groups)
        right = s2o.mix_tree(rows * gr[:, None], self.block, self.groups)
        return np.stack([left, right], axis=1)

    def check_fill(self, frames, what):
        pv = self.rows(frames)
        for k, g in enumerate(self.gpus):
            assert_bits_equal_finite(g.sample_panned(frames, SR), self.want(pv, k), "%s, handle %d, %d frames" % (what, k, frames))

    def check_pans(self, what):
        for k, g in enumerate(self.gpus):
            got = g.voice_pans()
            assert np.array_equal(got.view(np.uint32), self.pans[self.idx[k]].view(np.uint32)), what


def _drive(tw, lengths, what, programs=2):
    """note_ons under two pans (a program change — or, with one program, a change of its pan — between them), some notes
    off, restarts: one batch of events in front of every fill, the state carried from fill to fill"""
    V = tw.V
    if programs >= 2:
        tw.set_program_pan(0, -0.5, 1.0)
        tw.set_program_pan(1, 0.7, -1.0 / 3.0)
        if programs >= 3:
            tw.set_program_pan(2, 1.0, 1.0)                      # clamps above note 64
    else:
        tw.set_program_pan(0, -0.5, 1.0)
    for b, n in enumerate(lengths):
        if b == 0:
            for v in range(V):
                if v == V // 2:
                    if programs >= 2:
                        tw.program_change(1)
                    else:
                        tw.set_program_pan(0, 0.7, -1.0 / 3.0)   # later note_ons only
                tw.note_on(36 + v % 61)
        elif b == 1:
            for note in range(36, 97, 3):
                tw.note_off(note)
        else:
            if programs >= 2:
                tw.program_change((b + 1) % programs)
            else:
                tw.set_program_pan(0, [0.25, -1.0, 1.0][b % 3], [-1.0, 0.5, 1.0][b % 3])
            for k in range(min(V, 5 + 2 * b)):                   # restarts: the oldest voices, sounding or released
                tw.note_on(40 + (7 * k + b) % 50)
            tw.note_off(40 + b % 50)
        tw.check_fill(n, "%s, fill %d" % (what, b))
    tw.check_pans(what)
    assert len(np.unique(tw.pans)) > 4 or V <= 8


SHAPES = [(8, 0, 0), (17, 0, 0), (272, 64, 0), (1088, 64, 0), (1088, 64, 2), (1024, 256, 4)]


@pytest.mark.parametrize("programs", [1, 2])
@pytest.mark.parametrize("voices,block,groups", SHAPES)
def test_panned_fill_is_the_tree_over_the_scaled_rows(voices, block, groups, programs):
    """the parity matrix: every shape at 1, 16, 17 and 1000 frames (1000: a multiple of 4 — 16-byte loads; 1 and 17: the
    scalar loads), one shape also at max_frames.  programs = 1: a single patch, so the ONE-POLE kernel writes the rows, the
    program's pan changing between the note_ons; programs = 2: a bank of a one-pole and an LP2 patch with a pan each and
    program changes between the note_ons (the kernel with a patch per lane)."""
    tw = Twin(voices, max_frames=1024, block=block, groups=groups, bank=_bank2() if programs == 2 else None)
    lengths = [1000, 1, 16, 17] + ([1024] if (voices, groups) == (1088, 2) else [])
    _drive(tw, lengths, "%d voices, block %d, groups %d, %d programs" % (voices, block, groups, programs), programs)


def test_panned_fill_over_a_mixed_bank():
    """one-pole, LP2 and SVF under a DPW oscillator in one pool: the general kernel feeds the rows"""
    tw = Twin(272, max_frames=1024, block=64, bank=_bank_mixed())
    _drive(tw, [1000, 17, 256], "mixed bank", programs=3)


@pytest.mark.parametrize("voices,block", [(1088, 64), (4352, 256)])
def test_hard_left_is_the_mono_mix(voices, block):
    """every pan at -1: gL = 1, so L is what a twin handle's s2r_fill returns — the new kernels' tree held to the render
    kernel's own mixdown, no oracle in the loop — and R, sums of +-0 rooted at +0.0, is all +0.0"""
    a = s2.Synth(voices, max_frames=256, block_voices=block)
    b = s2.Synth(voices, max_frames=256, block_voices=block)
    for syn in (a, b):
        syn.set_patch(_onepole())
        for v in range(voices):
            syn.set_noise_seed(v, v)
        for v in range(voices):
            syn.note_on(36 + v % 61)
    a.set_voice_pans(np.full(voices, -1.0, dtype=F))
    for k, n in enumerate([256, 17, 250]):
        if k:
            for note in range(36 + k, 97, 4):
                a.note_off(note)
                b.note_off(note)
        got = a.sample_panned(n, SR)
        mono = b.sample(np.empty(n, dtype=F), SR)
        assert np.isfinite(mono).all() and np.abs(mono).max() > 0.0
        assert_bits_equal_finite(got[:, 0], mono, "hard left, %d voices, fill %d: L against s2r_fill" % (voices, k))
        assert not got[:, 1].view(np.uint32).any(), "hard left: R must be +0.0 everywhere"


def test_negated_pans_swap_the_channels():
    V = 272
    handles = []
    for sign in (1.0, -1.0):
        syn = s2.Synth(V, max_frames=512, block_voices=64)
        syn.set_patch_bank(_bank2())
        for v in range(V):
            syn.set_noise_seed(v, v)
        syn.set_program_pan(0, sign * -0.5, sign * 1.0)
        syn.set_program_pan(1, sign * 0.7, sign * (-1.0 / 3.0))
        for v in range(V):
            if v == 100:
                syn.program_change(1)
            syn.note_on(36 + v % 61)
        handles.append(syn)
    for k, n in enumerate([500, 17]):
        if k:
            for syn in handles:
                for note in range(36, 97, 5):
                    syn.note_off(note)
        x, y = handles[0].sample_panned(n, SR), handles[1].sample_panned(n, SR)
        assert np.isfinite(x).all() and not np.array_equal(x[:, 0], x[:, 1])
        assert_bits_equal_finite(y[:, 1], x[:, 0], "swap, fill %d: R of the negated handle against L" % k)
        assert_bits_equal_finite(y[:, 0], x[:, 1], "swap, fill %d: L of the negated handle against R" % k)
    assert np.array_equal(handles[1].voice_pans(), -handles[0].voice_pans())     # (as values: a pan of -0 is a pan of +0)


def test_default_pans_are_the_centre():
    """no pan ever set: L == R bit for bit, both the tree over rows * sqrtf(0.5)"""
    tw = Twin(272, max_frames=512, block=64)
    for v in range(272):
        tw.note_on(36 + v % 61)
    for n in (500, 17):
        pv = tw.rows(n)
        got = tw.gpus[0].sample_panned(n, SR)
        g = np.sqrt(F(0.5), dtype=F)
        want = s2o.mix_tree(pv * g, tw.block, 1)
        assert_bits_equal_finite(got[:, 0], want, "centre, L, %d frames" % n)
        assert_bits_equal_finite(got[:, 1], want, "centre, R, %d frames" % n)
    assert not tw.gpus[0].voice_pans().any()


@pytest.mark.parametrize("frames", [256, 250])
def test_events_inside_a_panned_fill(frames):
    """note_ons, note_offs, program changes and restarts of sounding voices at frames 0, 16, 48 and 240 of one fill: the
    expectation is built segment by segment from the oracle — events applied, render_voices(segment), the pan model
    updated per note_on, mix_tree per segment.  250 frames: the tail stays in the last segment."""
    V = 64
    tw = Twin(V, max_frames=256, block=64, bank=_bank2())
    tw.set_program_pan(0, -0.5, 1.0)
    tw.set_program_pan(1, 0.7, -1.0 / 3.0)
    for fill in range(2):                                        # the second fill starts from the state the first left
        ev = []
        if fill == 0:
            ev += [(ON, 36 + v % 61, 0) for v in range(V // 2)] + [(PROGRAM, 1, 0)] + [(ON, 36 + v % 61, 0) for v in range(V // 2, V - 4)]
        else:
            ev += [(OFF, 40, 0), (ON, 90, 0)]
        ev += [(ON, 50, 16), (OFF, 36, 16), (PROGRAM, 0, 16), (ON, 50, 16), (ON, 77, 16)]              # 50 twice: a sounding note again
        ev += [(OFF, 50, 48), (PROGRAM, 1, 48)] + [(ON, 60 + k, 48) for k in range(8)] + [(OFF, 61, 48)]  # past the pool: restarts
        ev += [(ON, 50, 240), (PROGRAM, 0, 240), (ON, 99, 240), (OFF, 77, 240)]
        arr = np.array([(k, n, f, 1.0) for k, n, f in ev], dtype=s2.NOTE_EVENT_DTYPE)
        tw.gpus[0].note_events(arr)
        got = tw.gpus[0].sample_panned(frames, SR)
        want = np.zeros((frames, 2), dtype=F)
        bounds = [0, 16, 48, 240, frames]
        for a, b in zip(bounds[:-1], bounds[1:]):
            for k, n, f in ev:
                if f == a:
                    tw.cpu_event(k, n)
            want[a:b] = tw.want(tw.rows(b - a))
        assert_bits_equal_finite(got, want, "timed events, %d frames, fill %d" % (frames, fill))
        tw.check_pans("timed events")
    # a mono fill consumes timed note_ons just as well: their pans are the voices' afterwards
    arr = np.array([(ON, 44, 0, 1.0), (PROGRAM, 1, 16, 0.0), (ON, 45, 16, 1.0)], dtype=s2.NOTE_EVENT_DTYPE)
    tw.gpus[0].note_events(arr)
    mono = tw.gpus[0].sample(np.empty(64, dtype=F), SR)
    tw.cpu_event(ON, 44)
    pv0 = tw.rows(16)
    tw.cpu_event(PROGRAM, 1)
    tw.cpu_event(ON, 45)
    pv1 = tw.rows(48)
    assert_bits_equal_finite(mono, np.concatenate([s2o.mix_tree(pv0, 64, 1), s2o.mix_tree(pv1, 64, 1)]), "mono fill with timed events")
    tw.check_pans("after a mono fill with timed events")
    tw.check_fill(32, "after a mono fill with timed events")


@pytest.mark.parametrize("interleave", [0, 16])
def test_shards_pan_their_own_voices(interleave):
    V = 512
    if interleave:
        shards = [dict(shard_interleave=16, shard_index=r, shard_count=2) for r in range(2)]
    else:
        shards = [dict(shard_begin=256 * r, shard_voices=256) for r in range(2)]
    tw = Twin(V, max_frames=512, block=64, shards=shards)
    assert [g.shard_voices for g in tw.gpus] == [256, 256]
    _drive(tw, [496, 17], "shards, interleave %d" % interleave, programs=1)
    if interleave:
        assert tw.idx[1][0] == 16 and tw.idx[0][16] == 32       # local order is not pool order


def test_panned_fills_coexist_with_the_other_fills():
    """s2r_fill, s2r_fill_panned and s2r_fill_stereo interleaved on one handle with the pool-resident kernel switched on:
    every buffer and the final state match the oracle; a device-list handle refuses the panned fill and stays usable"""
    V = 1024
    tw = Twin(V, max_frames=256, block=256)
    gpu = tw.gpus[0]
    gpu.set_resident(True)
    tw.set_program_pan(0, 0.3, -1.0)
    for v in range(V):
        tw.note_on(36 + v % 61)
    for k, kind in enumerate(["mono", "panned", "stereo", "panned", "mono", "mono", "panned"]):
        n = [256, 256, 128, 17, 256, 16, 200][k]
        if k in (2, 4):
            for note in range(36 + k, 97, 6):
                tw.note_off(note)
        if k in (3, 6):
            for j in range(20):
                tw.note_on(45 + (j * 3 + k) % 40)
        pv = tw.rows(n)
        mono = s2o.mix_tree(pv, tw.block, 1)
        what = "coexistence, fill %d (%s)" % (k, kind)
        if kind == "mono":
            assert_bits_equal_finite(gpu.sample(np.empty(n, dtype=F), SR), mono, what)
        elif kind == "stereo":
            assert_bits_equal_finite(gpu.sample_stereo(n, SR), np.stack([mono, mono], axis=1), what)
        else:
            assert_bits_equal_finite(gpu.sample_panned(n, SR), tw.want(pv), what)
    st = gpu.export_state()
    for v in range(V):
        cv = tw.cpu.voice(v)
        assert bool(st["started"][v]) == bool(cv.has_current) and bool(st["released"][v]) == bool(cv.has_release)
        assert st["note"][v] == cv.note
        if cv.has_current:
            assert st["current_frame_offset"][v] == cv.current_frame_offset
            assert st["phase_accum"][v].view(np.uint32) == F(cv.state.phase_accum).view(np.uint32)
            assert st["lpf_last"][v].view(np.uint32) == F(cv.state.lpf_last).view(np.uint32)
        if cv.has_release:
            assert st["release_frame_offset"][v] == cv.release_frame_offset
    tw.check_pans("coexistence")
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    one = s2.Synth(512, max_frames=64, mix_groups=2)
    for syn in (multi, one):
        for v in range(512):
            syn.note_on(36 + v % 61)
    with pytest.raises(s2.S2rError) as err:
        multi.sample_panned(64, SR)
    assert err.value.status == s2s.S2R_ERR_INVALID
    x, y = multi.sample(np.empty(64, dtype=F), SR), one.sample(np.empty(64, dtype=F), SR)
    assert np.abs(y).max() > 0.0
    assert_bits_equal_finite(x, y, "the device-list handle after the refused panned fill")


def test_checkpoint_carries_the_pans():
    V = 272
    tw = Twin(V, max_frames=256, block=64, bank=_bank2())
    _drive(tw, [200, 17], "checkpoint, before", programs=2)
    a = tw.gpus[0]
    state, pans = a.export_state(), a.voice_pans()
    b = s2.Synth(V, max_frames=256, block_voices=64)
    b.set_patch_bank(_bank2())
    b.import_state(state)
    b.set_voice_pans(pans)
    assert np.array_equal(b.voice_pans().view(np.uint32), pans.view(np.uint32))
    for k, n in enumerate([256, 17]):
        for syn in (a, b):
            syn.note_off(40 + k)
        x, y = a.sample_panned(n, SR), b.sample_panned(n, SR)
        assert np.abs(x).max() > 0.0
        assert_bits_equal_finite(y, x, "resumed handle, fill %d" % k)


def test_range_checks_on_a_handle():
    check_ranges(s2.Synth(8, max_frames=64))
