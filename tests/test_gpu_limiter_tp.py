"""The master limiter's true-peak detector on the device.  Twin handles are fed the same events, one with the limiter
and one without; the twin's sample_master output is x — the master after the fader — and the expectation is the numpy float32 model of
the rule (test_limiter_tp_host.np_limiter_tp) over x with xh and gh carried from call to call in numpy.  No oracle and no
s2r_limiter_tp_reference is in the loop.  The ceiling is taken from the twin: half the peak of its first call.

Handles, events and the one-pole bank are tests/test_gpu_reverb.py's: 272 voices in 64-voice workgroups, eight programs on eight
buses.  Every comparison is on bits with no NaN allowance (helpers.assert_bits_equal_finite).  The kernel runs one workgroup per 256
frames; the detector reaches 16 frames back and is centred 8 back, so the short calls are of 1, 7, 8, 9, 15, 16 and 17 frames."""
import ctypes as C
import json

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_gpu_buses import ubits
from test_gpu_reverb import SR, V, _bank, _events, _handles
from test_limiter_host import PAIRS, np_limiter
from test_limiter_tp_host import HIST, LAT, TRUTH, check_ranges_tp, np_limiter_tp

pytestmark = pytest.mark.gpu
F = np.float32
CALLS = [1000, 1, 16, 17, 300, 255, 256, 257]


class LimTp:
    """the limiter of a handle in numpy: ceiling, lookahead, hold, detector and the carried state"""

    def __init__(self, L, H, ceiling=None, true_peak=True):
        self.L, self.H, self.c, self.tp = L, H, ceiling, true_peak
        self.reset()
        self.sp, self.d, self.mag = [], [], []                   # the model's s', d and sample magnitude of every true-peak call so far

    def reset(self):
        self.xh, self.gh = np.zeros((self.L + (HIST if self.tp else 0), 2), dtype=F), np.ones(2 * self.L + self.H, dtype=F)

    def set(self, handles, ceiling=None, L=None, H=None, true_peak=None):
        """as s2r_set_master_limiter_ex: another lookahead, hold or detector resets the state, another ceiling keeps it"""
        ceiling = self.c if ceiling is None else ceiling
        L, H, tp = self.L if L is None else L, self.H if H is None else H, self.tp if true_peak is None else true_peak
        for syn in handles:
            syn.set_master_limiter(ceiling, L, H, true_peak=tp)
            assert syn.get_master_limiter() == (float(F(ceiling)), L, H) and syn.get_master_limiter_detector() == int(tp)
        if (L, H, tp) != (self.L, self.H, self.tp):
            self.L, self.H, self.tp = L, H, tp
            self.reset()
        self.c = ceiling

    def expect(self, x):
        if self.tp:
            y, sp, self.xh, self.gh, d, mag = np_limiter_tp(x, self.c, self.L, self.H, self.xh, self.gh, detail=True)
            self.d.append(d), self.mag.append(mag)
        else:
            y, sp, self.xh, self.gh = np_limiter(x, self.c, self.L, self.H, self.xh, self.gh)
        self.sp.append(sp)
        return y, sp

    def limited(self):
        return float((np.concatenate(self.sp) < 1.0).mean())

    def interpolated(self):
        """the share of frames whose d is not the sample magnitude, in bits"""
        return float((ubits(np.concatenate(self.d)) != ubits(np.concatenate(self.mag))).mean())


def _lfill(a, b, lim, n, nb, what, stems=True):
    """one call on both handles: the twin's sample_master gives x, its stems and its meters; the limited handle's master is the
    model over x, its stems and master meters are the twin's, and its limiter meters are min s' and max |y| of the model"""
    x, st_b = b.sample_master(n, SR, nb)
    assert np.isfinite(x).all()
    if lim.c is None:                                            # the first call: the ceiling from the twin
        lim.set((a,), float(np.abs(x).max()) / 2.0)
        assert lim.c > 2.0 ** -20
    want, sp = lim.expect(x)
    got, st = a.sample_master(n, SR, nb, stems=stems)
    assert_bits_equal_finite(got, want, what + ": master")
    assert np.abs(got).max() <= F(lim.c), what
    if stems:
        assert_bits_equal_finite(st, st_b, what + ": stems")
    else:
        assert st is None
    for g, w, name in zip(a.meters(), b.meters(), ("peaks", "energies")):
        assert_bits_equal_finite(g, w, what + ": master section " + name)
    assert_bits_equal_finite(np.array(a.limiter_meters(), dtype=F), np.array([sp.min(), np.abs(want).max()], dtype=F), what + ": limiter meters")
    return x, got


def _state_read_back(a, lim):
    xh, gh = a.limiter_state()
    assert xh.shape == lim.xh.shape and gh.shape == lim.gh.shape
    assert_bits_equal_finite(xh, lim.xh, "xh read back")
    assert_bits_equal_finite(gh, lim.gh, "gh read back")


@pytest.mark.parametrize("L,H", PAIRS)
def test_true_peak_limiter_is_the_rule_over_the_master(L, H):
    """the parity matrix: every (lookahead, hold) pair, calls of 1000, 1, 16, 17, 300, 255, 256 and 257 frames with events between
    them, 1, 3 or 8 buses by the pair's place in the list, every other call without stems, static returns and a master fader of 0.7.
    On the model, before anything is compared: at least a quarter of the case's frames are limited, and in at least a quarter the
    detector's magnitude differs in bits from the sample's."""
    a, b = _handles()
    nb = (1, 3, 8)[PAIRS.index((L, H)) % 3]
    for syn in (a, b):
        for bus in range(s2.MAX_BUSES):
            syn.set_bus_return(bus, 1.0 - bus / 16.0)
        syn.set_master_fader(0.7)
        syn.snap_master()
    lim = LimTp(L, H)
    # the model first, over the twin alone: the case must limit, and interpolate, before the device is asked anything
    xs = []
    for fill, n in enumerate(CALLS):
        _events((b,), V, fill)
        xs.append(b.sample_master(n, SR, nb)[0])
    probe = LimTp(L, H, float(np.abs(xs[0]).max()) / 2.0)
    for x in xs:
        probe.expect(x)
    print("L %d H %d, %d buses: %.3f of the model's frames are limited, %.3f have an interpolated magnitude" % (L, H, nb, probe.limited(), probe.interpolated()))
    assert probe.limited() >= 0.25, probe.limited()
    assert probe.interpolated() >= 0.25, probe.interpolated()
    # ... then both handles from the start, on a second twin
    b = _handles()[1]
    for bus in range(s2.MAX_BUSES):
        b.set_bus_return(bus, 1.0 - bus / 16.0)
    b.set_master_fader(0.7)
    b.snap_master()
    ys = []
    for fill, n in enumerate(CALLS):
        _events((a, b), V, fill)
        x, got = _lfill(a, b, lim, n, nb, "L %d H %d, %d buses, fill %d of %d frames" % (L, H, nb, fill, n), stems=fill % 2 == 0)
        assert_bits_equal_finite(x, xs[fill], "the second twin")
        ys.append(got)
    assert lim.limited() >= 0.25 and ubits(np.concatenate(ys)).any()
    _state_read_back(a, lim)


@pytest.mark.parametrize("L,H", [(48, 0), (257, 1)])
def test_every_workgroup_edge(L, H):
    """the kernel's workgroup covers 256 frames, the last one writes the next gains and all of them the next input frames: calls of
    255, 256, 257, 511, 512, 513 and 1024 frames.  At (48, 0) a workgroup's window begins inside the call from the second on (G = 96);
    at (257, 1) from the fourth (G = 515)."""
    a, b = _handles(64)
    lim = LimTp(L, H)
    for fill, n in enumerate([255, 256, 257, 511, 512, 513, 1024]):
        _events((a, b), 64, fill)
        _lfill(a, b, lim, n, 2, "workgroup edges, L %d H %d, fill %d of %d frames" % (L, H, fill, n), stems=False)
        _state_read_back(a, lim)
    print("workgroup edges, L %d H %d: %.3f of the model's frames are limited" % (L, H, lim.limited()))
    assert lim.limited() >= 0.25 and lim.interpolated() >= 0.25


@pytest.mark.parametrize("L,H", [(1, 0), (5, 3)])
def test_calls_around_the_latency_and_the_history(L, H):
    """runs of calls of 1, 7, 8, 9, 15, 16 and 17 frames, four times over: the detector's 16 frames and the output's L + 8 come from
    xh, from xh and the call, or from the call alone; the state is read back after every call"""
    a, b, probe = _handles(64, max_frames=64, n=3)
    _events((probe,), 64, 0)                                     # (the first frame of a stream is silent: the ceiling from a third handle's 64)
    lim = LimTp(L, H)
    lim.set((a,), float(np.abs(probe.sample_master(64, SR, 2)[0]).max()) / 2.0)
    assert lim.c > 2.0 ** -20
    fill = 0
    for _ in range(4):
        for n in [1, 7, 8, 9, 15, 16, 17]:
            _events((a, b), 64, fill)
            _lfill(a, b, lim, n, 2, "short calls, L %d H %d, fill %d of %d frames" % (L, H, fill, n), stems=fill % 2 == 0)
            _state_read_back(a, lim)
            fill += 1
    assert lim.limited() >= 0.25 and lim.interpolated() >= 0.25


@pytest.mark.parametrize("L,H", [(1, 0), (48, 7), (1024, 4096)])
def test_the_delay_on_the_device(L, H):
    """no model in the loop.  Under the largest ceiling the master is the twin's delayed by L + 8 frames in every bit, across calls,
    behind L + 8 frames of +0.0; min_gain is 1 and out_peak the peak of what came out; the stems are not delayed"""
    a, b = _handles()
    a.set_master_limiter(2.0 ** 20, L, H, true_peak=True)
    D = L + LAT
    xs, ys = [], []
    for fill, n in enumerate([300, 17, 1, 256, 1000]):
        _events((a, b), V, fill)
        x, st_b = b.sample_master(n, SR, 8)
        y, st = a.sample_master(n, SR, 8)
        xs.append(x), ys.append(y)
        assert_bits_equal_finite(st, st_b, "the stems are not delayed")
        assert a.limiter_meters() == (1.0, float(np.abs(y).max()))
    x, y = np.concatenate(xs), np.concatenate(ys)
    assert float(np.abs(x).max()) < 2.0 ** 18 and ubits(x).any()
    assert_bits_equal_finite(y[D:], x[:len(x) - D], "the delay")
    assert not ubits(y[:D]).any()


def test_checkpoint_in_the_middle_of_a_gain_reduction():
    """voices, pans, mix, sends and the limiter — parameters and detector through the getters, state through limiter_state, read while
    gh holds gains below 1 — into a fresh handle: the continuations are equal on bits, and equal to the model"""
    a, b = _handles(max_frames=512)
    lim = LimTp(240, 480)
    _events((a, b), V, 0)
    _lfill(a, b, lim, 400, 4, "before the checkpoint")
    _events((a, b), V, 1)
    _lfill(a, b, lim, 100, 4, "before the checkpoint, a call shorter than both histories")
    xh, gh = a.limiter_state()
    assert xh.shape == (240 + HIST, 2) and gh.min() < 1.0 and ubits(xh).any()
    params, det = a.get_master_limiter(), a.get_master_limiter_detector()
    assert det == s2.LIMITER_TRUE_PEAK
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    c = s2.Synth(V, max_frames=512, block_voices=64)
    c.set_patch_bank(_bank())
    c.import_state(state)
    c.set_voice_pans(pans)
    c.set_voice_mix(gains, buses)
    c.set_voice_sends(sends, sbuses)
    c.set_master_limiter(*params, true_peak=det == s2.LIMITER_TRUE_PEAK)
    c.set_limiter_state(xh, gh)
    for g, w in zip(c.limiter_state(), (xh, gh)):
        assert_bits_equal_finite(g, w, "the restored state read back")
    for k, n in enumerate([100, 400]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        _, got = _lfill(a, b, lim, n, 4, "the checkpointed handle, fill %d" % k)
        assert_bits_equal_finite(c.sample_master(n, SR, 4)[0], got, "the resumed handle, fill %d" % k)
        assert c.limiter_meters() == a.limiter_meters()


def test_switching_the_detector_on_one_handle():
    """in the middle of a gain reduction the ceiling moves: the next call is the model with the new ceiling over the SAME state.  Then
    the detector moves to the sample peak: the state resets, and the call equals test_limiter_host.np_limiter from the initial state;
    back to the true peak: the initial state again, asserted against the model over a state that was NOT reset too"""
    a, b = _handles()
    lim = LimTp(64, 100)
    _events((a, b), V, 0)
    _lfill(a, b, lim, 300, 4, "before the changes")
    assert lim.gh.min() < 1.0
    lim.set((a,), lim.c * 1.5)
    _events((a, b), V, 1)
    x, got = _lfill(a, b, lim, 300, 4, "after the ceiling moved")
    assert not np.array_equal(ubits(got), ubits(np_limiter_tp(x, lim.c, 64, 100)[0]))       # (a reset state would have shown)
    lim.set((a,), true_peak=False)
    assert lim.xh.shape == (64, 2) and not ubits(lim.xh).any() and (lim.gh == 1.0).all()
    _state_read_back(a, lim)
    _events((a, b), V, 2)
    x, got = _lfill(a, b, lim, 300, 4, "after the detector moved to the sample peak")
    assert_bits_equal_finite(got, np_limiter(x, lim.c, 64, 100)[0], "the sample-peak rule from the initial state")
    kept = lim.gh.copy()
    assert kept.min() < 1.0
    lim.set((a,), true_peak=True)
    assert lim.xh.shape == (64 + HIST, 2) and (lim.gh == 1.0).all()
    _state_read_back(a, lim)
    _events((a, b), V, 3)
    x, got = _lfill(a, b, lim, 300, 4, "after the detector moved back")
    assert not np.array_equal(ubits(got), ubits(np_limiter_tp(x, lim.c, 64, 100, np.zeros((64 + HIST, 2), F), kept)[0]))
    assert lim.limited() >= 0.25


def test_with_the_other_master_stages_on():
    """the loudness meter and the PCM stage behind the limiter, 24 bits without dither: master_lr is still the model; the meter's
    true peak of what the limiter wrote is at most C (1 + 2 e), e from the committed float64 measurement; and no sample of the
    master clips in the PCM stage.  The master fader brings the unlimited master's peak to 1.9 — from a third handle's first call —,
    so the ceiling, half of it, lies under full scale.  Asserted on the twin: without a limiter the meter reads more than the bound,
    and the PCM stage clips."""
    e = json.load(open(TRUTH))["e"]
    a, b, probe = _handles(n=3)
    _events((probe,), V, 0)
    peak = float(np.abs(probe.sample_master(1000, SR, 8)[0]).max())
    assert peak > 1.9
    for syn in (a, b):
        syn.set_master_fader(1.9 / peak)
        syn.snap_master()
        syn.set_master_loudness(SR)
        syn.set_master_pcm(24, "none")
    lim = LimTp(48, 0)
    for fill, n in enumerate([1000, 257, 16, 1000]):
        _events((a, b), V, fill)
        _lfill(a, b, lim, n, 8, "with loudness and PCM, fill %d of %d frames" % (fill, n))
        last, held = a.true_peak()
        print("fill %d: true peak %.6f C held %.6f C, bound %.6f C; the twin's %.6f C" % (fill, last.max() / lim.c, held.max() / lim.c, 1.0 + 2.0 * e, b.true_peak()[0].max() / lim.c))
        assert float(held.max()) <= lim.c * (1.0 + 2.0 * e), (fill, held, lim.c)
        clips_last, clips_held = a.pcm_clips()
        assert not clips_last[2 * s2.MAX_BUSES:].any() and not clips_held[2 * s2.MAX_BUSES:].any()
    assert 0.9 < lim.c < 1.0
    assert float(b.true_peak()[1].max()) > lim.c * (1.0 + 2.0 * e) and b.pcm_clips()[1][2 * s2.MAX_BUSES:].any()
    assert lim.limited() >= 0.25


def test_refusals_and_range_checks_on_a_handle():
    """size mismatches of the state pair in either mode, the detector's range and the resets (test_limiter_tp_host.check_ranges_tp);
    a refused fill leaves the state where it was; a device-list handle refuses the new entries"""
    check_ranges_tp(s2.Synth(8, max_frames=64))
    a, b = _handles(max_frames=256)
    lim = LimTp(64, 100)
    _events((a, b), V, 0)
    _lfill(a, b, lim, 100, 2, "before the refusals")
    L, h = a.L, a.h
    out, st = np.full(2 * 300, 7.0, dtype=F), np.full(2 * 2 * 300, 7.0, dtype=F)
    op, sp = out.ctypes.data_as(s2s._f32p), st.ctypes.data_as(s2s._f32p)
    assert L.s2r_fill_master(h, op, sp, st.size, 2, 257, SR) == s2s.S2R_ERR_TOO_MANY_FRAMES
    assert L.s2r_set_master_limiter_ex(h, lim.c, 64, 100, 2) == s2s.S2R_ERR_PATCH_RANGE
    buf = np.zeros(2 * (64 + HIST), dtype=F)
    gbuf = np.ones(228, dtype=F)
    for n_x, n_g in ((128, 228), (160, 227), (159, 228)):
        assert L.s2r_set_limiter_state(h, buf.ctypes.data_as(s2s._f32p), n_x, gbuf.ctypes.data_as(s2s._f32p), n_g) == s2s.S2R_ERR_INVALID
    assert (out == 7.0).all() and a.get_master_limiter_detector() == s2.LIMITER_TRUE_PEAK
    _state_read_back(a, lim)
    _events((a, b), V, 1)
    _lfill(a, b, lim, 64, 2, "after the refusals")
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    n = C.c_uint32()
    assert multi.L.s2r_set_master_limiter_ex(multi.h, 0.25, 48, 0, 1) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_master_limiter_detector(multi.h, C.byref(n)) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_master_limiter_ex(multi.h, 0.25, 48, 0, 2) == s2s.S2R_ERR_PATCH_RANGE     # the values are looked at first
