"""The master limiter on the device.  Twin handles are fed the same events, one with a limiter and one without; the
twin's sample_master output is x — the master after the fader — and the expectation is the numpy float32 model of the rule
(test_limiter_host.np_limiter) over x with xh and gh carried from call to call in numpy.  No oracle and no s2r_limiter_reference
is in the loop.  The ceiling is taken from the twin: half the peak of its first call.

Handles, events and the one-pole bank are tests/test_gpu_reverb.py's: 272 voices in 64-voice workgroups, eight programs on eight
buses.  Every comparison is on bits with no NaN allowance (helpers.assert_bits_equal_finite).  The kernel runs one workgroup per 256
frames, so the block edges are calls of a multiple of 256 frames, plus and minus one."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_gpu_buses import ubits
from test_gpu_panned import ON
from test_gpu_reverb import SR, V, _bank, _events, _handles, _ir
from test_limiter_host import PAIRS, check_ranges, np_limiter

pytestmark = pytest.mark.gpu
F = np.float32
CALLS = [1000, 1, 16, 17, 300, 255, 256, 257]


class Lim:
    """the limiter of a handle in numpy: ceiling, lookahead, hold and the carried state"""

    def __init__(self, L, H, ceiling=None):
        self.L, self.H, self.c = L, H, ceiling
        self.reset()
        self.sp = []                                             # the model's s' of every call so far

    def reset(self):
        self.xh, self.gh = np.zeros((self.L, 2), dtype=F), np.ones(2 * self.L + self.H, dtype=F)

    def set(self, handles, ceiling=None, L=None, H=None):
        """as s2r_set_master_limiter: another lookahead or hold resets the state, another ceiling keeps it"""
        ceiling = self.c if ceiling is None else ceiling
        L, H = self.L if L is None else L, self.H if H is None else H
        for syn in handles:
            syn.set_master_limiter(ceiling, L, H)
            assert syn.get_master_limiter() == (float(F(ceiling)), L, H)
        if (L, H) != (self.L, self.H):
            self.L, self.H = L, H
            self.reset()
        self.c = ceiling

    def expect(self, x):
        y, sp, self.xh, self.gh = np_limiter(x, self.c, self.L, self.H, self.xh, self.gh)
        self.sp.append(sp)
        return y, sp

    def limited(self):
        return float((np.concatenate(self.sp) < 1.0).mean())


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


@pytest.mark.parametrize("L,H", PAIRS)
def test_limiter_is_the_rule_over_the_master(L, H):
    """the parity matrix: every (lookahead, hold) pair, calls of 1000, 1, 16, 17, 300, 255, 256 and 257 frames with events between
    them, 1, 3 or 8 buses by the pair's place in the list, every other call without stems, static returns and a master fader of 0.7.
    On the model, before anything is compared: at least a quarter of the case's frames are limited."""
    a, b = _handles()
    nb = (1, 3, 8)[PAIRS.index((L, H)) % 3]
    for syn in (a, b):
        for bus in range(s2.MAX_BUSES):
            syn.set_bus_return(bus, 1.0 - bus / 16.0)
        syn.set_master_fader(0.7)
        syn.snap_master()
    lim = Lim(L, H)
    # the model first, over the twin alone: the case must limit before the device is asked anything
    xs = []
    for fill, n in enumerate(CALLS):
        _events((b,), V, fill)
        xs.append(b.sample_master(n, SR, nb)[0])
    probe = Lim(L, H, float(np.abs(xs[0]).max()) / 2.0)
    for x in xs:
        probe.expect(x)
    print("L %d H %d, %d buses: %.3f of the model's frames are limited" % (L, H, nb, probe.limited()))
    assert probe.limited() >= 0.25, probe.limited()
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
    xh, gh = a.limiter_state()
    assert_bits_equal_finite(xh, lim.xh, "xh read back")
    assert_bits_equal_finite(gh, lim.gh, "gh read back")


def _timed(handles, fill, frames):
    ev = [(ON, 50 + fill + 7 * k, f, v) for k, (f, v) in enumerate(zip(frames, (0.6, 1.0)))]
    for syn in handles if ev else ():
        syn.note_events(np.array(ev, dtype=s2.NOTE_EVENT_DTYPE))


@pytest.mark.parametrize("L,H", [(48, 0), (240, 480), (1024, 4096)])
def test_past_one_block_with_reverbs_ramps_events_and_slices(L, H, monkeypatch):
    """max_frames = 2501 on 32-voice pools: calls of 1024 (four full workgroups), 1025 (a fifth of one frame), 2501, 7 and 1031
    frames; timed note_ons at 1008 and 1024 where the call reaches them and a rows buffer of 48 frames, so the master arrives in
    event segments and slices; a K = 300 reverb on bus 1 of three on both handles; returns and the master fader on their way in
    every call.  In the last three calls the master fader is at 2^-6 and lower: a quiet tail, in which — asserted on the model, for
    the two pairs whose recovery of L + H + W frames fits into it — at least a tenth of the case's frames pass with a gain of exactly
    1, while at least a quarter are limited."""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    a, b = _handles(32, max_frames=2501)
    for syn in (a, b):
        syn.set_bus_reverb(1, _ir(300, 23, True), 0.25, 1.0)
    lim = Lim(L, H)
    for fill, n in enumerate([1024, 1025, 2501, 7, 1031, 2501]):
        _events((a, b), 32, fill)
        _timed((a, b), fill, [f for f in (1008, 1024) if f < n])
        for syn in (a, b):
            syn.set_bus_return(0, [0.25, 1.0, 0.5, 0.0, 0.75, 1.0][fill])
            syn.set_bus_return(2, [1.0, 0.5, 1.0, 0.25, 1.0, 1.0][fill])
            syn.set_master_fader([0.7, 1.0, 0.85, 2.0 ** -6, 2.0 ** -6, 2.0 ** -8][fill])
        _lfill(a, b, lim, n, 3, "past one block, L %d H %d, fill %d of %d frames" % (L, H, fill, n), stems=fill % 2 == 1)
    sp = np.concatenate(lim.sp)
    print("L %d H %d: %.3f of the model's frames are limited, %.3f pass at 1" % (L, H, (sp < 1.0).mean(), (sp == 1.0).mean()))
    assert (sp < 1.0).mean() >= 0.25
    if 2 * L + H + 1 < 3532:                                     # the tail is 7 + 1031 + 2501 frames long
        assert (sp == 1.0).mean() >= 0.1
    a.L.s2r_debug_pan_slice.restype = C.c_uint32
    a.L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    assert a.L.s2r_debug_pan_slice(a.h) == 48


@pytest.mark.parametrize("L,H", [(240, 480), (254, 0), (127, 128), (1024, 4096)])
def test_every_block_edge(L, H):
    """the kernel's workgroup covers 256 frames and its state loop strides by the whole grid: calls of 255, 256, 257, 511, 512, 513,
    767, 768, 769, 1023 and 1024 frames — with G = 960 the three-workgroup calls go round the state loop twice and the 1024-frame
    call once; with G = 6144 every call goes round it several times.  L + H + 1 = 255 and 256 sit at the edges of the minimum's
    doubling: one below a power of two, and the power itself."""
    a, b = _handles(64)
    lim = Lim(L, H)
    for fill, n in enumerate([255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024]):
        _events((a, b), 64, fill)
        _lfill(a, b, lim, n, 2, "block edges, L %d H %d, fill %d of %d frames" % (L, H, fill, n), stems=False)
    print("block edges, L %d H %d: %.3f of the model's frames are limited" % (L, H, lim.limited()))
    assert lim.limited() >= 0.25
    xh, gh = a.limiter_state()
    assert_bits_equal_finite(xh, lim.xh, "xh read back")
    assert_bits_equal_finite(gh, lim.gh, "gh read back")


def test_properties_on_the_device():
    """no model in the loop.  Under the largest ceiling, far above the twin's peak, the master is the twin's delayed by L frames in
    every bit, across calls, behind L frames of +0.0, min_gain is 1 and out_peak the peak of what came out; after
    clear_master_limiter both handles agree again with no delay; set again, the delay starts from +0.0 once more.  sample_buses and
    sample_panned ignore a limiter, and their calls do not move its state."""
    a, b = _handles()
    L = 48
    a.set_master_limiter(2.0 ** 20, L, 7)
    xs, ys = [], []
    for fill, n in enumerate([300, 17, 1, 256, 1000]):
        _events((a, b), V, fill)
        x, st_b = b.sample_master(n, SR, 8)
        y, st = a.sample_master(n, SR, 8)
        xs.append(x), ys.append(y)
        assert_bits_equal_finite(st, st_b, "the stems are not delayed")
        for g, w in zip(a.meters(), b.meters()):
            assert_bits_equal_finite(g, w, "the master section's meters are over the limiter's input")
        assert a.limiter_meters() == (1.0, float(np.abs(y).max()))
        if fill == 1:                                            # other fills between two master fills: ignored, and nothing moves
            state = a.limiter_state()
            _events((a, b), V, 10)
            assert_bits_equal_finite(a.sample_buses(64, SR, 8), b.sample_buses(64, SR, 8), "a bus fill beside the limiter")
            assert_bits_equal_finite(a.sample_panned(64, SR), b.sample_panned(64, SR), "a panned fill beside the limiter")
            for g, w in zip(a.limiter_state(), state):
                assert_bits_equal_finite(g, w, "the state after other fills")
    x, y = np.concatenate(xs), np.concatenate(ys)
    assert float(np.abs(x).max()) < 2.0 ** 20 and ubits(x).any()
    assert_bits_equal_finite(y[L:], x[:len(x) - L], "the delay")
    assert not ubits(y[:L]).any()
    a.clear_master_limiter()
    assert a.get_master_limiter() == (0.0, 0, 0)
    _events((a, b), V, 5)
    assert_bits_equal_finite(a.sample_master(300, SR, 8)[0], b.sample_master(300, SR, 8)[0], "after clear_master_limiter")
    a.set_master_limiter(2.0 ** 20, L, 7)                        # off, then on: the initial state
    _events((a, b), V, 6)
    x, y = b.sample_master(300, SR, 8)[0], a.sample_master(300, SR, 8)[0]
    assert_bits_equal_finite(y[L:], x[:300 - L], "the delay after setting it again")
    assert not ubits(y[:L]).any()


def test_a_ceiling_change_keeps_the_state_and_a_lookahead_change_resets_it():
    """in the middle of a gain reduction the ceiling moves: the next call is the model with the new ceiling over the SAME state —
    and differs from the model over a reset state, asserted on the model; then the lookahead moves, and then the hold: each time the
    next call is the model from the initial state"""
    a, b = _handles()
    lim = Lim(64, 100)
    _events((a, b), V, 0)
    _lfill(a, b, lim, 300, 4, "before the changes")
    assert lim.gh.min() < 1.0
    lim.set((a,), lim.c * 1.5)
    _events((a, b), V, 1)
    x, got = _lfill(a, b, lim, 300, 4, "after the ceiling moved")
    assert not np.array_equal(ubits(got), ubits(np_limiter(x, lim.c, 64, 100)[0]))
    lim.set((a,), L=48)
    assert not ubits(lim.xh).any() and (lim.gh == 1.0).all()
    _events((a, b), V, 2)
    _lfill(a, b, lim, 300, 4, "after the lookahead moved")
    lim.set((a,), H=0)
    _events((a, b), V, 3)
    _lfill(a, b, lim, 300, 4, "after the hold moved")
    assert lim.limited() >= 0.25


def test_checkpoint_in_the_middle_of_a_gain_reduction():
    """voices, pans, mix, sends and the limiter — parameters through get_master_limiter, state through limiter_state, read while gh
    holds gains below 1 — into a fresh handle: the continuations are equal on bits, and equal to the model"""
    a, b = _handles(max_frames=512)
    lim = Lim(240, 480)
    _events((a, b), V, 0)
    _lfill(a, b, lim, 400, 4, "before the checkpoint")
    _events((a, b), V, 1)
    _lfill(a, b, lim, 100, 4, "before the checkpoint, a call shorter than both histories")
    xh, gh = a.limiter_state()
    assert gh.min() < 1.0 and ubits(xh).any()
    params = a.get_master_limiter()
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    c = s2.Synth(V, max_frames=512, block_voices=64)
    c.set_patch_bank(_bank())
    c.import_state(state)
    c.set_voice_pans(pans)
    c.set_voice_mix(gains, buses)
    c.set_voice_sends(sends, sbuses)
    c.set_master_limiter(*params)
    c.set_limiter_state(xh, gh)
    for g, w in zip(c.limiter_state(), (xh, gh)):
        assert_bits_equal_finite(g, w, "the restored state read back")
    for k, n in enumerate([100, 400]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        _, got = _lfill(a, b, lim, n, 4, "the checkpointed handle, fill %d" % k)
        assert_bits_equal_finite(c.sample_master(n, SR, 4)[0], got, "the resumed handle, fill %d" % k)
        assert c.limiter_meters() == a.limiter_meters()


def test_refusals_change_nothing():
    """refused master fills — no bus, nine buses, short stems, a null master, too many frames, a begun fill in flight — leave the
    limiter's state and meters as they were, and the next fill equals the model as if they had not happened.  A device-list handle
    refuses every limiter entry and renders on; a handle with an exchange attached takes the setters and refuses the fill."""
    a, b = _handles(max_frames=256)
    lim = Lim(64, 100)
    _events((a, b), V, 0)
    _lfill(a, b, lim, 100, 2, "before the refusals")
    L, h = a.L, a.h
    out, st = np.full(2 * 300, 7.0, dtype=F), np.full(2 * 2 * 300, 7.0, dtype=F)
    op, sp = out.ctypes.data_as(s2s._f32p), st.ctypes.data_as(s2s._f32p)
    refusals = [
        ("no bus", lambda: L.s2r_fill_master(h, op, sp, st.size, 0, 64, SR), s2s.S2R_ERR_INVALID),
        ("nine buses", lambda: L.s2r_fill_master(h, op, sp, st.size, 9, 64, SR), s2s.S2R_ERR_INVALID),
        ("short stems", lambda: L.s2r_fill_master(h, op, sp, 2 * 2 * 64 - 1, 2, 64, SR), s2s.S2R_ERR_INVALID),
        ("null master", lambda: L.s2r_fill_master(h, None, sp, st.size, 2, 64, SR), s2s.S2R_ERR_INVALID),
        ("too many frames", lambda: L.s2r_fill_master(h, op, sp, st.size, 2, 257, SR), s2s.S2R_ERR_TOO_MANY_FRAMES),
    ]
    for fill, (name, call, status) in enumerate(refusals):
        state, meters = a.limiter_state(), a.limiter_meters()
        assert call() == status, name
        assert (out == 7.0).all() and (st == 7.0).all(), name   # nothing was written
        assert a.limiter_meters() == meters, name
        for g, w in zip(a.limiter_state(), state):
            assert_bits_equal_finite(g, w, name + ": the state")
        _events((a, b), V, fill + 1)
        _lfill(a, b, lim, 64, 2, "after the refusal: " + name)
    for bad in [(float("nan"), 64, 100), (0.25, 0, 0), (0.25, 1025, 0), (0.25, 64, 4097)]:          # a refused setter likewise
        assert L.s2r_set_master_limiter(h, *bad) == s2s.S2R_ERR_PATCH_RANGE
    assert a.get_master_limiter() == (float(F(lim.c)), 64, 100)
    a.sample_begin(64, SR)
    assert L.s2r_fill_master(h, op, sp, st.size, 2, 64, SR) == s2s.S2R_ERR_INVALID
    assert (out == 7.0).all()
    b.sample(np.empty(64, dtype=F), SR)
    a.sample_end(np.empty(64, dtype=F))
    _events((a, b), V, 7)
    _lfill(a, b, lim, 64, 2, "after the fill in flight")
    # a device list refuses every entry and renders on
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    one = s2.Synth(512, max_frames=64, mix_groups=2)
    for syn in (multi, one):
        for v in range(512):
            syn.note_on(36 + v % 61)
    f, n = C.c_float(), C.c_uint32()
    M, mh = multi.L, multi.h
    buf = np.zeros(512, dtype=F)
    bp = buf.ctypes.data_as(s2s._f32p)
    assert M.s2r_set_master_limiter(mh, 0.25, 48, 0) == s2s.S2R_ERR_INVALID
    assert M.s2r_clear_master_limiter(mh) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_master_limiter(mh, C.byref(f), C.byref(n), C.byref(n)) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_limiter_state(mh, bp, 96, bp, 96) == s2s.S2R_ERR_INVALID
    assert M.s2r_set_limiter_state(mh, bp, 96, bp, 96) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_limiter_meters(mh, C.byref(f), C.byref(f)) == s2s.S2R_ERR_INVALID
    assert M.s2r_set_master_limiter(mh, 0.25, 0, 0) == s2s.S2R_ERR_PATCH_RANGE             # the values are looked at first
    x, y = multi.sample(np.empty(64, dtype=F), SR), one.sample(np.empty(64, dtype=F), SR)
    assert np.abs(y).max() > 0.0
    assert_bits_equal_finite(x, y, "the device-list handle after the refused limiter calls")
    # an exchange attached: the setters are taken, the fill is refused like the bus fill
    xg = s2.Synth(V, max_frames=64, block_voices=64)
    xg.exchange_create(1)
    xg.set_master_limiter(0.25, 4, 3)
    xg.set_limiter_state(np.zeros((4, 2), dtype=F), np.full(11, 0.5, dtype=F))
    assert xg.get_master_limiter() == (0.25, 4, 3) and (xg.limiter_state()[1] == 0.5).all()
    assert xg.L.s2r_fill_master(xg.h, op, sp, st.size, 2, 64, SR) == s2s.S2R_ERR_INVALID
    assert (out == 7.0).all() and (st == 7.0).all()
    xg.clear_master_limiter()


def test_timing_entry_and_range_checks_on_a_handle():
    """s2r_debug_limiter_ms: -1 without s2r_set_timing; under it the limiter kernel's time of the last master fill, 0 when that
    fill ran none.  Then the range checks on a real handle (test_limiter_host.check_ranges)."""
    a = _handles()[0]
    ms = a.L.s2r_debug_limiter_ms
    ms.restype, ms.argtypes = C.c_float, [C.c_void_p]
    _events((a,), V, 0)
    a.set_master_limiter(0.25, 48, 0)
    a.sample_master(300, SR, 2)
    assert ms(a.h) == -1.0
    a.set_timing(True)
    a.sample_master(300, SR, 2)
    assert 0.0 < ms(a.h) < 100.0
    a.clear_master_limiter()
    a.sample_master(300, SR, 2)
    assert ms(a.h) == 0.0
    check_ranges(s2.Synth(8, max_frames=64))
