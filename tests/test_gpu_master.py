"""The master section on the device.  Twin handles are fed the same events; the twin's sample_buses output is y — the
stems, reverbs included where both carry them — and the expectation is the numpy float32 model of the rule
(test_master_host.np_master, np_meters) over y with the returns' and the master fader's pairs carried from call to call.  No oracle
and no s2r_master_reference is in the loop.

Handles, events and the one-pole bank are tests/test_gpu_reverb.py's: 272 voices in 64-voice workgroups, eight programs on eight
buses, buses 6 and 7 sounding through sends alone, the voices booked past a call's last bus folded onto it.  Every comparison is on
bits with no NaN allowance (helpers.assert_bits_equal_finite) unless a test says why it compares values."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_gpu_buses import ubits
from test_gpu_panned import ON
from test_gpu_reverb import SR, V, Model, _bank, _events, _handles, _ir
from test_master_host import check_ranges, np_energy, np_master, np_meters
from test_reverb_host import crafted_denormal

pytestmark = pytest.mark.gpu
F = np.float32
CALLS = [1000, 1, 16, 17, 300, 255, 256, 257]


class Master:
    """the master section of a handle in numpy: the returns' and the master fader's target and applied positions"""

    def __init__(self):
        self.r0, self.r1 = np.ones(s2.MAX_BUSES, dtype=F), np.ones(s2.MAX_BUSES, dtype=F)
        self.m0, self.m1 = F(1.0), F(1.0)

    def ret(self, handles, bus, level):
        for syn in handles:
            syn.set_bus_return(bus, level)
        self.r1[bus] = level

    def fader(self, handles, level):
        for syn in handles:
            syn.set_master_fader(level)
        self.m1 = F(level)

    def snap(self, handles=()):
        for syn in handles:
            syn.snap_master()
        self.r0, self.m0 = self.r1.copy(), self.m1

    def moving(self, nb):
        return bool((self.r0[:nb] != self.r1[:nb]).any() or self.m0 != self.m1)

    def static(self, y):
        """what the call would return from the applied positions alone"""
        nb = y.shape[0]
        return np_master(y, self.r0[:nb], self.r0[:nb], self.m0, self.m0)

    def expect(self, y):
        """what a call returns whose stems are y [n_buses, N, 2]; every pair arrives"""
        nb = y.shape[0]
        want = np_master(y, self.r0[:nb], self.r1[:nb], self.m0, self.m1)
        self.snap()
        return want

    def check_committed(self, syn):
        assert self.r0.tolist() == self.r1.tolist() and self.m0 == self.m1
        for b in range(s2.MAX_BUSES):
            assert syn.get_bus_return(b) == (float(self.r1[b]), float(self.r1[b])), b
        assert syn.get_master_fader() == (float(self.m1), float(self.m1))


def _check_meters(syn, y, master, what):
    peak, energy = syn.meters()
    wp, we = np_meters(y, master)
    assert_bits_equal_finite(peak, wp, what + ": peaks")
    assert_bits_equal_finite(energy, we, what + ": energies")
    return peak, energy


def _mfill(a, b, mm, n, nb, what, stems=True):
    """one call on both handles: the twin's sample_buses gives y, the master fill of `a` is the model over y, its stems are y and its
    meters are the rule over y and the model's master"""
    y = b.sample_buses(n, SR, nb)
    assert np.isfinite(y).all()
    want = mm.expect(y)
    got, st = a.sample_master(n, SR, nb, stems=stems)
    assert_bits_equal_finite(got, want, what + ": master")
    if stems:
        assert_bits_equal_finite(st, y, what + ": stems")
    else:
        assert st is None
    _check_meters(a, y, want, what)
    return y, got


@pytest.mark.parametrize("n_buses", [1, 2, 3, 8])
def test_master_is_the_rule_over_the_stems(n_buses):
    """the parity matrix: static returns 1 - b / 16 and a master fader of 0.7, calls of 1000, 1, 16, 17, 300, 255, 256 and 257 frames
    with events between them.  The call's last bus carries the folded voices; with eight buses, buses 6 and 7 sound through sends
    only — every bus is asserted to sound, so no return multiplies silence."""
    a, b = _handles()
    mm = Master()
    for bus in range(s2.MAX_BUSES):
        mm.ret((a,), bus, 1.0 - bus / 16.0)
    mm.fader((a,), 0.7)
    mm.snap((a,))
    for fill, n in enumerate(CALLS):
        _events((a, b), V, fill)
        y, got = _mfill(a, b, mm, n, n_buses, "%d buses, fill %d of %d frames" % (n_buses, fill, n))
        assert all(ubits(y[q]).any() for q in range(n_buses)) and ubits(got).any()
        if n_buses > 1:                                          # the returns are visible: not the plain sum times the master
            assert not np.array_equal(ubits(got), ubits(np_master(y, np.ones(n_buses, dtype=F), np.ones(n_buses, dtype=F), 0.7, 0.7)))
    mm.check_committed(a)


def test_returns_and_master_ramp_across_a_call():
    """returns and master move between calls, buses 1 and 3 of four stay: every call against the ramped model, applied read back
    equal to target afterwards; a ramped call of more than one frame differs from its static expectation in bits (asserted on the
    model); a one-frame call equals the static one and commits; snap_master is a hard cut."""
    a, b = _handles()
    mm = Master()
    mm.ret((a,), 1, 0.75)
    mm.ret((a,), 3, 1.0 / 3.0)
    mm.snap((a,))
    walk = [(300, 0.0, 0.5, 0.25), (257, 1.0, 0.5, 1.0), (1, 0.5, 0.0, 0.5), (1000, 0.5, 1.0, 0.0), (16, 0.25, 1.0, 0.7), (17, 0.25, 1.0, 0.7)]
    for fill, (n, ret0, ret2, fader) in enumerate(walk):
        _events((a, b), V, fill)
        mm.ret((a,), 0, ret0)
        mm.ret((a,), 2, ret2)
        mm.fader((a,), fader)
        moving = mm.moving(4)
        assert moving == (fill != 5)
        assert a.get_bus_return(0) == (float(mm.r1[0]), float(mm.r0[0])) and a.get_master_fader() == (float(mm.m1), float(mm.m0))
        y = b.sample_buses(n, SR, 4)
        static = mm.static(y)
        want = mm.expect(y)
        if n == 1 or not moving:
            assert_bits_equal_finite(want, static, "fill %d: the static expectation" % fill)
        else:
            assert not np.array_equal(ubits(want), ubits(static)), "fill %d: the ramp changes no bit of the model" % fill
        got, st = a.sample_master(n, SR, 4)
        assert_bits_equal_finite(got, want, "ramped fill %d of %d frames: master" % (fill, n))
        assert_bits_equal_finite(st, y, "ramped fill %d: stems" % fill)
        _check_meters(a, y, want, "ramped fill %d" % fill)
        mm.check_committed(a)
    # a hard cut: the targets set, snapped, and the next call is static at them
    mm.ret((a,), 0, 1.0)
    mm.ret((a,), 1, 0.0)
    mm.fader((a,), 0.5)
    mm.snap((a,))
    mm.check_committed(a)
    _events((a, b), V, len(walk))
    y = b.sample_buses(300, SR, 4)
    assert_bits_equal_finite(a.sample_master(300, SR, 4)[0], mm.static(y), "after snap_master")


def test_with_reverbs_the_histories_and_faders_move_as_in_a_bus_fill():
    """both handles carry a K = 257 reverb on bus 0 and a K = 600 reverb on bus 6 (send-only), so the twin's sample_buses is y with
    the reverbs in it.  Three master fills — shorter than both histories, longer than both, between them — while program 0's fader
    moves; then a sample_buses call on both handles is equal on bits: the master fill moved the histories and committed the program
    faders exactly as the bus fill does."""
    a, b = _handles()
    mm = Master()
    for syn in (a, b):
        syn.set_bus_reverb(0, _ir(257, 21, True), 0.25, 1.0)
        syn.set_bus_reverb(6, _ir(600, 22), 1.0, 0.5)
    mm.ret((a,), 6, 0.5)
    mm.snap((a,))
    faders = [(0.25, 1.0), (0.7, -0.5), (0.7, -0.5)]
    for fill, n in enumerate([100, 1000, 300]):
        _events((a, b), V, fill)
        for syn in (a, b):
            syn.set_program_fader(0, *faders[fill])
        mm.ret((a,), 0, [0.5, 1.0, 1.0][fill])
        mm.fader((a,), [0.7, 0.7, 0.25][fill])
        y, _ = _mfill(a, b, mm, n, 8, "with reverbs, fill %d of %d frames" % (fill, n))
        assert ubits(y[6]).any()
        f = a.get_program_fader(0)
        assert f == b.get_program_fader(0) and f[:2] == f[2:]    # committed on both
        for bus in (0, 6):
            assert_bits_equal_finite(a.bus_reverb_history(bus), b.bus_reverb_history(bus), "history of bus %d after fill %d" % (bus, fill))
    _events((a, b), V, 3)
    assert_bits_equal_finite(a.sample_buses(300, SR, 8), b.sample_buses(300, SR, 8), "a bus fill after the master fills")
    _events((a, b), V, 4)
    _mfill(a, b, mm, 64, 8, "a master fill after the bus fill")


def _timed(handles, fill, frames):
    ev = [(ON, 50 + fill + 7 * k, f, v) for k, (f, v) in enumerate(zip(frames, (0.6, 1.0)))]
    for syn in handles if ev else ():
        syn.note_events(np.array(ev, dtype=s2.NOTE_EVENT_DTYPE))


def test_past_one_block_and_one_tile(monkeypatch):
    """max_frames = 2501 on 32-voice pools: calls of 1024 (four full meter blocks), 1025 (a fifth block of one frame), 2501 (ten
    blocks, the last of 197 frames), 7 and 1031 frames; timed note_ons at 1008 and 1024 where the call reaches them and a rows
    buffer of 48 frames, so the stems arrive in event segments and slices; a K = 300 reverb on bus 1 of three on both handles, so its
    finish kernel is the last stem writer past its tile of 1024 frames; returns and master on their way in every call: the ramp's
    index counts from the start of the call, not of a block."""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    a, b = _handles(32, max_frames=2501)
    mm = Master()
    for syn in (a, b):
        syn.set_bus_reverb(1, _ir(300, 23, True), 0.25, 1.0)
    for fill, n in enumerate([1024, 1025, 2501, 7, 1031]):
        _events((a, b), 32, fill)
        _timed((a, b), fill, [f for f in (1008, 1024) if f < n])
        mm.ret((a,), 0, [0.25, 1.0, 0.5, 0.0, 0.75][fill])
        mm.ret((a,), 2, [1.0, 0.5, 1.0, 0.25, 1.0][fill])
        mm.fader((a,), [0.7, 0.25, 1.0, 0.5, 0.7][fill])
        y = b.sample_buses(n, SR, 3)
        nb = y.shape[0]
        want = np_master(y, mm.r0[:nb], mm.r1[:nb], mm.m0, mm.m1)
        if n > 256:                                              # a block-relative index is another signal: the test can tell them apart
            i = np.arange(n) % 256
            wrong = want.copy()
            for c in range(2):
                t = np.zeros(n, dtype=F)
                for q in range(nb):
                    d = F(mm.r1[q] - mm.r0[q]) / F(n)
                    t = t + (mm.r0[q] + i.astype(F) * d) * y[q, :, c]
                wrong[:, c] = (mm.m0 + i.astype(F) * (F(mm.m1 - mm.m0) / F(n))) * t
            assert not np.array_equal(ubits(wrong), ubits(want))
        mm.snap()
        got, st = a.sample_master(n, SR, 3)
        what = "past one block, fill %d of %d frames" % (fill, n)
        assert_bits_equal_finite(got, want, what + ": master")
        assert_bits_equal_finite(st, y, what + ": stems")
        _check_meters(a, y, want, what)
        assert all(ubits(y[q]).any() for q in range(3))
    a.L.s2r_debug_pan_slice.restype = C.c_uint32
    a.L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    assert a.L.s2r_debug_pan_slice(a.h) == 48


def test_meters():
    """no model of the sum in the loop: the peaks are max |.| of the returned stems and master on bits, the energies the tree rule
    over them; s2r_get_meters returns S2R_ERR_INVALID before the first master fill and with a capacity too small; a refused call
    leaves the meters as they were; a call of fewer buses reports fewer entries."""
    a, b = _handles()
    L, h = a.L, a.h
    n = C.c_uint32()
    buf = np.zeros(2 * 9, dtype=F)
    p = buf.ctypes.data_as(s2s._f32p)
    assert L.s2r_get_meters(h, C.byref(n), p, p, buf.size) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        a.meters()
    assert err.value.status == s2s.S2R_ERR_INVALID
    _events((a, b), V, 0)
    a.sample_buses(64, SR, 8), b.sample_buses(64, SR, 8)        # a bus fill makes no meters
    assert L.s2r_get_meters(h, C.byref(n), p, p, buf.size) == s2s.S2R_ERR_INVALID
    a.set_bus_return(2, 0.25)
    a.set_master_fader(0.5)
    for fill, (frames, nb) in enumerate([(1000, 8), (257, 3), (1, 1)]):
        _events((a, b), V, fill + 1)
        b.sample_buses(frames, SR, nb)
        got, st = a.sample_master(frames, SR, nb)
        peak, energy = a.meters()
        assert peak.shape == (nb + 1, 2) and energy.shape == (nb + 1, 2)
        chans = np.concatenate([st, got[None]], axis=0)
        assert_bits_equal_finite(peak, np.abs(chans).max(axis=1), "fill %d: peaks" % fill)
        assert_bits_equal_finite(energy, np.array([[np_energy(ch[:, c]) for c in range(2)] for ch in chans], dtype=F), "fill %d: energies" % fill)
        assert (peak > 0.0).all() and (energy > 0.0).all()
        if frames > 256:
            plain = np.array([[np_energy(ch[:, c], tree=False) for c in range(2)] for ch in chans], dtype=F)
            assert not np.array_equal(ubits(plain), ubits(energy))   # the tree is visible in the device's bits
        assert L.s2r_get_meters(h, C.byref(n), p, p, 2 * (nb + 1) - 1) == s2s.S2R_ERR_INVALID
        assert L.s2r_get_meters(h, C.byref(n), None, None, 2 * (nb + 1)) == s2s.S2R_OK and n.value == nb
        assert L.s2r_get_meters(h, None, p, None, buf.size) == s2s.S2R_OK
        assert_bits_equal_finite(buf[:2 * (nb + 1)].reshape(-1, 2), peak, "peaks through the raw entry")
    before = a.meters()
    out = np.empty(2 * 1100, dtype=F)
    op = out.ctypes.data_as(s2s._f32p)
    assert L.s2r_fill_master(h, op, None, 0, 9, 16, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_master(h, op, None, 0, 2, 1025, SR) == s2s.S2R_ERR_TOO_MANY_FRAMES
    assert L.s2r_fill_master(h, None, None, 0, 2, 16, SR) == s2s.S2R_ERR_INVALID
    after = a.meters()
    for x, y in zip(before, after):
        assert_bits_equal_finite(y, x, "the meters after refused calls")


def test_properties_without_a_model():
    """master only equals the master of the same call with stems (twin handles), meters included; one bus with every level 1: the
    master is the stem as values, and on bits wherever the stem is not -0.0 (+0.0 + 1 * -0.0 is +0.0); every return 0.5 under a
    master of 1: the sum in bus order of exact halves; a muted bus: the model over the other buses, on bits."""
    a, b, c = _handles(n=3)
    for fill, n in enumerate([300, 17]):
        _events((a, b, c), V, fill)
        a.set_bus_return(1, [0.25, 1.0][fill])
        c.set_bus_return(1, [0.25, 1.0][fill])
        with_stems, st = a.sample_master(n, SR, 3)
        only, none = c.sample_master(n, SR, 3, stems=False)
        assert none is None and ubits(with_stems).any()
        assert_bits_equal_finite(only, with_stems, "master only, fill %d" % fill)
        assert_bits_equal_finite(st, b.sample_buses(n, SR, 3), "the stems beside it")
        for x, y in zip(a.meters(), c.meters()):
            assert_bits_equal_finite(y, x, "the meters of the master-only call")
    for syn in (a, c):
        syn.set_bus_return(1, 1.0)
        syn.snap_master()
    # one bus, every level 1
    _events((a, b, c), V, 2)
    got, st = a.sample_master(300, SR, 1)
    b.sample_buses(300, SR, 1), c.sample_master(300, SR, 1)
    assert np.array_equal(got, st[0]) and ubits(got).any()
    keep = ubits(st[0]) != 0x80000000
    assert np.array_equal(ubits(got)[keep], ubits(st[0])[keep])
    # every return 0.5, master 1: exact halves, added in bus order
    for bus in range(s2.MAX_BUSES):
        a.set_bus_return(bus, 0.5)
    a.snap_master()
    _events((a, b, c), V, 3)
    y = b.sample_buses(300, SR, 8)
    c.sample_buses(300, SR, 8)
    got = a.sample_master(300, SR, 8)[0]
    mag = np.abs(y.astype(np.float64))
    assert not ((mag > 0.0) & (mag < 2.0 ** -125)).any()         # halving is exact: no half is a denormal
    t = np.zeros((300, 2), dtype=F)
    for q in range(8):
        t = t + y[q] * F(0.5)
    assert_bits_equal_finite(got, t, "every return 0.5")
    # bus 2 of four muted: the model over buses 0, 1 and 3
    for bus in range(s2.MAX_BUSES):
        a.set_bus_return(bus, 1.0 - bus / 16.0)
    a.set_bus_return(2, 0.0)
    a.set_master_fader(0.7)
    a.snap_master()
    _events((a, b, c), V, 4)
    y = b.sample_buses(300, SR, 4)
    got = a.sample_master(300, SR, 4)[0]
    r = np.array([1.0, 1.0 - 1.0 / 16.0, 1.0 - 3.0 / 16.0], dtype=F)
    assert ubits(y[2]).any()
    assert_bits_equal_finite(got, np_master(y[[0, 1, 3]], r, r, 0.7, 0.7), "bus 2 muted")


def test_denormals_are_kept():
    """an idle bus — no voice is ever started — whose K = 1300 reverb carries a crafted history: response x 2^-70 over a uniform
    history x 2^-68, as in tests/test_gpu_reverb_tiles.py, under a return of 0.5 and a master of 1.  The condition is stated on the
    model alone and before anything is compared, so a flushing device cannot pass by agreeing with a flushed expectation: at least
    90 % of the model's first K - 1 master frames are non-zero and below 2^-126.  Master, stems and meters on bits: the bus's peak is
    a denormal and its energy — squares of denormals — is +0.0 by the rule."""
    K, n = 1300, 1500
    pairs = [crafted_denormal(K, 41 + c) for c in range(2)]
    ir, hist = (np.stack([p[k] for p in pairs], axis=1) for k in range(2))
    model = Model()
    model.set(1, ir, 0.0, 1.0)
    model.fx[1]["hist"] = hist.copy()
    y = model.expect(np.zeros((2, n, 2), dtype=F))
    r = np.array([1.0, 0.5], dtype=F)
    want = np_master(y, r, r, 1.0, 1.0)
    mag = np.abs(want[:K - 1].astype(np.float64))
    assert ((mag > 0.0) & (mag < 2.0 ** -126)).mean() >= 0.9
    a = _handles(32, max_frames=1504)[0]
    a.set_bus_reverb(1, ir, 0.0, 1.0)
    a.set_bus_reverb_history(1, hist)
    a.set_bus_return(1, 0.5)
    a.snap_master()
    got, st = a.sample_master(n, SR, 2)
    assert_bits_equal_finite(got, want, "denormal master")
    assert_bits_equal_finite(st, y, "denormal stems")
    peak, energy = _check_meters(a, y, want, "denormal meters")
    assert 0.0 < float(peak[1].min()) < 2.0 ** -126 and not ubits(energy).any()


def test_other_fills_ignore_the_master_section():
    """returns and master away from 1, one of them on its way: sample_buses and sample_panned are the twin's on bits and commit
    nothing"""
    a, b = _handles()
    for bus in range(s2.MAX_BUSES):
        a.set_bus_return(bus, 0.25)
    a.set_master_fader(0.5)
    a.snap_master()
    a.set_bus_return(1, 1.0)
    a.set_master_fader(0.0)
    for fill, n in enumerate([300, 17]):
        _events((a, b), V, fill)
        x = b.sample_buses(n, SR, 8)
        assert ubits(x).any()
        assert_bits_equal_finite(a.sample_buses(n, SR, 8), x, "bus fill beside the master section")
        assert_bits_equal_finite(a.sample_panned(n, SR), b.sample_panned(n, SR), "panned fill beside the master section")
    assert a.get_bus_return(1) == (1.0, 0.25) and a.get_master_fader() == (0.0, 0.5)


def test_checkpoint_in_the_middle_of_a_ramp():
    """state, pans, mix, sends, program faders and the return and master pairs, read while targets differ from applied, into a fresh
    handle — set the applied values, snap, set the targets: the continuations are equal on bits"""
    a, b = _handles(max_frames=512)
    mm = Master()
    mm.ret((a,), 0, 0.5)
    mm.ret((a,), 2, 0.25)
    mm.fader((a,), 0.7)
    _events((a, b), V, 0)
    _mfill(a, b, mm, 200, 4, "before the checkpoint")
    mm.ret((a,), 0, 1.0)
    mm.ret((a,), 3, 0.0)
    mm.fader((a,), 0.25)
    rets = [a.get_bus_return(q) for q in range(s2.MAX_BUSES)]
    fader = a.get_master_fader()
    assert rets[0] == (1.0, 0.5) and rets[3] == (0.0, 1.0) and fader[0] != fader[1]
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    c = s2.Synth(V, max_frames=512, block_voices=64)
    c.set_patch_bank(_bank())
    c.import_state(state)
    c.set_voice_pans(pans)
    c.set_voice_mix(gains, buses)
    c.set_voice_sends(sends, sbuses)
    for q, (target, applied) in enumerate(rets):
        c.set_bus_return(q, applied)
    c.set_master_fader(fader[1])
    c.snap_master()
    for q, (target, applied) in enumerate(rets):
        c.set_bus_return(q, target)
    c.set_master_fader(fader[0])
    assert [c.get_bus_return(q) for q in range(s2.MAX_BUSES)] == rets and c.get_master_fader() == fader
    for k, n in enumerate([100, 400]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        if k == 1:
            mm.ret((a, c), 2, 1.0)
        _, got = _mfill(a, b, mm, n, 4, "the checkpointed handle, fill %d" % k)
        got_c, st_c = c.sample_master(n, SR, 4)
        assert_bits_equal_finite(got_c, got, "the resumed handle, fill %d" % k)
        for x, y in zip(a.meters(), c.meters()):
            assert_bits_equal_finite(y, x, "the resumed handle's meters, fill %d" % k)


def test_refusals_change_nothing():
    """n_buses 0 and 9, a stems capacity too small, a null master_lr, too many frames and a begun fill in flight: after each refusal
    the next master fill equals the model, as if the refused call had not happened — returns and master still on their way, meters and
    reverb history as they were.  A device-list handle refuses every handle entry; a handle with an exchange attached takes the
    setters and refuses the fill."""
    a, b = _handles(max_frames=256)
    mm = Master()
    for syn in (a, b):
        syn.set_bus_reverb(0, _ir(300, 24), 0.25, 1.0)
    _events((a, b), V, 0)
    _mfill(a, b, mm, 100, 2, "before the refusals")
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
        mm.ret((a,), 0, [0.5, 1.0, 0.25, 0.75, 1.0][fill])
        mm.fader((a,), [0.7, 0.25, 1.0, 0.5, 0.7][fill])
        meters, hist, pair = a.meters(), a.bus_reverb_history(0), a.get_bus_return(0)
        assert call() == status, name
        assert (out == 7.0).all() and (st == 7.0).all(), name   # nothing was written
        assert a.get_bus_return(0) == pair and pair[0] != pair[1]
        for x, y in zip(meters, a.meters()):
            assert_bits_equal_finite(y, x, name + ": the meters")
        assert_bits_equal_finite(a.bus_reverb_history(0), hist, name + ": the history")
        _events((a, b), V, fill + 1)
        _mfill(a, b, mm, 64, 2, "after the refusal: " + name)
    # a begun fill in flight
    mm.ret((a,), 1, 0.5)
    a.sample_begin(64, SR)
    assert L.s2r_fill_master(h, op, sp, st.size, 2, 64, SR) == s2s.S2R_ERR_INVALID
    assert (out == 7.0).all() and a.get_bus_return(1) == (0.5, 1.0)
    b.sample(np.empty(64, dtype=F), SR)
    a.sample_end(np.empty(64, dtype=F))
    _events((a, b), V, 7)
    _mfill(a, b, mm, 64, 2, "after the fill in flight")
    mm.check_committed(a)
    # a device list refuses every handle entry and renders on
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    one = s2.Synth(512, max_frames=64, mix_groups=2)
    for syn in (multi, one):
        for v in range(512):
            syn.note_on(36 + v % 61)
    f, n = C.c_float(), C.c_uint32()
    M, mh = multi.L, multi.h
    assert M.s2r_set_bus_return(mh, 0, 0.5) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_bus_return(mh, 0, C.byref(f), None) == s2s.S2R_ERR_INVALID
    assert M.s2r_set_master_fader(mh, 0.5) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_master_fader(mh, C.byref(f), None) == s2s.S2R_ERR_INVALID
    assert M.s2r_snap_master(mh) == s2s.S2R_ERR_INVALID
    assert M.s2r_fill_master(mh, op, sp, st.size, 2, 64, SR) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_meters(mh, C.byref(n), op, op, 18) == s2s.S2R_ERR_INVALID
    assert M.s2r_set_bus_return(mh, 0, 1.5) == s2s.S2R_ERR_PATCH_RANGE                # the values are looked at first
    with pytest.raises(s2.S2rError) as err:
        multi.sample_master(64, SR, 2)
    assert err.value.status == s2s.S2R_ERR_INVALID
    x, y = multi.sample(np.empty(64, dtype=F), SR), one.sample(np.empty(64, dtype=F), SR)
    assert np.abs(y).max() > 0.0
    assert_bits_equal_finite(x, y, "the device-list handle after the refused master calls")
    # an exchange attached: the setters are taken, the fill is refused like the bus fill
    xg = s2.Synth(V, max_frames=64, block_voices=64)
    xg.exchange_create(1)
    xg.set_bus_return(0, 0.5)
    xg.set_master_fader(0.5)
    xg.snap_master()
    assert xg.get_bus_return(0) == (0.5, 0.5) and xg.get_master_fader() == (0.5, 0.5)
    assert xg.L.s2r_fill_buses(xg.h, sp, st.size, 2, 64, SR) == s2s.S2R_ERR_INVALID
    assert xg.L.s2r_fill_master(xg.h, op, sp, st.size, 2, 64, SR) == s2s.S2R_ERR_INVALID
    assert xg.L.s2r_fill_master(xg.h, op, None, 0, 2, 64, SR) == s2s.S2R_ERR_INVALID
    assert (out == 7.0).all() and (st == 7.0).all()


def test_range_checks_on_a_handle():
    check_ranges(s2.Synth(8, max_frames=64))
