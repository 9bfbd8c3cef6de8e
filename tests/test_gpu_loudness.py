"""The loudness and true-peak meters on the device.  Twin handles are fed the same events, one with the meter and one
without: the twin's sample_master gives the stems and the master, which the metered handle must return in the same bits, and the
expectation for the hop rows, the state and the true peak is s2r_loudness_reference over the twin's output, with state, position and
rows carried from call to call in numpy (tests/test_loudness_host.py holds that function to a numpy model of the rule).

Handles, events and the one-pole bank are tests/test_gpu_reverb.py's on 32-voice pools, max_frames 1024 or 2048.  Every comparison is
on bits with no NaN allowance.  The kernel stages tiles of T = 256 frames for its walk and runs one true-peak workgroup per 256 frames,
so its edges are calls of a multiple of 256 frames, plus and minus one; it does not group tiles."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_gpu_buses import ubits
from test_gpu_panned import ON
from test_gpu_reverb import SR, _bank, _events, _handles, _ir

pytestmark = pytest.mark.gpu
F = np.float32
V = 32
T = 256                                                          # S2R_LOUDNESS_TILE and S2R_LOUDNESS_BLOCK
MASTER = s2.MAX_BUSES
BLOCK = 8                                                        # frames a walker takes at a time (s2r_loudness.hip: kLdBlock)
# the parity matrix: the frames of its calls, and the (n_buses, hop) it runs them at.  Hop 17 is there for the walkers' fast path: a
# block of eight frames runs without a hop test when hop - pos > 8, and over CALLS hop 17 starts a block at every distance from 1 to
# 9 — 8, where the hop ends on the block's last frame and `>` and `>=` part, among them; the hops 16, 48, 100 and 4800 never meet 8
# (tests/test_loudness_host.py asserts both through walker_distances).  (8, 16) feeds all 18 walker lanes at the smallest hop.
CALLS = (1, 2, 3, 4, 5, T - 1, T, T + 1, 1023, 1024, 2047, 2048)
PARITY = ((1, 16), (2, 48), (3, 100), (8, 4800), (8, 17), (8, 16))


def walker_distances(hop, calls, pos=0):
    """the schedule of the kernel's walkers (s2r_loudness.hip, workgroup 0) replayed on the books, no arithmetic on samples: a call is
    walked in tiles of T frames, a tile in full blocks of BLOCK frames and then a tail of fewer, frame by frame; `pos`, the frames into
    the hop, is carried from call to call.  -> (the set of hop - pos met at the start of a full block, the number of full blocks, pos)"""
    met, blocks = set(), 0
    for n in calls:
        for t0 in range(0, n, T):
            cnt = min(T, n - t0)
            full = cnt // BLOCK
            for _ in range(full):
                met.add(hop - pos)
                pos = (pos + BLOCK) % hop                        # (hop >= 16: at most one hop ends inside a block)
            blocks += full
            pos = (pos + cnt - full * BLOCK) % hop
    return met, blocks, pos


class Meter:
    """the meter of a handle in numpy: parameters, the carried state and position, the window of hop rows and the held true peak"""

    def __init__(self, hop, max_hops=32, coeffs=None):
        self.hop, self.max_hops = hop, max_hops
        self.c = s2.loudness_design(SR) if coeffs is None else np.asarray(coeffs, dtype=F)
        self.reset()

    def reset(self):
        self.state, self.pos = np.zeros(s2.LOUDNESS_STATE, dtype=F), 0
        self.rows = np.zeros((0, s2.LOUDNESS_CHANNELS), dtype=F)
        self.last, self.held = np.zeros(2, dtype=F), np.zeros(2, dtype=F)
        self.made = 0                                            # hop rows since the reset, dropped ones included

    def set(self, *handles):
        for syn in handles:
            syn.set_master_loudness(SR, self.hop, self.max_hops, self.c)
            c, hop, max_hops, n = syn.get_master_loudness()
            assert_bits_equal_finite(c, self.c.reshape(2, 5), "the coefficients read back")
            assert (hop, max_hops, n) == (self.hop, self.max_hops, 0)
        self.reset()

    def expect(self, stems, x):
        rows, self.state, self.pos, self.last = s2.loudness_reference(self.c, self.hop, stems, x, self.state, self.pos)
        assert np.isfinite(rows).all() and np.isfinite(self.state).all()
        self.made += len(rows)
        self.rows = np.concatenate([self.rows, rows])[-self.max_hops:]
        self.held = np.maximum(self.held, self.last)

    def check(self, syn, what, state=False):
        assert syn.get_master_loudness()[3] == len(self.rows), what
        assert_bits_equal_finite(syn.loudness_hops(), self.rows, what + ": hop rows")
        last, held = syn.true_peak()
        assert_bits_equal_finite(last, self.last, what + ": true peak of the call")
        assert_bits_equal_finite(held, self.held, what + ": true peak held")
        if state:                                                # (a read fetches the state, and the next fill sends it back: not after every call)
            st, pos = syn.loudness_state()
            assert pos == self.pos, what
            assert_bits_equal_finite(st, self.state, what + ": state")


def _mfill(a, b, m, n, nb, what, stems=True, state=False):
    """one call on both handles: the metered handle returns the twin's bits, and its rows, true peak and (on request) state are the
    reference's over the twin's stems and master"""
    x, st_b = b.sample_master(n, SR, nb)
    assert np.isfinite(x).all() and np.isfinite(st_b).all()
    m.expect(st_b, x)
    got, st = a.sample_master(n, SR, nb, stems=stems)
    assert_bits_equal_finite(got, x, what + ": master")
    if stems:
        assert_bits_equal_finite(st, st_b, what + ": stems")
    else:
        assert st is None
    for g, w, name in zip(a.meters(), b.meters(), ("peaks", "energies")):
        assert_bits_equal_finite(g, w, what + ": master section " + name)
    m.check(a, what, state)
    return x, st_b


def _to_hop_edge(a, b, m, delta, nb, max_frames, what, fill):
    """calls until the next one can end `delta` frames past the end of a hop, then that call"""
    while True:
        left = m.hop - m.pos + delta
        if left <= 0:
            left += m.hop
        n = min(left, max_frames)
        _events((a, b), V, fill)
        _mfill(a, b, m, n, nb, "%s: %d frames towards a hop's end %+d" % (what, n, delta), stems=fill % 2 == 0)
        fill += 1
        if n == left:
            assert m.pos == delta % m.hop
            return fill


def _ceiling(fraction):
    """a ceiling the limiter has to work for: that fraction of the peak of a twin's first 1024 frames"""
    b = _handles(V, max_frames=1024)[1]
    _events((b,), V, 0)
    peak = float(np.abs(b.sample_master(1024, SR, 8)[0]).max())
    assert peak > 2.0 ** -10
    return peak * fraction


@pytest.mark.parametrize("limiter", [False, True])
def test_output_is_unchanged_and_rows_follow_the_reference(limiter):
    """master and stems of the metered handle are the twin's bits, with and without a limiter on both, with and without stems; eight
    buses, hop 48"""
    a, b = _handles(V, max_frames=1024)
    ceiling = _ceiling(0.25) if limiter else None
    if limiter:
        for syn in (a, b):
            syn.set_master_limiter(ceiling, 48, 100)
    m = Meter(48)
    m.set(a)
    xs = []
    for fill, n in enumerate([300, 1024, 17, 256, 1000]):
        _events((a, b), V, fill)
        xs.append(_mfill(a, b, m, n, 8, "limiter %s, fill %d of %d frames" % (limiter, fill, n), stems=fill % 2 == 0, state=fill in (1, 4))[0])
    x = np.concatenate(xs)
    assert ubits(x).any() and m.made >= 32 and (m.rows[:, 2 * MASTER:] > 0.0).all()
    if limiter:
        assert a.limiter_meters()[0] < 1.0 and np.abs(x).max() <= F(ceiling)


@pytest.mark.parametrize("nb,hop", PARITY)
def test_rows_state_and_true_peak_are_the_reference(nb, hop):
    """the parity matrix, max_frames 2048: CALLS — calls of 1 to 5 frames, of T - 1, T and T + 1, of 1023, 1024, 2047 and 2048
    frames —, then calls that end exactly on a hop, one frame before one and one frame after one; events between the calls, every
    other call without stems, the state compared after the short calls, the tile edges and at the end.  With eight buses at hops 17
    and 16 every walker lane is fed while a hop ends inside most blocks, at hop 17 on a block's last frame too (walker_distances)"""
    a, b = _handles(V, max_frames=2048)
    m = Meter(hop)
    m.set(a)
    what = "%d buses, hop %d" % (nb, hop)
    calls = list(CALLS)
    for fill, n in enumerate(calls):
        _events((a, b), V, fill)
        _mfill(a, b, m, n, nb, "%s, fill %d of %d frames" % (what, fill, n), stems=fill % 2 == 0, state=fill in (4, 7))
    fill = len(calls)
    for delta in (0, -1, 1):
        fill = _to_hop_edge(a, b, m, delta, nb, 2048, what, fill)
    m.check(a, what + ", at the end", state=True)
    assert m.made >= 2
    fed = m.rows[:, :2 * nb]
    assert (fed[-1] > 0.0).all() and not ubits(m.rows[:, 2 * nb:2 * MASTER]).any() and (m.rows[-1, 2 * MASTER:] > 0.0).all()
    assert (m.held > 0.0).all()


def test_denormal_inputs():
    """program levels of 2^-132 and a master fader of 2^-2: stems and master are denormal throughout — asserted on the twin — and so
    are the filters' values; rows, state and true peak are the reference's bits"""
    a, b = _handles(V, max_frames=1024)
    for syn in (a, b):
        for p in range(8):
            syn.set_program_mix(p, 2.0 ** -132, 0.0, p % 3)
        syn.set_master_fader(0.25)
        syn.snap_master()
    m = Meter(48)
    m.set(a)
    tiny = float(np.finfo(F).tiny)
    for fill, n in enumerate([300, 257, 5]):
        _events((a, b), V, fill)
        x, st = _mfill(a, b, m, n, 3, "denormal inputs, fill %d" % fill, state=True)
        assert ubits(x).any() and np.abs(x).max() < tiny and ubits(st).any() and np.abs(st).max() < tiny
    filt = m.state[:72]
    assert ((filt != 0.0) & (np.abs(filt) < tiny)).any()
    assert (m.last > 0.0).all() and (m.last < tiny).all()


def _timed(handles, fill, frames):
    ev = [(ON, 50 + fill + 7 * k, f, v) for k, (f, v) in enumerate(zip(frames, (0.6, 1.0)))]
    for syn in handles if ev else ():
        syn.note_events(np.array(ev, dtype=s2.NOTE_EVENT_DTYPE))


def test_bus_stages_in_front_events_slices_and_a_changing_bus_count(monkeypatch):
    """an EQ on bus 0, a delay on bus 1 and a reverb on bus 2 of both handles, timed note_ons inside the calls, a rows buffer of 48
    frames so that the stems arrive in slices, returns and the master fader on their way, and n_buses 3, 8, 1, 2, 8 from call to call
    on one handle: a bus past the call's is fed zeros, and its row entries show it"""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    a, b = _handles(V, max_frames=2048)
    for syn in (a, b):
        syn.set_bus_eq(0, np.stack([s2.eq_design(s2.EQ_PEAK, 900.0, 6.0, 1.0, SR)]))
        syn.set_bus_delay(1, 333, 0.4, 0.2, 0.8, 0.6)
        syn.set_bus_reverb(2, _ir(300, 23, True), 0.25, 1.0)
    m = Meter(100)
    m.set(a)
    for fill, (n, nb) in enumerate([(1024, 3), (1025, 8), (2048, 1), (7, 2), (1031, 8)]):
        _events((a, b), V, fill)
        _timed((a, b), fill, [f for f in (1008, 1024) if f < n])
        for syn in (a, b):
            syn.set_bus_return(0, [0.25, 1.0, 0.5, 0.0, 0.75][fill])
            syn.set_master_fader([0.7, 1.0, 0.85, 0.5, 1.0][fill])
        before = m.made
        _mfill(a, b, m, n, nb, "stages in front, fill %d of %d frames on %d buses" % (fill, n, nb), stems=fill % 2 == 1, state=fill == 2)
        new = m.rows[len(m.rows) - min(m.made - before, len(m.rows)):]
        if fill == 2:                                            # one bus for 2048 frames: buses 1 .. 7 decay on zeros, bus 0 is fed
            assert len(new) >= 20 and (new[:, :2] > 0.0).all()
            assert (new[-1, 2:6] < new[0, 2:6]).all()
    a.L.s2r_debug_pan_slice.restype = C.c_uint32
    a.L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    assert a.L.s2r_debug_pan_slice(a.h) == 48


def test_checkpoint_in_the_middle_of_a_hop():
    """voices, pans, mix, sends and the meter — parameters, state and position in the middle of a hop, the stored rows — into a fresh
    handle: the continuations are equal on bits, equal to the reference, and read the same loudness"""
    a, b = _handles(V, max_frames=512)
    m = Meter(100, 32)
    m.set(a)
    for fill, n in enumerate([400, 512, 333]):
        _events((a, b), V, fill)
        _mfill(a, b, m, n, 4, "before the checkpoint, fill %d" % fill)
    st, pos = a.loudness_state()
    rows = a.loudness_hops()
    assert pos == 45 and len(rows) == 12 and ubits(st[72:90]).any()
    c_, hop, max_hops, _ = a.get_master_loudness()
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    c = s2.Synth(V, max_frames=512, block_voices=64)
    c.set_patch_bank(_bank())
    c.import_state(state)
    c.set_voice_pans(pans)
    c.set_voice_mix(gains, buses)
    c.set_voice_sends(sends, sbuses)
    c.set_master_loudness(SR, hop, max_hops, c_)
    c.set_loudness_state(st, pos)
    c.set_loudness_hops(rows)
    got_st, got_pos = c.loudness_state()
    assert got_pos == pos
    assert_bits_equal_finite(got_st, st, "the restored state read back")
    assert_bits_equal_finite(c.loudness_hops(), rows, "the restored rows read back")
    for k, n in enumerate([100, 512, 512, 512, 512, 400]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        x, _ = _mfill(a, b, m, n, 4, "the checkpointed handle, fill %d" % k, state=k == 5)
        assert_bits_equal_finite(c.sample_master(n, SR, 4)[0], x, "the resumed handle, fill %d" % k)
        assert_bits_equal_finite(c.loudness_hops(), m.rows, "the resumed handle's rows, fill %d" % k)
    for p in (0, 3, MASTER):
        assert c.loudness(p) == a.loudness(p) == s2.loudness_readings(m.rows, m.hop, p)
    assert m.made > 32 and len(m.rows) == 32                     # the window was reached
    lm, ls, li = a.loudness(MASTER)
    assert np.isfinite([lm, ls, li]).all()
    # the held true peak is no part of the checkpoint: the resumed handle holds the maximum since it was set
    assert (c.true_peak()[1] <= a.true_peak()[1]).all()


def test_reset_and_clear():
    """reset: state, rows and held true peak as after a set, the parameters kept — the next fill equals the reference from the initial
    state.  clear: off, the handle's fills equal the twin's, every entry that needs a meter refuses, and a bus fill or a panned fill
    between two master fills moves nothing."""
    a, b = _handles(V, max_frames=1024)
    m = Meter(48)
    m.set(a)
    for fill, n in enumerate([500, 333]):
        _events((a, b), V, fill)
        _mfill(a, b, m, n, 8, "before the reset, fill %d" % fill)
    before = (a.loudness_hops(), a.loudness_state(), a.true_peak())
    _events((a, b), V, 10)
    assert_bits_equal_finite(a.sample_buses(64, SR, 8), b.sample_buses(64, SR, 8), "a bus fill beside the meter")
    assert_bits_equal_finite(a.sample_panned(64, SR), b.sample_panned(64, SR), "a panned fill beside the meter")
    assert_bits_equal_finite(a.loudness_hops(), before[0], "rows after other fills")
    assert_bits_equal_finite(a.loudness_state()[0], before[1][0], "state after other fills")
    assert a.loudness_state()[1] == before[1][1]
    a.reset_master_loudness()
    m.reset()
    assert a.get_master_loudness()[1:] == (48, 32, 0)
    st, pos = a.loudness_state()
    assert pos == 0 and not ubits(st).any() and not ubits(np.concatenate(a.true_peak())).any()
    assert a.loudness(MASTER) == (-np.inf, -np.inf, -np.inf)
    _events((a, b), V, 2)
    _mfill(a, b, m, 700, 8, "after the reset", state=True)
    a.clear_master_loudness()
    assert a.get_master_loudness()[1:] == (0, 0, 0)
    _events((a, b), V, 3)
    x, st_b = b.sample_master(300, SR, 8)
    got, st = a.sample_master(300, SR, 8)
    assert_bits_equal_finite(got, x, "after clear_master_loudness: master")
    assert_bits_equal_finite(st, st_b, "after clear_master_loudness: stems")
    for call in (a.loudness_state, a.loudness_hops, a.true_peak, a.reset_master_loudness, lambda: a.loudness(0)):
        with pytest.raises(s2.S2rError) as e:
            call()
        assert e.value.status == s2s.S2R_ERR_INVALID
    m.set(a)                                                     # off, then on: the initial state
    _events((a, b), V, 4)
    _mfill(a, b, m, 300, 8, "set again", state=True)


def test_refusals_change_nothing():
    """refused master fills and refused setters leave parameters, state, rows, readings and true peak as they were, and the next
    fill equals the reference as if they had not happened; a device-list handle refuses every entry"""
    a, b = _handles(V, max_frames=256)
    m = Meter(16, 30)
    m.set(a)
    for fill in range(3):
        _events((a, b), V, fill)
        _mfill(a, b, m, 250, 2, "before the refusals, fill %d" % fill)
    L, h = a.L, a.h
    out, st = np.full(2 * 300, 7.0, dtype=F), np.full(2 * 2 * 300, 7.0, dtype=F)
    op, sp = out.ctypes.data_as(s2s._f32p), st.ctypes.data_as(s2s._f32p)
    good = np.ascontiguousarray(m.c, dtype=F).reshape(-1)
    gp = good.ctypes.data_as(s2s._f32p)
    nan = good.copy(); nan[3] = np.nan
    inf = good.copy(); inf[9] = np.inf
    state0, pos0 = a.loudness_state()
    zeros = np.zeros(18 * 31, dtype=F)
    zp = zeros.ctypes.data_as(s2s._f32p)
    refusals = [
        ("no bus", lambda: L.s2r_fill_master(h, op, sp, st.size, 0, 64, SR), s2s.S2R_ERR_INVALID),
        ("nine buses", lambda: L.s2r_fill_master(h, op, sp, st.size, 9, 64, SR), s2s.S2R_ERR_INVALID),
        ("short stems", lambda: L.s2r_fill_master(h, op, sp, 2 * 2 * 64 - 1, 2, 64, SR), s2s.S2R_ERR_INVALID),
        ("null master", lambda: L.s2r_fill_master(h, None, sp, st.size, 2, 64, SR), s2s.S2R_ERR_INVALID),
        ("too many frames", lambda: L.s2r_fill_master(h, op, sp, st.size, 2, 257, SR), s2s.S2R_ERR_TOO_MANY_FRAMES),
        ("hop 15", lambda: L.s2r_set_master_loudness(h, gp, 15, 30), s2s.S2R_ERR_PATCH_RANGE),
        ("hop past the range", lambda: L.s2r_set_master_loudness(h, gp, (1 << 20) + 1, 30), s2s.S2R_ERR_PATCH_RANGE),
        ("29 hops", lambda: L.s2r_set_master_loudness(h, gp, 16, 29), s2s.S2R_ERR_PATCH_RANGE),
        ("hops past the range", lambda: L.s2r_set_master_loudness(h, gp, 16, (1 << 18) + 1), s2s.S2R_ERR_PATCH_RANGE),
        ("a NaN", lambda: L.s2r_set_master_loudness(h, nan.ctypes.data_as(s2s._f32p), 16, 30), s2s.S2R_ERR_PATCH_RANGE),
        ("an infinity", lambda: L.s2r_set_master_loudness(h, inf.ctypes.data_as(s2s._f32p), 16, 30), s2s.S2R_ERR_PATCH_RANGE),
        ("null coefficients", lambda: L.s2r_set_master_loudness(h, None, 16, 30), s2s.S2R_ERR_INVALID),
        ("a short state", lambda: L.s2r_set_loudness_state(h, zp, 121, 0), s2s.S2R_ERR_INVALID),
        ("a long state", lambda: L.s2r_set_loudness_state(h, zp, 123, 0), s2s.S2R_ERR_INVALID),
        ("a null state", lambda: L.s2r_set_loudness_state(h, None, 122, 0), s2s.S2R_ERR_INVALID),
        ("a position at the hop", lambda: L.s2r_set_loudness_state(h, zp, 122, 16), s2s.S2R_ERR_PATCH_RANGE),
        ("rows of the wrong size", lambda: L.s2r_set_loudness_hops(h, zp, 2, 35), s2s.S2R_ERR_INVALID),
        ("null rows", lambda: L.s2r_set_loudness_hops(h, None, 2, 36), s2s.S2R_ERR_INVALID),
        ("rows past the window", lambda: L.s2r_set_loudness_hops(h, zp, 31, 18 * 31), s2s.S2R_ERR_PATCH_RANGE),
        ("a small state buffer", lambda: L.s2r_get_loudness_state(h, zp, 121, None), s2s.S2R_ERR_INVALID),
        ("a small rows buffer", lambda: L.s2r_get_loudness_hops(h, zp, 18 * 30 - 1, None), s2s.S2R_ERR_INVALID),
        ("programme 9", lambda: L.s2r_get_loudness(h, 9, (C.c_double * 3)()), s2s.S2R_ERR_PATCH_RANGE),
    ]
    assert len(m.rows) == 30
    for fill, (name, call, status) in enumerate(refusals):
        readings = a.loudness(MASTER)
        assert call() == status, name
        assert (out == 7.0).all() and (st == 7.0).all() and not zeros.any(), name
        m.check(a, name, state=True)
        assert a.loudness(MASTER) == readings, name
        assert a.get_master_loudness()[1:] == (16, 30, 30), name
        if fill % 4 == 0:
            _events((a, b), V, fill + 3)
            _mfill(a, b, m, 64, 2, "after the refusal: " + name)
    a.sample_begin(64, SR)
    assert L.s2r_fill_master(h, op, sp, st.size, 2, 64, SR) == s2s.S2R_ERR_INVALID
    assert (out == 7.0).all()
    b.sample(np.empty(64, dtype=F), SR)
    a.sample_end(np.empty(64, dtype=F))
    _events((a, b), V, 40)
    _mfill(a, b, m, 64, 2, "after the fill in flight", state=True)
    # a device list refuses every entry
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    M, mh = multi.L, multi.h
    u, z, d3 = C.c_uint32(), C.c_size_t(), (C.c_double * 3)()
    assert M.s2r_set_master_loudness(mh, gp, 16, 30) == s2s.S2R_ERR_INVALID
    assert M.s2r_clear_master_loudness(mh) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_master_loudness(mh, zp, C.byref(u), C.byref(u), C.byref(z)) == s2s.S2R_ERR_INVALID
    assert M.s2r_reset_master_loudness(mh) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_loudness(mh, 0, d3) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_true_peak(mh, zp, zp) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_loudness_state(mh, zp, 122, C.byref(u)) == s2s.S2R_ERR_INVALID
    assert M.s2r_set_loudness_state(mh, zp, 122, 0) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_loudness_hops(mh, zp, zeros.size, C.byref(z)) == s2s.S2R_ERR_INVALID
    assert M.s2r_set_loudness_hops(mh, zp, 0, 0) == s2s.S2R_ERR_INVALID
    assert M.s2r_set_master_loudness(mh, gp, 15, 30) == s2s.S2R_ERR_PATCH_RANGE            # the values are looked at first
    assert not zeros.any()


def test_a_long_run_cut_two_ways_reads_the_same():
    """three metered handles render the same 12 288 frames in calls of 1024, of 1008, 16, 272 and 752, and of 16 and 2032 frames (every
    cut at a multiple of 16 frames, where a split fill renders the same bits: the masters are compared first): rows, state and the
    momentary, short-term and integrated readings of every programme are the same bits; 122 hops of 100 frames"""
    hs = _handles(V, max_frames=2048, n=3)
    cuts = ([1024] * 12, [1008, 16, 272, 752] * 6, [16, 2032] * 6)
    masters = []
    for syn, cut in zip(hs, cuts):
        syn.set_master_loudness(SR, 100, 200)
        _events((syn,), V, 0)
        assert sum(cut) == 12288
        masters.append(np.concatenate([syn.sample_master(n, SR, 8, stems=False)[0] for n in cut]))
    rows = hs[0].loudness_hops()
    assert len(rows) == 122 and (rows > 0.0).all()
    for syn, x in zip(hs[1:], masters[1:]):
        assert_bits_equal_finite(x, masters[0], "the master, another cut")
        assert_bits_equal_finite(syn.loudness_hops(), rows, "rows, another cut")
        assert_bits_equal_finite(syn.loudness_state()[0], hs[0].loudness_state()[0], "state, another cut")
        assert syn.loudness_state()[1] == hs[0].loudness_state()[1] == 88
        assert_bits_equal_finite(syn.true_peak()[1], hs[0].true_peak()[1], "held true peak, another cut")
    for p in range(s2.LOUDNESS_PROGRAMMES):
        r = hs[0].loudness(p)
        assert np.isfinite(r).all(), (p, r)
        assert hs[1].loudness(p) == r and hs[2].loudness(p) == r
        assert r == s2.loudness_readings(rows, 100, p)
    print("master: momentary %.3f, short-term %.3f, integrated %.3f LKFS" % hs[0].loudness(MASTER))


def test_true_peak_under_a_limiter_that_holds_its_ceiling():
    """a limiter at ceiling C on a signal that it holds: no sample exceeds C, and the true peak is at least the master's sample peak —
    it is a maximum over the samples and the interpolated values between them"""
    ceiling = _ceiling(0.25)
    a, b = _handles(V, max_frames=1024)
    for syn in (a, b):
        syn.set_master_limiter(ceiling, 48, 100)
    m = Meter(4800)
    m.set(a)
    xs = []
    for fill in range(4):
        _events((a, b), V, fill)
        xs.append(_mfill(a, b, m, 1024, 8, "limited, fill %d" % fill, stems=False)[0])
    x = np.concatenate(xs)
    sample_peak = np.abs(x).max(axis=0)
    last, held = a.true_peak()
    print("ceiling %.6f: sample peak L %.6f R %.6f, true peak L %.6f R %.6f" % (ceiling, sample_peak[0], sample_peak[1], held[0], held[1]))
    assert a.limiter_meters()[0] < 1.0 and (sample_peak <= F(ceiling)).all()
    assert (held >= sample_peak).all() and (last <= held).all()


def test_timing_entry():
    """s2r_debug_loudness_ms: -1 without s2r_set_timing; under it the loudness kernel's time of the last master fill, 0 when that
    fill ran none"""
    a = _handles(V)[0]
    ms = a.L.s2r_debug_loudness_ms
    ms.restype, ms.argtypes = C.c_float, [C.c_void_p]
    _events((a,), V, 0)
    a.set_master_loudness(SR, 4800, 32)
    a.sample_master(300, SR, 2)
    assert ms(a.h) == -1.0
    a.set_timing(True)
    a.sample_master(300, SR, 2)
    assert 0.0 < ms(a.h) < 100.0
    a.clear_master_loudness()
    a.sample_master(300, SR, 2)
    assert ms(a.h) == 0.0
