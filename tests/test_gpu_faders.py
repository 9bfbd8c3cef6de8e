"""Live program faders on the device: s2r_fill_buses under moving faders bit for bit against the oracle's rows
times the [voices, frames] gain matrix of the ramp rule, built in numpy float32 from a model of every program's applied and
target pair and of the program every voice was started with, through s2o.mix_tree per bus and channel — and, without any
oracle, against a twin handle whose faders stand still.

Every mix is non-degenerate: seeds[v] = v, noise > 0, notes 36 + v % 61.  Every comparison is on bits with no NaN allowance
(helpers.assert_bits_equal_finite)."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
from oracle import s2o
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_fader_host import check_ranges, np_fader_gains
from test_gpu_buses import BusTwin, SETTINGS, VELS, _drive, _pair, _play, ubits
from test_gpu_panned import _bank2, ON, OFF, PROGRAM

pytestmark = pytest.mark.gpu
SR = 48000
F = np.float32
DEFAULT = (1.0, 0.0)
POOLS = [(8, 0, 0), (17, 0, 0), (272, 64, 0), (1088, 64, 2)]
BUS_COUNTS = [1, 2, 3, 8]
# the issue's fader walk: the state in front of fills of 1000, 1, 16, 17 and 1000 frames (the last one: no move, away from the default)
WALK = [(1.0, 0.0), (1.0 / 3.0, -0.25), (0.0, 2.0), (0.7, -2.0), (0.7, -2.0)]
LENGTHS = [1000, 1, 16, 17, 1000]


class FaderTwin(BusTwin):
    """test_gpu_buses.BusTwin with the model of the faders: target and applied pair per program, and the program every pool
    voice was started with (a voice never started: 0)."""

    def __init__(self, voices, **kw):
        super().__init__(voices, **kw)
        self.vprog = np.zeros(voices, dtype=np.int64)
        self.target, self.applied = {}, {}
        self.n_prog = 256

    def set_program_fader(self, program, fader, shift):
        self.target[program] = (fader, shift)
        for g in self.gpus:
            g.set_program_fader(program, fader, shift)

    def snap(self):
        self.applied = dict(self.target)
        for g in self.gpus:
            g.snap_program_faders()

    def commit(self):
        self.applied = dict(self.target)

    def moving(self):
        return any(self.target.get(p, DEFAULT) != self.applied.get(p, DEFAULT) for p in self.target)

    def _cpu_on(self, note, velocity=1.0):
        v = super()._cpu_on(note, velocity)
        self.vprog[v] = self.program
        return v

    def _pairs(self, which, idx):
        tab = np.array([which.get(p, DEFAULT) for p in range(self.n_prog)], dtype=F)
        return tab[self.vprog[idx], 0], tab[self.vprog[idx], 1]

    def ramp(self, k, n_call, ramp=True):
        """(G0_L, G0_R, d_L, d_R) of handle k's voices for a call of n_call frames; ramp=False: d = 0 (the static gains under
        the applied pairs)"""
        idx = self.idx[k]
        g0 = np_fader_gains(self.pans[idx], self.gains[idx], *self._pairs(self.applied, idx))
        g1 = np_fader_gains(self.pans[idx], self.gains[idx], *self._pairs(self.target if ramp else self.applied, idx))
        with np.errstate(under="ignore"):
            d = [((b - a).astype(F) / F(n_call)).astype(F) for a, b in zip(g0, g1)]
        return g0[0], g0[1], d[0], d[1]

    def want_faded(self, pv, n_buses, k=0, i0=0, n_call=None, ramp=True, only_bus=None):
        """[n_buses, frames, 2] for frames [i0, i0 + pv.shape[1]) of a call of n_call frames: the tree over rows * gb_c with
        g_c[v][i] = G0_c + (float)i * d_c, the product rounded, then the sum"""
        frames = pv.shape[1]
        n_call = frames if n_call is None else n_call
        idx = self.idx[k]
        rows = pv[idx]
        fold = np.minimum(self.buses[idx], n_buses - 1)
        g0l, g0r, dl, dr = self.ramp(k, n_call, ramp)
        i = np.arange(i0, i0 + frames).astype(F)
        out = np.zeros((n_buses, frames, 2), dtype=F)
        with np.errstate(under="ignore"):
            for c, (g0, d) in enumerate(((g0l, dl), (g0r, dr))):
                g = (g0[:, None] + (i[None, :] * d[:, None]).astype(F)).astype(F)
                for b in range(n_buses) if only_bus is None else [only_bus]:
                    gb = np.where((fold == b)[:, None], g, F(0.0)).astype(F)      # off the bus: +0.0, not a skipped term
                    out[b, :, c] = s2o.mix_tree((rows * gb).astype(F), self.block, self.groups)
        return out

    def assert_ramp_is_not_degenerate(self, pv, n_buses, k, want, what):
        """a ramped fill: some bus differs in bits from the expectation with d = 0, and a sounding voice stands still"""
        g0l, g0r, dl, dr = self.ramp(k, pv.shape[1])
        sounding = ubits(pv[self.idx[k]]).any(axis=1)
        assert (sounding & (dl == 0.0) & (dr == 0.0)).any(), "%s: no sounding voice with d == 0" % what
        assert (sounding & ((dl != 0.0) | (dr != 0.0))).any(), "%s: no sounding voice moves" % what
        for b in range(n_buses):
            still = self.want_faded(pv, n_buses, k, ramp=False, only_bus=b)
            if not np.array_equal(ubits(still[b]), ubits(want[b])):
                return
        raise AssertionError("%s: the ramp changes no bit of any bus" % what)

    def check_bus_fill(self, frames, n_buses, what):
        """BusTwin.check_bus_fill under the faders: ramped where a target differs from its applied pair; commits.  A ramped
        fill must not be degenerate — except one of a single frame, which cannot differ from d = 0: its only frame is i = 0,
        where g = G0 + 0 * d = G0 whatever d is (what such a fill does is commit: the next one starts from the new pair)."""
        pv = self.rows(frames)
        assert np.isfinite(pv).all()
        moving = self.moving()
        for k, (g, nb) in enumerate(zip(self.gpus, n_buses)):
            want = self.want_faded(pv, nb, k)
            if moving and frames > 1:
                self.assert_ramp_is_not_degenerate(pv, nb, k, want, what)
            elif moving:
                assert np.array_equal(ubits(want), ubits(self.want_faded(pv, nb, k, ramp=False))), what
            got = g.sample_buses(frames, SR, nb)
            assert_bits_equal_finite(got, want, "%s, handle %d, %d buses, %d frames" % (what, k, nb, frames))
        self.commit()
        self.check_faders(what)
        return pv

    def check_faders(self, what):
        for g in self.gpus:
            for p in self.target:
                want = self.target[p] + self.applied.get(p, DEFAULT)
                assert np.array_equal(ubits(g.get_program_fader(p)), ubits(want)), (what, p)


def _between(tw, b, programs):
    """what happens between two fills: note_offs, restarts under further settings (test_gpu_buses._drive's later stages), and
    one voice started at velocity 0 under full sensitivity — gain +0.0, so that it stands still under every fader"""
    if b == 1:
        for note in range(36, 97, 3):
            tw.note_off(note)
    else:
        if programs >= 2:
            tw.program_change((b + 1) % programs)
        tw.setting(b - 2)
        for k in range(min(tw.V // 2, 5 + 2 * b)):
            tw.note_on(40 + (7 * k + b) % 50, VELS[(k + b) % 4])
        tw.note_off(40 + b % 50)
    assert SETTINGS[2][:2] == (1.0 / 3.0, 1.0)
    tw.setting(2)                                                # level 1/3, sensitivity 1: velocity 0 gives gain +0.0
    tw.note_on(60 + b, 0.0)


@pytest.mark.parametrize("programs", [1, 2])
@pytest.mark.parametrize("voices,block,groups", POOLS)
def test_ramped_bus_fill_is_the_tree_over_the_rows_times_the_gain_matrix(voices, block, groups, programs):
    """the parity matrix: four handles in lockstep, one per bus count (1, 2, 3, 8), the voices set up by _drive's first stage;
    fills of 1000, 1, 16, 17 and 1000 frames with program 0's pair walking (1, 0) -> (1/3, -0.25) -> (0, 2) -> (0.7, -2) ->
    (0.7, -2) in front of them (with two programs the second one moves once, in front of the 16-frame fill): the first fill is
    the default path, the 1-, 16- and 17-frame fills ramp (16: the 16-byte loads), the last one has applied == target away
    from the default — the static kernels on recomputed gains."""
    tw = FaderTwin(voices, handles=len(BUS_COUNTS), max_frames=1024, block=block, groups=groups, bank=_bank2() if programs == 2 else None)
    what = "%d voices, block %d, groups %d, %d programs" % (voices, block, groups, programs)
    for b, n in enumerate(LENGTHS):
        tw.set_program_fader(0, *WALK[b])
        if programs == 2 and b == 2:
            tw.set_program_fader(1, 0.5, 0.25)
        if b == 0:
            _drive(tw, [n], BUS_COUNTS, what, programs)          # every voice started, one default fill (tw.check_bus_fill)
            continue
        _between(tw, b, programs)
        assert tw.moving() == (b < 4)
        tw.check_bus_fill(n, BUS_COUNTS, "%s, fill %d" % (what, b))
    tw.check_mix(what)
    assert tw.gpus[0].get_program_fader(0) == tuple(float(F(x)) for x in WALK[-1] * 2)


def _ramp_setup(tw):
    """272 voices over two programs on eight buses; program 0's fader on its way, program 1's standing away from the default"""
    for v in range(tw.V):
        if v % 34 == 0:
            tw.program_change((v // 34) % 2)
            tw.setting(v // 34)
        tw.note_on(36 + v % 61, VELS[(v + v // 4) % 4])
    tw.set_program_fader(1, 0.5, 0.25)
    tw.snap()
    tw.set_program_fader(0, 0.25, 1.0)
    assert tw.moving()


def test_the_frame_index_counts_from_the_start_of_the_call_across_event_segments():
    """a ramped 1000-frame fill with note_ons and note_offs at frames 16, 400 and 992: the host splits the fill there, and the
    ramp's i runs on through the segments; the note_ons at 16 land on the program whose fader moves, those at 400 on the still
    one.  The expectation is built segment by segment from the oracle."""
    tw = FaderTwin(272, max_frames=1024, block=64, bank=_bank2())
    _ramp_setup(tw)
    frames = 1000
    ev = [(OFF, 40, 0, 0.0), (PROGRAM, 0, 0, 0.0), (ON, 90, 0, 0.25)]
    ev += [(ON, 50, 16, 0.6), (OFF, 36, 16, 0.0), (ON, 77, 16, 1.0)]
    ev += [(OFF, 50, 400, 0.0), (PROGRAM, 1, 400, 0.0)] + [(ON, 60 + k, 400, VELS[(k + 1) % 4]) for k in range(8)] + [(OFF, 61, 400, 0.0)]
    ev += [(PROGRAM, 0, 992, 0.0), (ON, 52, 992, 1.0), (OFF, 77, 992, 0.0)]
    tw.gpus[0].note_events(np.array(ev, dtype=s2.NOTE_EVENT_DTYPE))
    got = tw.gpus[0].sample_buses(frames, SR, 8)
    want = np.zeros((8, frames, 2), dtype=F)
    local = np.zeros((8, frames, 2), dtype=F)                    # the same with i counted from the segment: must differ
    bounds = [0, 16, 400, 992, frames]
    for a, b in zip(bounds[:-1], bounds[1:]):
        for k, n, f, vel in ev:
            if f == a:
                tw.cpu_event(k, n, vel)
        pv = tw.rows(b - a)
        want[:, a:b] = tw.want_faded(pv, 8, i0=a, n_call=frames)
        local[:, a:b] = tw.want_faded(pv, 8, i0=0, n_call=frames)
    assert not np.array_equal(ubits(want[:, 16:]), ubits(local[:, 16:]))
    assert_bits_equal_finite(got, want, "ramp across event segments")
    tw.commit()
    tw.check_faders("after the segmented fill")
    tw.check_mix("after the segmented fill")
    tw.check_bus_fill(64, [8], "the static fill after it")


@pytest.mark.parametrize("frames", [256, 250])
def test_the_first_fader_call_finds_timed_note_ons_waiting(frames):
    """pans and a mix in use, one batch with note_ons at frames 0, 16 and 128 (program 1 from 16, program 0 again from 128) and
    a note_off at 128 — and only then the handle's FIRST fader call: the programs of the note_ons that wait join the pans and
    gains already queued for them.  The voices started at 0 and 128 ramp, those started at 16 stand still.  250 frames: the last
    segment holds 122, a frame per thread; the others take the 16-byte loads.  Segment by segment from the oracle."""
    tw = FaderTwin(272, max_frames=256, block=64, bank=_bank2())
    gpu = tw.gpus[0]
    tw.set_program_pan(0, -0.5, 1.0)
    tw.set_program_pan(1, 0.7, -1.0 / 3.0)
    tw.set_program_mix(0, 0.7, 0.5, 0)
    tw.set_program_mix(1, 1.0, 1.0 / 3.0, 1)
    ev = [(ON, 36 + v % 61, 0, VELS[v % 4]) for v in range(40)]
    ev += [(PROGRAM, 1, 16, 0.0)] + [(ON, 50 + k, 16, VELS[(k + 1) % 4]) for k in range(12)]
    ev += [(PROGRAM, 0, 128, 0.0)] + [(ON, 70 + k, 128, VELS[(k + 2) % 4]) for k in range(9)] + [(OFF, 40, 128, 0.0)]
    gpu.note_events(np.array(ev, dtype=s2.NOTE_EVENT_DTYPE))
    tw.set_program_fader(0, 0.25, 0.5)
    assert tw.moving()
    got = gpu.sample_buses(frames, SR, 2)
    want = np.zeros((2, frames, 2), dtype=F)
    still = np.zeros((2, frames, 2), dtype=F)
    started = {0: [], 16: [], 128: []}
    bounds = [0, 16, 128, frames]
    for a, b in zip(bounds[:-1], bounds[1:]):
        for k, n, f, vel in ev:
            if f == a and k == ON:
                started[a].append(tw._cpu_on(n, vel))
            elif f == a:
                tw.cpu_event(k, n, vel)
        pv = tw.rows(b - a)
        want[:, a:b] = tw.want_faded(pv, 2, i0=a, n_call=frames)
        still[:, a:b] = tw.want_faded(pv, 2, i0=a, n_call=frames, ramp=False)
    assert len(set(sum(started.values(), []))) == 40 + 12 + 9     # nobody took another's voice
    g0l, g0r, dl, dr = tw.ramp(0, frames)
    moves = (dl != 0.0) | (dr != 0.0)
    assert moves[started[0]].all() and moves[started[128]].all() and not moves[started[16]].any()
    assert not np.array_equal(ubits(want[0]), ubits(still[0])) and ubits(want[1]).any()
    assert_bits_equal_finite(got, want, "first fader call over waiting note_ons, %d frames" % frames)
    tw.commit()
    tw.check_faders("after the first fader call")
    tw.check_mix("after the first fader call")
    tw.check_bus_fill(64, [2], "the static fill after it")


def test_the_frame_index_counts_from_the_start_of_the_call_across_slices(monkeypatch):
    """the same ramp on a handle whose rows buffer holds 48 frames: 21 slices, one mixdown launch each"""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    tw = FaderTwin(272, max_frames=1024, block=64, bank=_bank2())
    _ramp_setup(tw)
    gpu = tw.gpus[0]
    pv = tw.rows(1000)
    want = tw.want_faded(pv, 8)
    local = np.concatenate([tw.want_faded(pv[:, a:a + 48], 8, i0=0, n_call=1000) for a in range(0, 1000, 48)], axis=1)
    assert not np.array_equal(ubits(want), ubits(local))
    got = gpu.sample_buses(1000, SR, 8)
    gpu.L.s2r_debug_pan_slice.restype = C.c_uint32
    gpu.L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    assert gpu.L.s2r_debug_pan_slice(gpu.h) == 48
    assert_bits_equal_finite(got, want, "ramp across slices")
    tw.commit()
    tw.check_bus_fill(100, [8], "the static fill after it, sliced")


def test_still_programs_are_untouched_and_a_snapped_half_is_half():
    """no oracle in the loop: two handles fed identically, program 0 on bus 0 and program 1 on bus 1; only the second handle
    moves program 1's fader.  Bus 0 is equal in bits over the ramped fill, bus 1 differs; snapped to fader 0.5, shift 0, bus 1
    of the second handle is 0.5f times the first handle's, bit for bit — a power of two commutes with every rounding while
    nothing it scales is denormal, which a third handle's per-voice rows show (the half-level case's inputs)."""
    voices = 272
    a, b = _pair(voices, 64, bank=_bank2(), max_frames=1024)
    probe = _pair(voices, 64, bank=_bank2(), max_frames=1024)[0]
    for syn in (a, b, probe):
        syn.set_program_pan(0, -0.5, 1.0)
        syn.set_program_pan(1, 0.7, -1.0 / 3.0)
        syn.set_program_mix(0, 0.7, 0.5, 0)
        syn.set_program_mix(1, 1.0, 1.0 / 3.0, 1)
    _play((a, b, probe), voices, 2, 0)
    b.set_program_fader(1, 0.5, 0.0)
    x, y = a.sample_buses(1000, SR, 2), b.sample_buses(1000, SR, 2)
    assert np.isfinite(x).all() and np.abs(x[0]).max() > 0.0 and np.abs(x[1]).max() > 0.0
    assert np.array_equal(ubits(x[0]), ubits(y[0])), "bus 0 holds the still program's voices only"
    assert not np.array_equal(ubits(x[1]), ubits(y[1]))
    assert np.array_equal(ubits(x[1][0]), ubits(y[1][0]))        # frame 0 of the ramp is the applied gain
    probe.render_voices(1000, SR)
    pans = a.voice_pans()
    assert np.abs(pans).max() <= 0.95                            # both pan gains of every voice are above 0.15
    for n in (200, 17):
        _play((a, b, probe), voices, 2, 1 if n == 200 else 2)
        b.set_program_fader(1, 0.25, 1.0)                        # overwritten before any fill sees it
        b.set_program_fader(1, 0.5, 0.0)
        b.snap_program_faders()
        assert b.get_program_fader(1) == (0.5, 0.0, 0.5, 0.0)
        rows = probe.render_voices(n, SR)
        mag = np.abs(rows.astype(np.float64))
        assert not ((mag > 0.0) & (mag < 2.0 ** -90)).any()     # times a gain of at least 2^-8 where it is not 0: no denormal term
        gains, _ = a.voice_mix()
        assert gains[gains > 0.0].min() >= 2.0 ** -5
        x, y = a.sample_buses(n, SR, 2), b.sample_buses(n, SR, 2)
        assert np.abs(x[1]).max() > 0.0
        assert_bits_equal_finite(y[0], x[0], "snapped half, bus 0, %d frames" % n)
        assert_bits_equal_finite(y[1], x[1] * F(0.5), "snapped half, bus 1, %d frames" % n)


def test_default_faders_change_nothing_and_only_the_bus_fill_applies_them():
    """faders set to (1, 0) explicitly against a handle that never called a fader entry: bit-equal bus fills; then faders at
    (0.25, 1): s2r_fill_panned, s2r_fill and s2r_fill_stereo equal those of the handle without faders — and leave the move
    pending"""
    voices = 272
    a, b = _pair(voices, 64, bank=_bank2(), max_frames=512)
    for syn in (a, b):
        syn.set_program_pan(0, -0.5, 1.0)
        syn.set_program_pan(1, 0.7, -1.0 / 3.0)
        syn.set_program_mix(1, 0.7, 0.5, 1)
    for p in range(2):
        a.set_program_fader(p, 1.0, 0.0)
    for fill, n in enumerate([500, 17]):
        _play((a, b), voices, 2, fill)
        x, y = a.sample_buses(n, SR, 2), b.sample_buses(n, SR, 2)
        assert np.abs(y).max() > 0.0
        assert_bits_equal_finite(x, y, "explicit defaults, fill %d" % fill)
    for p in range(2):
        a.set_program_fader(p, 0.25, 1.0)
    _play((a, b), voices, 2, 2)
    assert_bits_equal_finite(a.sample_panned(100, SR), b.sample_panned(100, SR), "panned fill under faders")
    assert_bits_equal_finite(a.sample(np.empty(64, dtype=F), SR), b.sample(np.empty(64, dtype=F), SR), "mono fill under faders")
    assert_bits_equal_finite(a.sample_stereo(33, SR), b.sample_stereo(33, SR), "stereo copy under faders")
    assert a.get_program_fader(0) == (0.25, 1.0, 1.0, 0.0)       # nobody committed anything
    x, y = a.sample_buses(64, SR, 2), b.sample_buses(64, SR, 2)
    assert not np.array_equal(ubits(x), ubits(y))
    assert a.get_program_fader(0) == (0.25, 1.0, 0.25, 1.0) and a.get_program_fader(1) == (0.25, 1.0, 0.25, 1.0)


def test_commit_refusal_and_snap():
    """applied == target after a ramped fill; a fill refused for a buffer one float short leaves applied alone, and the next
    good fill ramps from the old pair; snap followed by a fill is the static expectation.  All against the oracle."""
    tw = FaderTwin(272, max_frames=256, block=64, bank=_bank2())
    gpu = tw.gpus[0]
    _ramp_setup(tw)
    tw.check_bus_fill(100, [3], "first ramp")                    # (check_faders: applied == target)
    assert gpu.get_program_fader(0) == (0.25, 1.0, 0.25, 1.0)
    tw.set_program_fader(0, 0.75, -0.5)
    out = np.full(2 * 64 * 3, 7.0, dtype=F)
    assert gpu.L.s2r_fill_buses(gpu.h, out.ctypes.data_as(s2s._f32p), out.size - 1, 3, 64, SR) == s2s.S2R_ERR_INVALID
    assert (out == 7.0).all() and gpu.get_program_fader(0) == (0.75, -0.5, 0.25, 1.0)
    tw.check_faders("after the refused fill")
    tw.note_off(40)
    tw.check_bus_fill(64, [3], "the ramp after the refused fill")
    tw.set_program_fader(0, 1.0 / 3.0, 0.25)
    tw.set_program_fader(1, 1.0, 0.0)
    tw.snap()
    assert not tw.moving()
    tw.check_faders("after the snap")
    tw.check_bus_fill(48, [3], "the static fill after a snap")


@pytest.mark.parametrize("flushed", [False, True])
def test_a_voice_follows_the_program_it_was_started_with(flushed):
    """voices started on program 0, then program_change(1), then the FIRST fader call of the handle moves program 0: the held
    voices ramp (their programs come from the device — flushed: a fill has applied their note_ons — or from the events the
    host still holds), voices started afterwards on program 1 do not"""
    V = 272
    tw = FaderTwin(V, max_frames=256, block=64, bank=_bank2())
    tw.set_program_pan(0, -0.5, 1.0)
    tw.set_program_pan(1, 0.7, -1.0 / 3.0)
    tw.set_program_mix(1, 0.7, 0.5, 1)
    for v in range(V // 2):
        tw.note_on(36 + v % 61, VELS[v % 4])
    if flushed:
        tw.check_bus_fill(32, [2], "before any fader")
    tw.program_change(1)
    tw.set_program_fader(0, 0.25, 0.5)
    for v in range(V // 2, V - 8):
        tw.note_on(36 + v % 61, VELS[(v + 1) % 4])
    g0l, g0r, dl, dr = tw.ramp(0, 200)
    assert (dl[:V // 2] != 0.0).all() and not dl[V // 2:V - 8].any() and not dr[V // 2:V - 8].any()      # (the last 8 were never started)
    tw.check_bus_fill(200, [2], "program 0 moves after the program change")
    tw.set_program_fader(1, 0.5, -1.0)
    tw.check_bus_fill(17, [2], "then program 1")


def test_checkpoint_carries_the_faders():
    """state, voice pans, voice mix and every program's four fader values exported with a move pending; a fresh handle takes
    the applied values, snaps, then takes the targets: its next two bus fills are the first handle's, bit for bit"""
    V = 272
    tw = FaderTwin(V, max_frames=256, block=64, bank=_bank2())
    _ramp_setup(tw)
    tw.check_bus_fill(100, [8], "checkpoint, before")
    tw.set_program_fader(0, 0.75, -1.5)
    tw.set_program_fader(1, 0.0, 0.25)
    a = tw.gpus[0]
    state, pans, (gains, buses) = a.export_state(), a.voice_pans(), a.voice_mix()
    faders = [a.get_program_fader(p) for p in range(2)]
    assert all(f[:2] != f[2:] for f in faders)
    b = s2.Synth(V, max_frames=256, block_voices=64)
    b.set_patch_bank(_bank2())
    b.import_state(state)
    b.set_voice_pans(pans)
    b.set_voice_mix(gains, buses)
    for p, f in enumerate(faders):
        b.set_program_fader(p, f[2], f[3])
    b.snap_program_faders()
    for p, f in enumerate(faders):
        b.set_program_fader(p, f[0], f[1])
    assert [b.get_program_fader(p) for p in range(2)] == faders
    for k, n in enumerate([256, 17]):
        tw.note_off(40 + k)
        b.note_off(40 + k)
        pv = tw.rows(n)
        want = tw.want_faded(pv, 8)
        assert_bits_equal_finite(a.sample_buses(n, SR, 8), want, "the checkpointed handle, fill %d" % k)
        assert_bits_equal_finite(b.sample_buses(n, SR, 8), want, "the resumed handle, fill %d" % k)
        tw.commit()
        assert [b.get_program_fader(p) for p in range(2)] == [a.get_program_fader(p) for p in range(2)]


@pytest.mark.parametrize("interleave", [0, 16])
def test_shards_ramp_their_own_voices(interleave):
    V = 512
    if interleave:
        shards = [dict(shard_interleave=16, shard_index=r, shard_count=2) for r in range(2)]
    else:
        shards = [dict(shard_begin=256 * r, shard_voices=256) for r in range(2)]
    tw = FaderTwin(V, max_frames=512, block=64, shards=shards, bank=_bank2())
    assert [g.shard_voices for g in tw.gpus] == [256, 256]
    step = V // 16
    for v in range(V):
        if v % step == 0:
            tw.program_change((v // step) % 2)                   # both programs in both shards, contiguous or dealt out
            tw.setting(v // step)
        tw.note_on(36 + v % 61, VELS[(v + v // 4) % 4])
    tw.check_bus_fill(64, [3, 8], "shards, interleave %d, default" % interleave)
    tw.set_program_fader(0, 1.0 / 3.0, -0.25)
    tw.check_bus_fill(496, [3, 8], "shards, interleave %d, ramp" % interleave)
    tw.note_off(40)
    tw.set_program_fader(0, 0.0, 2.0)
    tw.check_bus_fill(17, [3, 8], "shards, interleave %d, second ramp" % interleave)
    tw.check_bus_fill(16, [3, 8], "shards, interleave %d, static" % interleave)


def test_refusals_leave_the_handle_usable():
    """program >= bank size: S2R_ERR_INVALID; a device-list handle refuses all three entries with S2R_ERR_INVALID (it keeps no
    faders, as it keeps no voice mix, and takes no bus fill) and renders on; the single-device handle renders on, equal to the
    oracle"""
    tw = FaderTwin(272, max_frames=256, block=64, bank=_bank2())
    gpu = tw.gpus[0]
    _ramp_setup(tw)
    L, h = gpu.L, gpu.h
    before = [gpu.get_program_fader(p) for p in range(2)]
    assert L.s2r_set_program_fader(h, 2, 0.5, 0.0) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_program_fader(h, 255, 1.0, 0.0) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_program_fader(h, 2, None, None, None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_program_fader(h, 0, 1.5, 0.0) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_program_fader(h, 2, 1.5, 0.0) == s2s.S2R_ERR_PATCH_RANGE        # the values are looked at first
    assert [gpu.get_program_fader(p) for p in range(2)] == before
    tw.check_bus_fill(64, [4], "after the refusals")
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    one = s2.Synth(512, max_frames=64, mix_groups=2)
    for syn in (multi, one):
        for v in range(512):
            syn.note_on(36 + v % 61)
    f = C.c_float()
    assert multi.L.s2r_set_program_fader(multi.h, 0, 0.5, 0.0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_program_fader(multi.h, 0, 1.0, 0.0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_program_fader(multi.h, 0, C.byref(f), None, None, None) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_snap_program_faders(multi.h) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        multi.set_program_fader(0, 0.5, 0.0)
    assert err.value.status == s2s.S2R_ERR_INVALID
    x, y = multi.sample(np.empty(64, dtype=F), SR), one.sample(np.empty(64, dtype=F), SR)
    assert np.abs(y).max() > 0.0
    assert_bits_equal_finite(x, y, "the device-list handle after the refused fader calls")


def test_range_checks_on_a_handle():
    check_ranges(s2.Synth(8, max_frames=64))
