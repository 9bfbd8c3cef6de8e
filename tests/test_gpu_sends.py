"""Aux sends on the device: s2r_fill_buses bit for bit against the oracle's rows times the gains of the send
rule — gb = M + A per voice, bus and channel, built in numpy float32 from a model of every voice's send and send bus at its
note_on on top of test_gpu_faders' model of pans, gains, buses and faders — through s2o.mix_tree per bus and channel; and, without
any oracle, against the product's own bus fill on a twin handle.

Every mix is non-degenerate: seeds[v] = v, noise > 0, notes 36 + v % 61.  Every comparison is on bits with no NaN allowance
(helpers.assert_bits_equal_finite)."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite, oracle_cfg_from_patch
from oracle import s2o
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_gpu_buses import SETTINGS, SHAPES, VELS, _pair, _play, ubits
from test_gpu_faders import FaderTwin
from test_gpu_panned import _bank2, ON, OFF, PROGRAM
from test_send_host import check_ranges

pytestmark = pytest.mark.gpu
SR = 48000
F = np.float32
BUS_COUNTS = [1, 2, 3, 8]
# (main bus, send, send bus) beside SETTINGS[j]'s level, sensitivity, pan and spread.  No voice is booked on bus 0: it sounds
# through sends only, in every call of two buses or more (so does bus 6 of an 8-bus call).  1: the send lands on the voice's own
# bus; 2: in a 3-bus call a folded main (3 -> 2) and a folded send (7 -> 2) meet on the last bus, in a 2-bus call every pair does;
# 4: a send of 0 with a bus; 7: main and send both on bus 7.
ROUTES = [(1, 0.5, 0), (2, 1.0, 2), (3, 1.0 / 3.0, 7), (5, 0.7, 1), (7, 0.0, 4), (1, 1.0, 0), (2, 0.5, 6), (7, 1.0 / 3.0, 7)]


class SendTwin(FaderTwin):
    """test_gpu_buses.BusTwin (through test_gpu_faders.FaderTwin, for the fills under moving faders) with the model of the voices'
    sends: the send and the send bus of the program current at the note_on; a voice never started: 0 on bus 0."""

    def __init__(self, voices, **kw):
        super().__init__(voices, **kw)
        self.send = {}                                           # program -> (send, send_bus)
        self.sends = np.zeros(voices, dtype=F)                   # the model: pool order
        self.sbuses = np.zeros(voices, dtype=np.uint8)

    def set_program_send(self, program, send, send_bus):
        self.send[program] = (send, send_bus)
        for g in self.gpus:
            g.set_program_send(program, send, send_bus)

    def setting(self, j):
        level, sens, _, pan, spread = SETTINGS[j % len(SETTINGS)]
        bus, send, send_bus = ROUTES[j % len(ROUTES)]
        self.set_program_mix(self.program, level, sens, bus)
        self.set_program_pan(self.program, pan, spread)
        self.set_program_send(self.program, send, send_bus)

    def _cpu_on(self, note, velocity=1.0):
        v = super()._cpu_on(note, velocity)
        send, send_bus = self.send.get(self.program, (0.0, 0))
        self.sends[v] = F(send)
        self.sbuses[v] = send_bus
        return v

    def want_sends(self, pv, n_buses, k=0, i0=0, n_call=None, ramp=True, only_bus=None):
        """[n_buses, frames, 2] for frames [i0, i0 + pv.shape[1]) of a call of n_call frames.  With (G0, d) of FaderTwin.ramp (d = 0
        without a moving fader): H0 = G0 * s, e = d * s; per bus base = sel(G0) + sel(H0), step = sel(d) + sel(e) — the main
        select on min(bus, n - 1), the send's on min(sb, n - 1), +0.0 where it misses, one rounded add each; g[i] = base +
        (float)i * step, the product rounded, then the sum; the tree over rows * g."""
        frames = pv.shape[1]
        n_call = frames if n_call is None else n_call
        idx = self.idx[k]
        rows = pv[idx]
        fm = np.minimum(self.buses[idx], n_buses - 1)
        fs = np.minimum(self.sbuses[idx], n_buses - 1)
        s = self.sends[idx]
        g0l, g0r, dl, dr = self.ramp(k, n_call, ramp)
        i = np.arange(i0, i0 + frames).astype(F)
        zero = F(0.0)
        out = np.zeros((n_buses, frames, 2), dtype=F)
        with np.errstate(under="ignore"):
            for c, (g0, d) in enumerate(((g0l, dl), (g0r, dr))):
                h0, e = (g0 * s).astype(F), (d * s).astype(F)
                for b in range(n_buses) if only_bus is None else [only_bus]:
                    base = (np.where(fm == b, g0, zero) + np.where(fs == b, h0, zero)).astype(F)
                    step = (np.where(fm == b, d, zero) + np.where(fs == b, e, zero)).astype(F)
                    if step.any():
                        g = (base[:, None] + (i[None, :] * step[:, None]).astype(F)).astype(F)
                    else:
                        g = base[:, None]                        # (base + i * +0.0 = base: gains are not negative)
                    out[b, :, c] = s2o.mix_tree((rows * g).astype(F), self.block, self.groups)
        return out

    def send_only_buses(self, pv, n_buses, k, want):
        """the buses of an n_buses call on which no voice is booked and which sound all the same: through sends alone"""
        idx = self.idx[k]
        fm = np.minimum(self.buses[idx], n_buses - 1)
        fs = np.minimum(self.sbuses[idx], n_buses - 1)
        fed = ubits(pv[idx]).any(axis=1) & (self.sends[idx] > 0.0) & (self.gains[idx] > 0.0)
        return [b for b in range(n_buses) if not (fm == b).any() and (fed & (fs == b)).any() and ubits(want[b]).any()]

    def check_bus_fill(self, frames, n_buses, what):
        """handle k fills n_buses[k] buses under the send rule (ramped where a fader is on its way; commits); in every call of
        two buses or more a bus sounds through sends only; a ramped fill of more than one frame differs from d = 0"""
        pv = self.rows(frames)
        assert np.isfinite(pv).all()
        moving = self.moving()
        for k, (g, nb) in enumerate(zip(self.gpus, n_buses)):
            want = self.want_sends(pv, nb, k)
            where = "%s, handle %d, %d buses, %d frames" % (what, k, nb, frames)
            if nb >= 2:
                assert self.send_only_buses(pv, nb, k, want), "%s: no bus sounds through sends only" % where
            if moving and frames > 1:
                assert any(not np.array_equal(ubits(want[b]), ubits(self.want_sends(pv, nb, k, ramp=False, only_bus=b)[b]))
                           for b in range(nb)), "%s: the ramp changes no bit" % where
            got = g.sample_buses(frames, SR, nb)
            assert_bits_equal_finite(got, want, where)
        self.commit()
        self.check_faders(what)
        return pv

    def check_sends(self, what):
        for k, g in enumerate(self.gpus):
            sends, buses = g.voice_sends()
            idx = self.idx[k]
            assert np.array_equal(ubits(sends), ubits(self.sends[idx])), what
            assert np.array_equal(buses, self.sbuses[idx]), what
        self.check_mix(what)


def _start_all(tw, programs):
    """every voice started, the eight settings over the pool (a program change in front of each where the bank has several)"""
    V = tw.V
    step = max(1, V // 8)
    for v in range(V):
        if v % step == 0:
            if programs >= 2:
                tw.program_change((v // step) % programs)
            tw.setting(v // step)                                # later note_ons only
        tw.note_on(36 + v % 61, VELS[(v + v // 4) % 4])
    # the model holds the cases: every send value; a send onto the voice's own bus; sends above a 2- and a 3-bus call's last bus;
    # a folded main and a folded send that meet on the last bus of a 3-bus call; a send of 0 with a bus; nobody booked on bus 0
    live = tw.sends > 0.0
    want = np.array([0.0, 1.0, 0.5, 1.0 / 3.0, 0.7], dtype=F)
    assert np.isin(want, tw.sends).all()
    assert (live & (tw.sbuses == tw.buses)).any() and (live & (tw.sbuses != tw.buses)).any()
    assert (live & (tw.sbuses > 2)).any() and (live & (tw.buses > 2) & (tw.sbuses > 2)).any()
    assert (~live & (tw.sbuses > 0)).any() and not (tw.buses == 0).any() and (live & (tw.sbuses == 0)).any()


def _later(tw, b, programs):
    """what happens in front of the fills after the first: note_offs, then restarts under further settings"""
    if b == 1:
        for note in range(36, 97, 3):
            tw.note_off(note)
    else:
        if programs >= 2:
            tw.program_change((b + 1) % programs)
        tw.setting(5 if b == 2 else 0)                           # (both send to bus 0: it keeps sounding in the smallest pools too)
        for k in range(min(tw.V // 2, 5 + 2 * b)):               # restarts: the oldest voices, sounding or released
            tw.note_on(40 + (7 * k + b) % 50, VELS[(k + b) % 4])
        tw.note_off(40 + b % 50)


@pytest.mark.parametrize("programs", [1, 2])
@pytest.mark.parametrize("voices,block,groups", SHAPES)
def test_bus_fill_with_sends_is_the_tree_over_the_rows_times_main_plus_send(voices, block, groups, programs):
    """the parity matrix: four handles in lockstep, one per bus count (1, 2, 3, 8), fills of 1000 (16-byte loads), 1, 16 and 17
    frames (scalar loads, a tail), eight (send, send bus) settings over the pool"""
    tw = SendTwin(voices, handles=len(BUS_COUNTS), max_frames=1024, block=block, groups=groups, bank=_bank2() if programs == 2 else None)
    what = "%d voices, block %d, groups %d, %d programs" % (voices, block, groups, programs)
    for b, n in enumerate([1000, 1, 16, 17]):
        if b == 0:
            _start_all(tw, programs)
        else:
            _later(tw, b, programs)
        tw.check_bus_fill(n, BUS_COUNTS, "%s, fill %d" % (what, b))
    tw.check_sends(what)


@pytest.mark.parametrize("voices,block,groups", [(272, 64, 0), (1088, 64, 2)])
def test_sends_under_moving_faders(voices, block, groups):
    """the same under moving faders: ramps of 16, 17 and 1000 frames (and a static fill away from the default behind them), the
    expectation from base = sel(G0) + sel(G0 * s), step = sel(d) + sel(d * s)"""
    tw = SendTwin(voices, handles=len(BUS_COUNTS), max_frames=1024, block=block, groups=groups, bank=_bank2())
    what = "%d voices, block %d, groups %d, faders" % (voices, block, groups)
    _start_all(tw, 2)
    walk = [(1.0 / 3.0, -0.25), (0.0, 2.0), (0.7, -2.0), (0.7, -2.0)]
    for b, n in enumerate([16, 17, 1000, 64]):
        tw.set_program_fader(0, *walk[b])
        if b == 1:
            tw.set_program_fader(1, 0.5, 0.25)
        if b:
            _later(tw, b, 2)
        assert tw.moving() == (b < 3)
        tw.check_bus_fill(n, BUS_COUNTS, "%s, fill %d" % (what, b))
    tw.check_sends(what)


def _twins(voices=272, n=2, max_frames=1024):
    hs = _pair(voices, 64, bank=_bank2(), max_frames=max_frames)
    if n == 3:
        hs.append(_pair(voices, 64, bank=_bank2(), max_frames=max_frames)[0])
    for syn in hs:
        syn.set_program_pan(0, -0.5, 1.0)
        syn.set_program_pan(1, 0.7, -1.0 / 3.0)
    return hs


def test_a_full_send_to_an_empty_bus_is_the_main_bus():
    """no oracle in the loop: every program on bus 0 with send 1 to bus 1 — h = g * 1 = g, gb on bus 1 = +0.0 + g = g: bus 1
    equals bus 0 bit for bit, bus 2 is +0.0 everywhere"""
    voices = 272
    a, = _twins(voices)[:1]
    a.set_program_mix(0, 0.7, 0.5, 0)
    a.set_program_mix(1, 1.0, 1.0 / 3.0, 0)
    for p in range(2):
        a.set_program_send(p, 1.0, 1)
    for fill, n in enumerate([500, 17]):
        _play((a,), voices, 2, fill)
        x = a.sample_buses(n, SR, 3)
        assert np.isfinite(x).all() and (x[0] < 0.0).any() and (x[0] > 0.0).any()
        assert_bits_equal_finite(x[1], x[0], "send 1 to bus 1, fill %d" % fill)
        assert not ubits(x[2]).any()


def test_sends_leave_the_other_buses_alone_and_sends_of_zero_change_nothing():
    """no oracle in the loop: handle a sends to buses 2 and 3, handle b never heard of sends: buses 0 and 1 are equal bit for bit
    (M + +0.0 = M), buses 2 and 3 sound on a only.  Handle c has every send set to 0 onto a bus — the kernels with sends run
    there — and equals b on every bus."""
    voices = 272
    a, b, c = _twins(voices, 3)
    for syn in (a, b, c):
        syn.set_program_mix(0, 0.7, 0.5, 0)
        syn.set_program_mix(1, 1.0, 1.0 / 3.0, 1)
    a.set_program_send(0, 0.5, 2)
    a.set_program_send(1, 1.0 / 3.0, 3)
    c.set_program_send(0, 0.0, 2)
    c.set_program_send(1, 0.7, 3)
    c.set_program_send(1, 0.0, 3)
    for fill, n in enumerate([500, 17, 1]):
        _play((a, b, c), voices, 2, fill)
        x, y, z = (syn.sample_buses(n, SR, 4) for syn in (a, b, c))
        assert np.isfinite(y).all() and np.abs(y[0]).max() > 0.0 and np.abs(y[1]).max() > 0.0
        assert_bits_equal_finite(x[:2], y[:2], "buses 0 and 1 beside sends, fill %d" % fill)
        assert np.abs(x[2]).max() > 0.0 and np.abs(x[3]).max() > 0.0 and not ubits(y[2:]).any()
        assert_bits_equal_finite(z, y, "every send 0, fill %d" % fill)
    sends, buses = c.voice_sends()
    assert not ubits(sends).any() and set(np.unique(buses)) == {2, 3}
    sends, buses = b.voice_sends()
    assert not ubits(sends).any() and not buses.any()


def test_half_a_send_to_an_empty_bus_is_half_of_the_main_bus():
    """no oracle in the loop: every program on bus 0, send 0.5 to bus 1: every float of bus 1 is 0.5f times bus 0's, bit for bit —
    a power of two commutes with every rounding while nothing it scales is denormal, which a probe handle's per-voice rows and
    the voices' gains show"""
    voices = 272
    a, probe = _twins(voices)
    for syn in (a, probe):
        syn.set_program_mix(0, 0.7, 0.5, 0)
        syn.set_program_mix(1, 1.0, 1.0 / 3.0, 0)
    for p in range(2):
        a.set_program_send(p, 0.5, 1)
    for fill, n in enumerate([500, 17]):
        _play((a, probe), voices, 2, fill)
        rows = probe.render_voices(n, SR)
        mag = np.abs(rows.astype(np.float64))
        assert not ((mag > 0.0) & (mag < 2.0 ** -90)).any()     # times a gain of at least 2^-8 where it is not 0: no denormal term
        assert np.abs(a.voice_pans()).max() <= 0.95              # both pan gains of every voice are above 0.15
        gains, _ = a.voice_mix()
        assert gains[gains > 0.0].min() >= 2.0 ** -5
        x = a.sample_buses(n, SR, 2)
        assert np.isfinite(x).all() and np.abs(x[0]).max() > 0.0
        assert_bits_equal_finite(x[1], x[0] * F(0.5), "send 0.5, fill %d" % fill)


@pytest.mark.parametrize("frames", [256, 250])
def test_events_inside_a_bus_fill_with_sends(frames):
    """note_ons, note_offs and program changes at frames 0, 16, 48 and 240 of one fill: a note_on's send takes effect at its
    frame, from its segment on.  The expectation is built segment by segment from the oracle."""
    V = 64
    tw = SendTwin(V, max_frames=256, block=64, bank=_bank2())
    tw.set_program_pan(0, -0.5, 1.0)
    tw.set_program_pan(1, 0.7, -1.0 / 3.0)
    tw.set_program_mix(0, 0.7, 0.5, 1)
    tw.set_program_mix(1, 1.0, 1.0, 3)
    tw.set_program_send(0, 0.5, 2)
    tw.set_program_send(1, 1.0 / 3.0, 0)
    for fill in range(2):                                        # the second fill starts from the state the first left
        ev = []
        if fill == 0:
            ev += [(ON, 36 + v % 61, 0, VELS[v % 4]) for v in range(V // 2)] + [(PROGRAM, 1, 0, 0.0)]
            ev += [(ON, 36 + v % 61, 0, VELS[(v + 1) % 4]) for v in range(V // 2, V - 4)]
        else:
            ev += [(OFF, 40, 0, 0.0), (ON, 90, 0, 0.25)]
        ev += [(ON, 50, 16, 0.6), (OFF, 36, 16, 0.0), (PROGRAM, 0, 16, 0.0), (ON, 50, 16, 0.25), (ON, 77, 16, 1.0)]
        ev += [(OFF, 50, 48, 0.0), (PROGRAM, 1, 48, 0.0)] + [(ON, 60 + k, 48, VELS[(k + 1) % 4]) for k in range(8)] + [(OFF, 61, 48, 0.0)]
        ev += [(ON, 50, 240, 1.0), (PROGRAM, 0, 240, 0.0), (ON, 99, 240, 0.6), (OFF, 77, 240, 0.0)]
        tw.gpus[0].note_events(np.array(ev, dtype=s2.NOTE_EVENT_DTYPE))
        got = tw.gpus[0].sample_buses(frames, SR, 4)
        want = np.zeros((4, frames, 2), dtype=F)
        late = np.zeros((4, frames, 2), dtype=F)                 # the same with the sends of the fill's END throughout: must differ
        bounds = [0, 16, 48, 240, frames]
        pvs = []
        for a, b in zip(bounds[:-1], bounds[1:]):
            for k, n, f, vel in ev:
                if f == a:
                    tw.cpu_event(k, n, vel)
            pvs.append(tw.rows(b - a))
            want[:, a:b] = tw.want_sends(pvs[-1], 4)
        for pv, a, b in zip(pvs, bounds[:-1], bounds[1:]):
            late[:, a:b] = tw.want_sends(pv, 4)
        assert ubits(want[0]).any() and ubits(want[2]).any() and not np.array_equal(ubits(want[:, :240]), ubits(late[:, :240]))
        assert_bits_equal_finite(got, want, "timed events, %d frames, fill %d" % (frames, fill))
        tw.check_sends("timed events")
    # a mono fill consumes timed note_ons just as well: their sends are the voices' afterwards
    ev = [(ON, 44, 0, 0.6), (PROGRAM, 1, 16, 0.0), (ON, 45, 16, 0.25)]
    tw.gpus[0].note_events(np.array(ev, dtype=s2.NOTE_EVENT_DTYPE))
    tw.gpus[0].sample(np.empty(64, dtype=F), SR)
    tw.cpu_event(ON, 44, 0.6)
    tw.rows(16)
    tw.cpu_event(PROGRAM, 1)
    tw.cpu_event(ON, 45, 0.25)
    tw.rows(48)
    tw.check_sends("after a mono fill with timed events")
    tw.check_bus_fill(32, [4], "after a mono fill with timed events")


@pytest.mark.parametrize("frames", [256, 250])
@pytest.mark.parametrize("n_buses", [3, 8])
def test_pans_levels_sends_and_a_moving_fader_over_event_segments_and_slices(n_buses, frames, monkeypatch):
    """every attribute of the mixer in one fill: pans with key spread, levels and buses on both programs, sends from both to
    different buses, program 0's fader on its way, note_ons, note_offs and program changes at frames 0, 16 and 128, and a rows
    buffer of 48 frames, so that the segments are sliced as well.  The expectation is the oracle's rows times M + A under the
    ramp, segment by segment.  Then a checkpoint with a fader move pending into a fresh handle: the next fill is equal on both."""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    V = 272
    tw = SendTwin(V, max_frames=256, block=64, bank=_bank2())
    a = tw.gpus[0]
    tw.set_program_pan(0, -0.5, 1.0)
    tw.set_program_pan(1, 0.7, -1.0 / 3.0)
    tw.set_program_mix(0, 0.7, 0.5, 1)
    tw.set_program_mix(1, 1.0, 1.0 / 3.0, 3)                     # (a 3-bus call folds it onto bus 2, where its send lands too)
    tw.set_program_send(0, 0.5, 0)
    tw.set_program_send(1, 1.0 / 3.0, 2)
    for v in range(V // 2):
        if v % 34 == 0:
            tw.program_change((v // 34) % 2)
        tw.note_on(36 + v % 61, VELS[(v + v // 4) % 4])
    tw.set_program_fader(1, 0.5, 0.25)
    tw.snap()
    tw.set_program_fader(0, 0.25, 1.0)
    ev = [(OFF, 40, 0, 0.0), (PROGRAM, 0, 0, 0.0), (ON, 90, 0, 0.25), (PROGRAM, 1, 0, 0.0), (ON, 91, 0, 0.6)]
    ev += [(ON, 50, 16, 0.6), (OFF, 36, 16, 0.0), (PROGRAM, 0, 16, 0.0), (ON, 50, 16, 0.25), (ON, 77, 16, 1.0)]
    ev += [(OFF, 50, 128, 0.0), (PROGRAM, 1, 128, 0.0)] + [(ON, 60 + k, 128, VELS[(k + 1) % 4]) for k in range(8)] + [(OFF, 61, 128, 0.0)]
    a.note_events(np.array(ev, dtype=s2.NOTE_EVENT_DTYPE))
    got = a.sample_buses(frames, SR, n_buses)
    a.L.s2r_debug_pan_slice.restype = C.c_uint32
    a.L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    assert a.L.s2r_debug_pan_slice(a.h) == 48
    want = np.zeros((n_buses, frames, 2), dtype=F)
    still = np.zeros((n_buses, frames, 2), dtype=F)
    bounds = [0, 16, 128, frames]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        for k, n, f, vel in ev:
            if f == lo:
                tw.cpu_event(k, n, vel)
        pv = tw.rows(hi - lo)
        want[:, lo:hi] = tw.want_sends(pv, n_buses, i0=lo, n_call=frames)
        still[:, lo:hi] = tw.want_sends(pv, n_buses, i0=lo, n_call=frames, ramp=False)
    assert ubits(want[0]).any() and ubits(want[2]).any() and not np.array_equal(ubits(want), ubits(still))
    assert_bits_equal_finite(got, want, "everything at once, %d buses, %d frames" % (n_buses, frames))
    tw.commit()
    tw.check_faders("everything at once")
    tw.check_sends("everything at once")
    # the checkpoint: state, voice pans, voice mix, voice sends and the faders' four values, a move pending
    tw.set_program_fader(0, 0.75, -1.5)
    tw.set_program_fader(1, 0.0, 0.25)
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    faders = [a.get_program_fader(p) for p in range(2)]
    assert all(f[:2] != f[2:] for f in faders)
    b = s2.Synth(V, max_frames=256, block_voices=64)
    b.set_patch_bank(_bank2())
    b.import_state(state)
    b.set_voice_pans(pans)
    b.set_voice_mix(gains, buses)
    b.set_voice_sends(sends, sbuses)
    for p, f in enumerate(faders):
        b.set_program_fader(p, f[2], f[3])
    b.snap_program_faders()
    for p, f in enumerate(faders):
        b.set_program_fader(p, f[0], f[1])
    assert [b.get_program_fader(p) for p in range(2)] == faders
    tw.note_off(41)
    b.note_off(41)
    pv = tw.rows(frames)
    want = tw.want_sends(pv, n_buses)
    x, y = a.sample_buses(frames, SR, n_buses), b.sample_buses(frames, SR, n_buses)
    assert_bits_equal_finite(x, want, "the checkpointed handle")
    assert_bits_equal_finite(y, x, "the resumed handle")


def test_checkpoint_carries_the_voice_sends():
    V = 272
    tw = SendTwin(V, max_frames=256, block=64, bank=_bank2())
    _start_all(tw, 2)
    tw.check_bus_fill(200, [8], "checkpoint, before")
    a = tw.gpus[0]
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    assert ubits(sends).any() and sbuses.any()
    b = s2.Synth(V, max_frames=256, block_voices=64)
    b.set_patch_bank(_bank2())
    b.import_state(state)
    b.set_voice_pans(pans)
    b.set_voice_mix(gains, buses)
    b.set_voice_sends(sends, sbuses)
    got = b.voice_sends()
    assert np.array_equal(ubits(got[0]), ubits(sends)) and np.array_equal(got[1], sbuses)
    # a refused set_voice_sends changes nothing
    u8p = C.POINTER(C.c_uint8)
    for bad_send, bad_bus in [(1.5, 0), (float("nan"), 0), (0.5, 8)]:
        s2_, b2 = np.full(V, 0.5, dtype=F), np.full(V, 1, dtype=np.uint8)
        s2_[-1], b2[-1] = bad_send, bad_bus
        assert b.L.s2r_set_voice_sends(b.h, s2_.ctypes.data_as(s2s._f32p), b2.ctypes.data_as(u8p)) == s2s.S2R_ERR_PATCH_RANGE
        got = b.voice_sends()
        assert np.array_equal(ubits(got[0]), ubits(sends)) and np.array_equal(got[1], sbuses)
    for k, n in enumerate([256, 17]):
        tw.note_off(40 + k)
        b.note_off(40 + k)
        pv = tw.check_bus_fill(n, [8], "the checkpointed handle, fill %d" % k)
        assert_bits_equal_finite(b.sample_buses(n, SR, 8), tw.want_sends(pv, 8), "resumed handle, fill %d" % k)


def test_a_new_bank_keeps_the_survivors_sends():
    """s2r_set_patch_bank with the same two patches and a third: programs 0 and 1 keep their sends, program 2 starts at (0, 0);
    note_ons after it follow them"""
    V = 272
    tw = SendTwin(V, max_frames=256, block=64, bank=_bank2())
    _start_all(tw, 2)
    tw.check_bus_fill(48, [8], "before the new bank")
    before = [tw.gpus[0].get_program_send(p) for p in range(2)]
    assert all(s > 0.0 for s, _ in before)
    bank3 = _bank2() + [_bank2()[0]]
    tw.gpus[0].set_patch_bank(bank3)
    tw.cpu.set_bank([oracle_cfg_from_patch(p) for p in bank3])
    assert [tw.gpus[0].get_program_send(p) for p in range(2)] == before and tw.gpus[0].get_program_send(2) == (0.0, 0)
    for p in (2, 1):
        tw.program_change(p)
        for k in range(6):
            tw.note_on(50 + 3 * k + p, VELS[k % 4])
    assert not tw.sends[tw.vprog == 2].any() and (tw.vprog == 2).sum() == 6
    tw.check_bus_fill(64, [8], "after the new bank")
    tw.check_sends("after the new bank")


def test_the_other_fills_ignore_sends():
    """s2r_fill_panned, s2r_fill and s2r_fill_stereo of a handle with sends equal those of a handle without"""
    voices = 272
    a, b = _twins(voices, max_frames=512)
    for syn in (a, b):
        syn.set_program_mix(1, 0.7, 0.5, 1)
    a.set_program_send(0, 1.0, 1)
    a.set_program_send(1, 0.5, 0)
    _play((a, b), voices, 2, 0)
    assert_bits_equal_finite(a.sample_panned(100, SR), b.sample_panned(100, SR), "panned fill beside sends")
    assert_bits_equal_finite(a.sample(np.empty(64, dtype=F), SR), b.sample(np.empty(64, dtype=F), SR), "mono fill beside sends")
    assert_bits_equal_finite(a.sample_stereo(33, SR), b.sample_stereo(33, SR), "stereo copy beside sends")
    x, y = a.sample_buses(64, SR, 2), b.sample_buses(64, SR, 2)
    assert np.abs(y).max() > 0.0 and not np.array_equal(ubits(x), ubits(y))


@pytest.mark.parametrize("interleave", [0, 16])
def test_shards_send_their_own_voices(interleave):
    V = 512
    if interleave:
        shards = [dict(shard_interleave=16, shard_index=r, shard_count=2) for r in range(2)]
    else:
        shards = [dict(shard_begin=256 * r, shard_voices=256) for r in range(2)]
    tw = SendTwin(V, max_frames=512, block=64, shards=shards, bank=_bank2())
    assert [g.shard_voices for g in tw.gpus] == [256, 256]
    step = V // 16
    for v in range(V):
        if v % step == 0:
            tw.program_change((v // step) % 2)                   # every setting in both shards, contiguous or dealt out
            tw.setting(v // step)
        tw.note_on(36 + v % 61, VELS[(v + v // 4) % 4])
    tw.check_bus_fill(16, [3, 8], "shards, interleave %d" % interleave)
    tw.note_off(40)
    tw.set_program_fader(0, 1.0 / 3.0, -0.25)
    tw.check_bus_fill(17, [3, 8], "shards, interleave %d, ramp" % interleave)
    tw.check_bus_fill(496, [3, 8], "shards, interleave %d, static" % interleave)
    tw.check_sends("shards")
    if interleave:
        assert tw.idx[1][0] == 16 and tw.idx[0][16] == 32       # local order is not pool order


def test_refusals_leave_the_handle_usable():
    """values out of range and a program past the bank change nothing and the handle renders on, equal to the oracle; a
    device-list handle refuses all four entries with S2R_ERR_INVALID and renders on"""
    tw = SendTwin(272, max_frames=256, block=64, bank=_bank2())
    gpu = tw.gpus[0]
    _start_all(tw, 2)
    L, h = gpu.L, gpu.h
    before = [gpu.get_program_send(p) for p in range(2)]
    assert L.s2r_set_program_send(h, 2, 0.5, 0) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_program_send(h, 255, 1.0, 0) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_program_send(h, 2, None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_program_send(h, 0, 1.5, 0) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_program_send(h, 0, 0.5, 8) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_program_send(h, 2, float("nan"), 0) == s2s.S2R_ERR_PATCH_RANGE        # the values are looked at first
    assert [gpu.get_program_send(p) for p in range(2)] == before
    tw.check_bus_fill(64, [4], "after the refusals")
    tw.check_sends("after the refusals")
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    one = s2.Synth(512, max_frames=64, mix_groups=2)
    for syn in (multi, one):
        for v in range(512):
            syn.note_on(36 + v % 61)
    f, u = C.c_float(), C.c_uint32()
    sends, buses = np.zeros(512, dtype=F), np.zeros(512, dtype=np.uint8)
    u8p = C.POINTER(C.c_uint8)
    assert multi.L.s2r_set_program_send(multi.h, 0, 0.5, 1) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_program_send(multi.h, 0, 0.0, 0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_program_send(multi.h, 0, C.byref(f), C.byref(u)) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_voice_sends(multi.h, sends.ctypes.data_as(s2s._f32p), buses.ctypes.data_as(u8p)) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_voice_sends(multi.h, sends.ctypes.data_as(s2s._f32p), buses.ctypes.data_as(u8p)) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        multi.set_program_send(0, 0.5, 1)
    assert err.value.status == s2s.S2R_ERR_INVALID
    x, y = multi.sample(np.empty(64, dtype=F), SR), one.sample(np.empty(64, dtype=F), SR)
    assert np.abs(y).max() > 0.0
    assert_bits_equal_finite(x, y, "the device-list handle after the refused send calls")


def test_range_checks_on_a_handle():
    check_ranges(s2.Synth(8, max_frames=64))
