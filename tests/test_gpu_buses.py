"""The voice mixer on the device: s2r_fill_buses bit for bit against the oracle's rows, a Python model of the
note_on rule for pans, gains and buses, and s2o.mix_tree per bus and channel over rows * gb_c — and, without any oracle,
against the product's own panned fill.

Every mix is non-degenerate: seeds[v] = v, noise > 0, notes 36 + v % 61.  Every comparison is on bits with no NaN
allowance (helpers.assert_bits_equal_finite)."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
from oracle import s2o
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_gpu_panned import Twin, np_gains, _bank2, _bank_mixed, _onepole, ON, OFF, PROGRAM
from test_mix_host import check_ranges, np_voice_gain
from test_pan_host import np_voice_pan

pytestmark = pytest.mark.gpu
SR = 48000
F = np.float32
VELS = [0.0, 0.25, 0.6, 1.0]
# (level, velocity_sens, bus, pan, key_spread): every bus once, the ends of every range among them
SETTINGS = [(1.0, 0.0, 0, -0.5, 1.0), (0.7, 0.5, 1, 0.7, -1.0 / 3.0), (1.0 / 3.0, 1.0, 2, 0.0, 0.0), (0.25, 0.25, 3, 1.0, 1.0),
            (1.0, 0.7, 4, -1.0, 0.5), (0.5, 0.0, 5, 0.25, -1.0), (0.7, 1.0 / 3.0, 6, -0.25, 0.25), (1.0, 1.0, 7, 0.5, 0.0)]


def ubits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


class BusTwin(Twin):
    """test_gpu_panned.Twin with the model of the voices' gains and buses beside the model of their pans.  `scales`: handle k
    is given every program level times scales[k] (the model keeps scale 1)."""

    def __init__(self, voices, handles=1, scales=None, shards=None, **kw):
        super().__init__(voices, shards=shards if shards is not None else [{}] * handles, **kw)
        self.scales = scales or [1.0] * len(self.gpus)
        self.mix = {}                                            # program -> (level, velocity_sens, bus)
        self.gains = np.ones(voices, dtype=F)                    # the model: pool order
        self.buses = np.zeros(voices, dtype=np.uint8)

    def set_program_mix(self, program, level, sens, bus):
        self.mix[program] = (level, sens, bus)
        for g, sc in zip(self.gpus, self.scales):
            g.set_program_mix(program, level * sc, sens, bus)

    def setting(self, j):
        level, sens, bus, pan, spread = SETTINGS[j % len(SETTINGS)]
        self.set_program_mix(self.program, level, sens, bus)
        self.set_program_pan(self.program, pan, spread)

    def _cpu_on(self, note, velocity=1.0):
        v = self.cpu.next_voice_index()
        self.cpu.note_on(note, velocity)                         # (the reference stores the velocity and never uses it)
        self.cpu.set_seed(v, v)
        pan, spread = self.prog.get(self.program, (0.0, 0.0))
        level, sens, bus = self.mix.get(self.program, (1.0, 0.0, 0))
        self.pans[v] = np_voice_pan(pan, spread, note)
        self.gains[v] = np_voice_gain(level, sens, velocity)
        self.buses[v] = bus
        return v

    def note_on(self, note, velocity=1.0):
        v = self._cpu_on(note, velocity)
        for g in self.gpus:
            assert g.note_on(note, velocity) == v
        return v

    def cpu_event(self, kind, note, velocity=1.0):
        if kind == ON:
            self._cpu_on(note, velocity)
        else:
            super().cpu_event(kind, note)

    # --- expectations ---
    def scaled_gains(self, k=0):
        """(g_L, g_R) of handle k's voices: the pan gains times the voice's gain, one rounded multiply"""
        idx = self.idx[k]
        gl, gr = np_gains(self.pans[idx])
        w = self.gains[idx]
        return gl * w, gr * w

    def want_buses(self, pv, n_buses, k=0):
        """[n_buses, frames, 2]: per bus and channel the tree over the oracle's rows times gb_c"""
        idx = self.idx[k]
        rows = pv[idx]
        fold = np.minimum(self.buses[idx], n_buses - 1)
        out = np.empty((n_buses, pv.shape[1], 2), dtype=F)
        for b in range(n_buses):
            for c, g in enumerate(self.scaled_gains(k)):
                gb = np.where(fold == b, g, F(0.0)).astype(F)     # off the bus: a gain of +0.0, not a skipped term
                out[b, :, c] = s2o.mix_tree(rows * gb[:, None], self.block, self.groups)
        return out

    def check_bus_fill(self, frames, n_buses, what):
        """handle k fills n_buses[k] buses; the oracle's rows are rendered once for all of them"""
        pv = self.rows(frames)
        assert np.isfinite(pv).all()
        for k, (g, nb) in enumerate(zip(self.gpus, n_buses)):
            want = self.want_buses(pv, nb, k)
            got = g.sample_buses(frames, SR, nb)
            assert_bits_equal_finite(got, want, "%s, handle %d, %d buses, %d frames" % (what, k, nb, frames))
            if nb > 1:
                live = [b for b in range(nb) if ubits(want[b]).any()]
                assert len(live) >= 2 and any(not np.array_equal(ubits(want[live[0]]), ubits(want[b])) for b in live[1:]), \
                    "%s: fewer than two distinct sounding buses" % what
        return pv

    def check_mix(self, what):
        for k, g in enumerate(self.gpus):
            gains, buses = g.voice_mix()
            idx = self.idx[k]
            want = self.gains[idx] * F(self.scales[k])          # (a power of two: exact)
            assert np.array_equal(ubits(gains), ubits(want)), what
            assert np.array_equal(buses, self.buses[idx]), what
        self.check_pans(what)


def _drive(tw, lengths, n_buses, what, programs=2):
    """Eight (level, sensitivity, bus, pan, spread) settings over the first V note_ons — given to the current program between
    them, with a program change before each where the bank has several — velocities cycling through VELS; then note_offs;
    then restarts under further settings.  One batch of events in front of every fill, the state carried from fill to fill."""
    V = tw.V
    step = max(1, V // 8)
    for b, n in enumerate(lengths):
        if b == 0:
            for v in range(V):
                if v % step == 0:
                    if programs >= 2:
                        tw.program_change((v // step) % programs)
                    tw.setting(v // step)                        # later note_ons only
                tw.note_on(36 + v % 61, VELS[(v + v // 4) % 4])
            # every bus has a voice, buses 3..7 among them (a 3-bus call folds those onto bus 2), under several gains
            assert len(np.unique(tw.buses)) == min(V, 8) and (tw.buses >= 3).any() and len(np.unique(tw.gains)) >= 4
        elif b == 1:
            for note in range(36, 97, 3):
                tw.note_off(note)
        else:
            if programs >= 2:
                tw.program_change((b + 1) % programs)
            tw.setting(b - 2)                                    # (buses 0, 1, 2: the low buses keep voices in the smallest pools too)
            for k in range(min(V // 2, 5 + 2 * b)):              # restarts: the oldest voices, sounding or released
                tw.note_on(40 + (7 * k + b) % 50, VELS[(k + b) % 4])
            tw.note_off(40 + b % 50)
        tw.check_bus_fill(n, n_buses, "%s, fill %d" % (what, b))
    tw.check_mix(what)


SHAPES = [(8, 0, 0), (17, 0, 0), (272, 64, 0), (1088, 64, 2), (1024, 256, 4)]
BUS_COUNTS = [1, 2, 3, 8]


@pytest.mark.parametrize("programs", [1, 2])
@pytest.mark.parametrize("voices,block,groups", SHAPES)
def test_bus_fill_is_the_tree_over_the_scaled_rows_per_bus(voices, block, groups, programs):
    """the parity matrix: four handles in lockstep, one per bus count (1, 2, 3, 8 — 3: the voices booked on buses 3..7 fold
    onto bus 2, in the instantiation for 4 with its surplus bus), every shape at 1000, 1, 16 and 17 frames (1000: 16-byte
    loads; 1 and 17: the scalar loads), one shape also at max_frames.  programs = 1: the one-pole kernel writes the rows;
    programs = 2: a bank of a one-pole and an LP2 patch with program changes between the note_ons."""
    tw = BusTwin(voices, handles=len(BUS_COUNTS), max_frames=1024, block=block, groups=groups, bank=_bank2() if programs == 2 else None)
    lengths = [1000, 1, 16, 17] + ([1024] if (voices, groups) == (1088, 2) else [])
    _drive(tw, lengths, BUS_COUNTS, "%d voices, block %d, groups %d, %d programs" % (voices, block, groups, programs), programs)


def test_bus_fill_over_a_mixed_bank():
    """one-pole, LP2 and SVF under a DPW oscillator in one pool: the general kernel feeds the rows"""
    tw = BusTwin(272, handles=2, max_frames=1024, block=64, bank=_bank_mixed())
    _drive(tw, [1000, 17, 256], [4, 8], "mixed bank", programs=3)


def _pair(voices, block, groups=0, max_frames=512, bank=None):
    out = []
    for _ in range(2):
        syn = s2.Synth(voices, max_frames=max_frames, block_voices=block, mix_groups=groups)
        if bank is not None:
            syn.set_patch_bank(bank)
        else:
            syn.set_patch(_onepole())
        for v in range(voices):
            syn.set_noise_seed(v, v)
        out.append(syn)
    return out


def _play(handles, voices, programs, fill):
    """the same events on every handle: fill 0 starts every voice, later ones release and restart some"""
    for syn in handles:
        if fill == 0:
            for v in range(voices):
                if programs > 1 and v % 50 == 0:
                    syn.program_change((v // 50) % programs)
                syn.note_on(36 + v % 61, VELS[(v + v // 4) % 4])
        else:
            for note in range(36 + fill, 97, 4):
                syn.note_off(note)
            for k in range(9):
                syn.note_on(41 + 5 * k + fill, VELS[(k + fill) % 4])


@pytest.mark.parametrize("voices,block,groups", [(272, 64, 0), (1088, 64, 2)])
def test_one_bus_with_the_defaults_is_the_panned_fill(voices, block, groups):
    """no program mix ever set, n_buses = 1: every gain is the pan gain times 1.0f, so the bus fill is s2r_fill_panned of a twin
    handle, bit for bit — the new kernels held to the panned mixdown's, no oracle in the loop"""
    a, b = _pair(voices, block, groups, bank=_bank2())
    for syn in (a, b):
        syn.set_program_pan(0, -0.5, 1.0)
        syn.set_program_pan(1, 0.7, -1.0 / 3.0)
    for fill, n in enumerate([500, 17, 1]):
        _play((a, b), voices, 2, fill)
        got, want = a.sample_buses(n, SR, 1), b.sample_panned(n, SR)
        assert np.isfinite(want).all() and np.abs(want).max() > 0.0 and not np.array_equal(want[:, 0], want[:, 1])
        assert_bits_equal_finite(got[0], want, "defaults on one bus, fill %d" % fill)
    gains, buses = a.voice_mix()
    assert np.array_equal(ubits(gains), ubits(np.ones(voices, dtype=F))) and not buses.any()


@pytest.mark.parametrize("j", [0, 2, 3])
def test_every_program_on_one_bus_of_four(j):
    """all programs on bus j of n_buses = 4: bus j is the twin's panned fill; the three others — trees over rows * +0.0 rooted
    at +0.0, negative samples included — are bit pattern 0 everywhere"""
    voices = 272
    a, b = _pair(voices, 64, bank=_bank2())
    for syn in (a, b):
        syn.set_program_pan(0, -0.5, 1.0)
        syn.set_program_pan(1, 0.7, -1.0 / 3.0)
    for p in range(2):
        a.set_program_mix(p, 1.0, 0.0, j)
    for fill, n in enumerate([500, 17]):
        _play((a, b), voices, 2, fill)
        got, want = a.sample_buses(n, SR, 4), b.sample_panned(n, SR)
        assert np.isfinite(want).all() and (want < 0.0).any() and (want > 0.0).any()
        assert_bits_equal_finite(got[j], want, "all on bus %d, fill %d" % (j, fill))
        for other in range(4):
            if other != j:
                assert not ubits(got[other]).any(), "bus %d must be +0.0 everywhere (all voices are on bus %d)" % (other, j)


@pytest.mark.parametrize("voices,block,groups", [(272, 64, 0), (1024, 256, 4)])
def test_half_the_level_is_half_of_every_sample(voices, block, groups):
    """handle 1 has every program level halved, same sensitivities and velocities: every output float is 0.5f times handle 0's,
    bit for bit — a power-of-two scale commutes with every rounding as long as nothing it scales is denormal, which the test
    asserts on the oracle's rows: no non-zero |row * gain| lies below 2^-100"""
    tw = BusTwin(voices, handles=2, scales=[1.0, 0.5], max_frames=1024, block=block, groups=groups, bank=_bank2())
    step = max(1, voices // 8)
    for fill, n in enumerate([1000, 17]):
        if fill == 0:
            for v in range(voices):
                if v % step == 0:
                    tw.program_change((v // step) % 2)
                    tw.setting(v // step)
                tw.note_on(36 + v % 61, VELS[(v + v // 4) % 4])
        else:
            for note in range(36, 97, 3):
                tw.note_off(note)
        pv = tw.rows(n)
        for g in tw.scaled_gains():
            mag = np.abs(pv.astype(np.float64) * g.astype(np.float64)[:, None])
            assert not ((mag > 0.0) & (mag < 2.0 ** -100)).any()
        full, half = tw.gpus[0].sample_buses(n, SR, 3), tw.gpus[1].sample_buses(n, SR, 3)
        assert np.isfinite(full).all() and all(np.abs(full[b]).max() > 0.0 for b in range(3))
        assert_bits_equal_finite(half, full * F(0.5), "half level, fill %d" % fill)
        assert_bits_equal_finite(full, tw.want_buses(pv, 3), "half level: the full handle against the oracle, fill %d" % fill)
    tw.check_mix("half level")


def test_voice_mix_follows_the_note_on_rule():
    """gains and buses read back after note_ons under program changes and a set_program_mix in mid-stream (later note_ons
    only), velocities outside [0, 1] and NaN among them; a voice never started has gain 1 on bus 0"""
    V = 64
    tw = BusTwin(V, max_frames=64, block=64, bank=_bank2())
    tw.set_program_mix(0, 0.7, 0.5, 2)
    tw.set_program_mix(1, 1.0 / 3.0, 1.0, 5)
    vels = [1.5, -1.0, float("nan"), 0.0, 0.25, 0.6, 1.0, float("inf"), 2.0 ** -149, 1.0 - 2.0 ** -24]
    for v in range(V - 8):
        if v % 7 == 0:
            tw.program_change((v // 7) % 2)
        if v == 30:
            tw.set_program_mix(0, 0.25, 1.0, 7)
            before = tw.gains.copy(), tw.buses.copy()
        tw.note_on(36 + v % 61, vels[v % len(vels)])
    assert np.array_equal(ubits(tw.gains[:30]), ubits(before[0][:30])) and np.array_equal(tw.buses[:30], before[1][:30])
    tw.check_mix("voice mix after note_ons")
    assert (tw.gains[V - 8:] == 1.0).all() and not tw.buses[V - 8:].any()
    assert set(np.unique(tw.buses)) == {0, 2, 5, 7}
    # as a batch: the same rule per event, program changes inside the batch included
    ev = [(ON, 50, 0, 1.5), (PROGRAM, 1, 0, 0.0), (ON, 51, 0, float("nan")), (ON, 52, 0, -1.0), (PROGRAM, 0, 0, 0.0), (ON, 53, 0, 0.6)]
    tw.gpus[0].note_events(np.array(ev, dtype=s2.NOTE_EVENT_DTYPE))
    for k, n, f, vel in ev:
        tw.cpu_event(k, n, vel)
    tw.check_mix("voice mix after a batch")
    tw.check_bus_fill(48, [8], "after the batch")


@pytest.mark.parametrize("frames", [256, 250])
def test_events_inside_a_bus_fill(frames):
    """note_ons with their velocities, note_offs and program changes at frames 0, 16, 48 and 240 of one fill: gains and buses
    take effect at the event's frame.  The expectation is built segment by segment from the oracle."""
    V = 64
    tw = BusTwin(V, max_frames=256, block=64, bank=_bank2())
    tw.set_program_pan(0, -0.5, 1.0)
    tw.set_program_pan(1, 0.7, -1.0 / 3.0)
    tw.set_program_mix(0, 0.7, 0.5, 0)
    tw.set_program_mix(1, 1.0, 1.0, 3)
    for fill in range(2):                                        # the second fill starts from the state the first left
        ev = []
        if fill == 0:
            ev += [(ON, 36 + v % 61, 0, VELS[v % 4]) for v in range(V // 2)] + [(PROGRAM, 1, 0, 0.0)]
            ev += [(ON, 36 + v % 61, 0, VELS[(v + 1) % 4]) for v in range(V // 2, V - 4)]
        else:
            ev += [(OFF, 40, 0, 0.0), (ON, 90, 0, 0.25)]
        ev += [(ON, 50, 16, 0.6), (OFF, 36, 16, 0.0), (PROGRAM, 0, 16, 0.0), (ON, 50, 16, 0.25), (ON, 77, 16, 1.0)]
        ev += [(OFF, 50, 48, 0.0), (PROGRAM, 1, 48, 0.0)] + [(ON, 60 + k, 48, VELS[(k + 1) % 4]) for k in range(8)] + [(OFF, 61, 48, 0.0)]
        ev += [(ON, 50, 240, 1.0), (PROGRAM, 0, 240, 0.0), (ON, 99, 240, 0.0), (OFF, 77, 240, 0.0)]
        tw.gpus[0].note_events(np.array(ev, dtype=s2.NOTE_EVENT_DTYPE))
        got = tw.gpus[0].sample_buses(frames, SR, 4)
        want = np.zeros((4, frames, 2), dtype=F)
        bounds = [0, 16, 48, 240, frames]
        for a, b in zip(bounds[:-1], bounds[1:]):
            for k, n, f, vel in ev:
                if f == a:
                    tw.cpu_event(k, n, vel)
            want[:, a:b] = tw.want_buses(tw.rows(b - a), 4)
        assert ubits(want[0]).any() and ubits(want[3]).any()
        assert_bits_equal_finite(got, want, "timed events, %d frames, fill %d" % (frames, fill))
        tw.check_mix("timed events")
    # a mono fill consumes timed note_ons just as well: their gains and buses are the voices' afterwards
    ev = [(ON, 44, 0, 0.6), (PROGRAM, 1, 16, 0.0), (ON, 45, 16, 0.25)]
    tw.gpus[0].note_events(np.array(ev, dtype=s2.NOTE_EVENT_DTYPE))
    mono = tw.gpus[0].sample(np.empty(64, dtype=F), SR)
    tw.cpu_event(ON, 44, 0.6)
    pv0 = tw.rows(16)
    tw.cpu_event(PROGRAM, 1)
    tw.cpu_event(ON, 45, 0.25)
    pv1 = tw.rows(48)
    assert_bits_equal_finite(mono, np.concatenate([s2o.mix_tree(pv0, 64, 1), s2o.mix_tree(pv1, 64, 1)]), "mono fill with timed events")
    tw.check_mix("after a mono fill with timed events")
    tw.check_bus_fill(32, [4], "after a mono fill with timed events")


def test_checkpoint_carries_the_voice_mix():
    V = 272
    tw = BusTwin(V, max_frames=256, block=64, bank=_bank2())
    _drive(tw, [200, 17], [8], "checkpoint, before", programs=2)
    a = tw.gpus[0]
    state, pans, (gains, buses) = a.export_state(), a.voice_pans(), a.voice_mix()
    b = s2.Synth(V, max_frames=256, block_voices=64)
    b.set_patch_bank(_bank2())
    b.import_state(state)
    b.set_voice_pans(pans)
    b.set_voice_mix(gains, buses)
    got = b.voice_mix()
    assert np.array_equal(ubits(got[0]), ubits(gains)) and np.array_equal(got[1], buses)
    # a refused set_voice_mix changes nothing
    u8p = C.POINTER(C.c_uint8)
    for bad_gain, bad_bus in [(1.5, 0), (float("nan"), 0), (0.5, 8)]:
        g2, b2 = np.full(V, 0.5, dtype=F), np.full(V, 1, dtype=np.uint8)
        g2[-1], b2[-1] = bad_gain, bad_bus
        assert b.L.s2r_set_voice_mix(b.h, g2.ctypes.data_as(s2s._f32p), b2.ctypes.data_as(u8p)) == s2s.S2R_ERR_PATCH_RANGE
        got = b.voice_mix()
        assert np.array_equal(ubits(got[0]), ubits(gains)) and np.array_equal(got[1], buses)
    for k, n in enumerate([256, 17]):
        tw.note_off(40 + k)
        b.note_off(40 + k)
        pv = tw.check_bus_fill(n, [8], "the checkpointed handle, fill %d" % k)
        assert_bits_equal_finite(b.sample_buses(n, SR, 8), tw.want_buses(pv, 8), "resumed handle, fill %d" % k)


def test_bus_fills_coexist_with_the_other_fills():
    """a bus fill, then s2r_fill, s2r_fill_panned and fills through the pool-resident kernel on the same handle: every buffer
    matches the oracle; the bus fill allocates the rows buffer the panned fill then uses, and the bus count changes from call
    to call (8, 1, 3)"""
    V = 1024
    tw = BusTwin(V, max_frames=256, block=256)
    gpu = tw.gpus[0]
    L = gpu.L
    L.s2r_debug_pan_slice.restype = C.c_uint32
    L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    gpu.set_resident(True)
    assert L.s2r_debug_pan_slice(gpu.h) == 0
    for v in range(V):
        if v % 128 == 0:
            tw.setting(v // 128)
        tw.note_on(36 + v % 61, VELS[(v + v // 4) % 4])
    kinds = [("buses", 8, 256), ("mono", 0, 256), ("panned", 0, 256), ("buses", 1, 128), ("mono", 0, 16), ("mono", 0, 256), ("buses", 3, 17),
             ("panned", 0, 200), ("buses", 8, 200)]
    for k, (kind, nb, n) in enumerate(kinds):
        if k in (2, 4):
            for note in range(36 + k, 97, 6):
                tw.note_off(note)
        if k in (3, 6, 8):
            tw.setting(k)
            for j in range(20):
                tw.note_on(45 + (j * 3 + k) % 40, VELS[(j + k) % 4])
        what = "coexistence, fill %d (%s)" % (k, kind)
        if kind == "buses":
            tw.check_bus_fill(n, [nb], what)
            assert L.s2r_debug_pan_slice(gpu.h) == 256          # the rows buffer: allocated by the first bus fill, kept
            continue
        pv = tw.rows(n)
        if kind == "mono":
            assert_bits_equal_finite(gpu.sample(np.empty(n, dtype=F), SR), s2o.mix_tree(pv, tw.block, 1), what)
        else:
            assert_bits_equal_finite(gpu.sample_panned(n, SR), tw.want(pv), what)      # (ignores gains and buses)
    tw.check_mix("coexistence")


@pytest.mark.parametrize("interleave", [0, 16])
def test_shards_mix_their_own_voices_per_bus(interleave):
    V = 512
    if interleave:
        shards = [dict(shard_interleave=16, shard_index=r, shard_count=2) for r in range(2)]
    else:
        shards = [dict(shard_begin=256 * r, shard_voices=256) for r in range(2)]
    tw = BusTwin(V, max_frames=512, block=64, shards=shards)
    assert [g.shard_voices for g in tw.gpus] == [256, 256]
    # (contiguous shards: the first holds the voices of buses 0..3, the second those of buses 4..7 — eight buses there)
    _drive(tw, [496, 17], [3, 8], "shards, interleave %d" % interleave, programs=1)
    if interleave:
        assert tw.idx[1][0] == 16 and tw.idx[0][16] == 32       # local order is not pool order


def test_refusals_leave_the_handle_usable():
    """n_buses 0 and 9, a buffer one float short (nothing is consumed: the next fill is the oracle's for those frames), a
    device-list handle: S2R_ERR_INVALID each, and the handle renders on"""
    V = 272
    tw = BusTwin(V, max_frames=256, block=64)
    gpu = tw.gpus[0]
    for v in range(V):
        if v % 34 == 0:
            tw.setting(v // 34)
        tw.note_on(36 + v % 61, VELS[(v + v // 4) % 4])
    tw.check_bus_fill(64, [2], "before the refusals")
    out = np.full(2 * 64 * 9, 7.0, dtype=F)
    p = out.ctypes.data_as(s2s._f32p)
    assert gpu.L.s2r_fill_buses(gpu.h, p, out.size, 0, 64, SR) == s2s.S2R_ERR_INVALID
    assert gpu.L.s2r_fill_buses(gpu.h, p, out.size, 9, 64, SR) == s2s.S2R_ERR_INVALID
    assert gpu.L.s2r_fill_buses(gpu.h, p, 2 * 64 * 3 - 1, 3, 64, SR) == s2s.S2R_ERR_INVALID
    assert gpu.L.s2r_fill_buses(gpu.h, None, 2 * 64 * 3, 3, 64, SR) == s2s.S2R_ERR_INVALID
    assert (out == 7.0).all()                                    # nothing was written
    with pytest.raises(s2.S2rError) as err:
        gpu.sample_buses(64, SR, 9)
    assert err.value.status == s2s.S2R_ERR_INVALID
    tw.check_bus_fill(64, [3], "after the refusals: the frames nobody consumed")
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    one = s2.Synth(512, max_frames=64, mix_groups=2)
    for syn in (multi, one):
        for v in range(512):
            syn.note_on(36 + v % 61)
    with pytest.raises(s2.S2rError) as err:
        multi.sample_buses(64, SR, 2)
    assert err.value.status == s2s.S2R_ERR_INVALID
    gains, buses = np.ones(512, dtype=F), np.zeros(512, dtype=np.uint8)
    u8p = C.POINTER(C.c_uint8)
    assert multi.L.s2r_get_voice_mix(multi.h, gains.ctypes.data_as(s2s._f32p), buses.ctypes.data_as(u8p)) == s2s.S2R_ERR_INVALID
    x, y = multi.sample(np.empty(64, dtype=F), SR), one.sample(np.empty(64, dtype=F), SR)
    assert np.abs(y).max() > 0.0
    assert_bits_equal_finite(x, y, "the device-list handle after the refused bus fill")


def test_range_checks_on_a_handle():
    check_ranges(s2.Synth(8, max_frames=64))
