"""The PCM stage on the device.  Twin handles are fed the same events, one with the stage and one without: the twin's
sample_master gives the stems and the master, which the handle with the stage must return in the same bits (and the loudness and
spectrum rows, where those meters are on), and the expectation for the integers of all nine programmes, the state, t and the clip
counts is s2r_pcm_reference over the twin's output, carried from call to call in numpy (tests/test_pcm_host.py holds that function to
a numpy model of the rule).

Handles, events and the one-pole bank are tests/test_gpu_reverb.py's on 32-voice pools, max_frames 2048 at most.  The levels of the bank's programs are scaled down so that stems and master stay below full
scale (the clipping test scales them up again).  Every comparison is exact.  The kernel's walk stages TILE = 128 frames at a time (s2r_debug_pcm_tile), two tiles in flight and the write-out a third
behind: its edges are calls of TILE - 1, TILE, TILE + 1 and 2 TILE + 3 frames, the tap counts (0, 1 .. 2, 3 .. 5 and 6 .. 9 taps
run four instances of the walk) and who copies the master to the pinned output (the PCM kernel, the loudness kernel, the spectrum
kernel)."""
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
P = s2.PCM_PROGRAMMES
CH, TAPS = s2.PCM_CHANNELS, s2.PCM_MAX_TAPS
MASTER = s2.MAX_BUSES
TILE = 128
T_WRAP = 0xffffff80
SHAPER_OF_K = {0: 0, 1: 1, 2: 2, 5: 4, 9: 5}


def _taps(K, seed=0):
    """a shaper of K taps: the tables' where they have one, else seeded values whose sum of magnitudes stays below 4"""
    if K in SHAPER_OF_K:
        return s2.pcm_shaper(SHAPER_OF_K[K])
    return (np.random.default_rng(100 + K + seed).uniform(-1.0, 1.0, K) * 4.0 / K).astype(F)


class Stage:
    """the PCM stage of a handle in numpy: parameters, the carried state and t, the held clip counts, the last call's integers"""

    def __init__(self, bits=16, dither="tpdf", taps=(), seed=0):
        self.bits, self.dither, self.taps, self.seed = bits, dither, np.asarray(taps, dtype=F), seed
        self.reset()

    def reset(self):
        self.state, self.t = np.zeros((CH, TAPS), dtype=F), 0
        self.held, self.last, self.pcm = np.zeros(CH, dtype=np.uint32), np.zeros(CH, dtype=np.uint32), None

    def set(self, *handles):
        for syn in handles:
            syn.set_master_pcm(self.bits, self.dither, self.taps, self.seed)
            bits, dither, taps, seed = syn.get_master_pcm()
            assert (bits, dither, seed) == (self.bits, s2s._dither_arg(self.dither), self.seed)
            assert_bits_equal_finite(taps, self.taps, "the taps read back")
        self.reset()

    def load(self, syn, state, t):
        syn.set_pcm_state(state, t)
        self.state, self.t = np.array(state, dtype=F).reshape(CH, TAPS), t
        self.state[:, self.taps.size:] = 0.0

    def expect(self, stems, x):
        self.pcm, self.state, self.t, self.last = s2.pcm_reference(stems, x, self.bits, self.dither, self.taps, self.seed, self.state, self.t)
        self.held = self.held + self.last

    def check(self, syn, what, state=False):
        for p in range(P):
            got = syn.pcm(p)
            assert got.dtype == np.int32 and np.array_equal(got, self.pcm[p]), "%s: programme %d" % (what, p)
        last, held = syn.pcm_clips()
        assert np.array_equal(last, self.last) and np.array_equal(held, self.held), what
        if state:                                                # (a read fetches the state, and the next fill sends it back: not after every call)
            st, t = syn.pcm_state()
            assert t == self.t, what
            assert_bits_equal_finite(st, self.state, what + ": state")


def _pfill(a, b, m, n, nb, what, stems=True, state=False, loudness=False, spectrum=False):
    """one call on both handles: the handle with the stage returns the twin's bits, and its integers, counts and (on request) state
    are the reference's over the twin's stems and master"""
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
    if loudness:
        assert_bits_equal_finite(a.loudness_hops(), b.loudness_hops(), what + ": loudness rows")
        assert_bits_equal_finite(a.true_peak()[1], b.true_peak()[1], what + ": true peak")
    if spectrum:
        assert_bits_equal_finite(a.spectrum_rows(), b.spectrum_rows(), what + ": spectrum rows")
    m.check(a, what, state)
    return x, st_b


def _quiet(max_frames=1024, n=2, peak=0.25):
    """_handles with every program's level scaled so that the loudest sample of the stems and the master of a first fill of 1024
    frames is `peak`: the bank's 32 voices sum to many times full scale, which would leave every integer on a rail.  Returns the
    handles and what the scaled master's largest step from frame to frame was."""
    hs = _handles(V, max_frames=max_frames, n=n)
    probe = _handles(V, max_frames=1024)[0]
    _events((probe,), V, 0)
    x, st = probe.sample_master(1024, SR, 8)
    scale = min(1.0, peak / max(float(np.abs(x).max()), float(np.abs(st).max())))
    for syn in hs:
        for p in range(8):
            syn.set_program_mix(p, (1.0 - p / 16.0) * scale, p / 8.0, p)
    return hs, float(np.abs(np.diff(x, axis=0)).max()) * scale


def _limit(handles, max_frames):
    c = _quiet(max_frames)[0][1]                                 # (a ceiling the limiter has to work for, from a handle of its own)
    _events((c,), V, 0)
    ceiling = float(np.abs(c.sample_master(min(max_frames, 1024), SR, 8)[0]).max()) * 0.25
    for syn in handles:
        syn.set_master_limiter(ceiling, 48, 100)


def test_the_tile_is_the_one_named_here():
    tile = s2.load_library().s2r_debug_pcm_tile
    tile.restype, tile.argtypes = C.c_uint32, []
    assert tile() == TILE


# (buses, taps, bits, dither, limiter, loudness, spectrum): every value of each, and each writer of the pinned master — the PCM kernel
# (no meter), the loudness kernel, the spectrum kernel without the loudness kernel — behind the master kernel and behind the limiter
MATRIX = [(1, 0, 16, "tpdf", False, False, False), (2, 1, 8, "rect", True, False, False), (3, 5, 24, "none", False, True, False),
          (8, 9, 16, "tpdf", False, False, True), (8, 9, 24, "rect", True, True, True), (2, 5, 8, "tpdf", False, True, True),
          (3, 0, 24, "rect", True, False, True), (1, 9, 8, "none", False, False, False), (8, 1, 16, "none", True, True, False)]


@pytest.mark.parametrize("nb,K,bits,dither,limiter,loudness,spectrum", MATRIX)
def test_integers_state_and_counts_are_the_reference(nb, K, bits, dither, limiter, loudness, spectrum):
    """the parity matrix, max_frames 2048: calls of 1, 2, K, K + 1, TILE - 1, TILE, TILE + 1, 2 TILE + 3 and 2048 frames, events between
    the calls, every other call without stems; master, stems, loudness rows and spectrum rows are the twin's bits"""
    (a, b), _ = _quiet(2048)
    if limiter:
        _limit((a, b), 2048)
    for syn in (a, b):
        if loudness:
            syn.set_master_loudness(SR, 48, 64)
        if spectrum:
            syn.set_master_spectrum(256, 64, "hann", 8)
    m = Stage(bits, dither, _taps(K), seed=1000 + K)
    m.set(a)
    what = "%d buses, %d taps, %d bits, %s, limiter %s, loudness %s, spectrum %s" % (nb, K, bits, dither, limiter, loudness, spectrum)
    calls = [c for c in (1, 2, K, K + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 2048) if c]
    for fill, c in enumerate(calls):
        _events((a, b), V, fill)
        x, st = _pfill(a, b, m, c, nb, "%s, fill %d of %d frames" % (what, fill, c), stems=fill % 2 == 0, state=fill in (3, len(calls) - 1),
                       loudness=loudness, spectrum=spectrum)
    assert m.t == sum(calls) and not np.array_equal(m.pcm[MASTER, :, 0], m.pcm[MASTER, :, 1])
    assert np.abs(m.pcm[:nb]).max(axis=(1, 2)).all() and np.unique(m.pcm[MASTER]).size > 4 and not m.last[16:].any()
    # a bus past the call's is fed +0.0: nothing without dither, and with it the shaped dither alone, a few LSB
    assert np.abs(m.pcm[nb:MASTER]).max(initial=0) <= (0 if dither == "none" else 64)
    assert not ubits(m.state[:, K:]).any() and (K == 0 or ubits(m.state[:2 * nb, :K]).any())


@pytest.mark.parametrize("K", [2, 3, 4, 6, 7, 8])
def test_loaded_histories_near_the_wrap(K):
    """set_pcm_state loads random, denormal and rail-sized error histories with t just below 2^32 — the tap counts between the tables',
    so every instance of the walk runs with taps past K that are +0.0 —, and the entries past K come back as +0.0"""
    (a, b), _ = _quiet(512)
    m = Stage(16, "tpdf", _taps(K), seed=K)
    m.set(a)
    rng = np.random.default_rng(K)
    rails = np.where(rng.integers(0, 2, (CH, TAPS)) == 0, -2.0, 2.0).astype(F)
    tiny = (rng.integers(1, 1 << 22, (CH, TAPS)).astype(np.uint32) | (rng.integers(0, 2, (CH, TAPS)).astype(np.uint32) << 31)).view(F)
    for fill, st in enumerate((rng.uniform(-2.0, 2.0, (CH, TAPS)).astype(F), tiny, rails)):
        m.load(a, st, T_WRAP - 3 * fill)
        got, t = a.pcm_state()
        assert t == T_WRAP - 3 * fill and not ubits(got[:, K:]).any()
        assert_bits_equal_finite(got, m.state, "the loaded state read back")
        _events((a, b), V, fill)
        _pfill(a, b, m, 300 + fill, 4, "%d taps, history %d" % (K, fill), state=True)
        assert m.t < 1000                                        # (wrapped)


def test_both_rails_clip_and_the_clamp_runs():
    """a differentiator with a gain on every bus (it takes the bank's offset out, so that the signal swings both ways) and no
    limiter: the master passes full scale by a factor of about four in both directions, both rails clip, the errors are clamped, and
    integers, state and counts are still the reference's; afterwards the level returns and so does the loop"""
    (a, b), step = _quiet(1024)
    g = 4.0 / step
    for syn in (a, b):
        for bus in range(8):
            syn.set_bus_eq(bus, np.array([[g, -g, 0.0, 0.0, 0.0]], dtype=F))
    m = Stage(16, "tpdf", _taps(9), seed=5)
    m.set(a)
    lo = hi = 0.0
    rails = set()
    for fill, n in enumerate([700, 2 * TILE + 1, 1024, 1024]):
        _events((a, b), V, fill)
        x, st = _pfill(a, b, m, n, 8, "past full scale, fill %d" % fill, state=True)
        lo, hi = min(lo, float(x.min())), max(hi, float(x.max()))
        rails |= set(np.unique(m.pcm[MASTER])) & {-32768, 32767}
    assert hi > 1.5 and lo < -1.5 and rails == {-32768, 32767} and m.held[16] > 20 and m.held[17] > 20
    for syn in (a, b):
        for bus in range(8):
            syn.clear_bus_eq(bus)
    _events((a, b), V, 4)
    x, _ = _pfill(a, b, m, 400, 8, "back in range", state=True)
    assert np.abs(x).max() < 1.0 and not m.last[16:].any() and np.abs(m.state[16:]).max() <= 1.5


def test_bus_count_stages_events_and_slices(monkeypatch):
    """a bus count that changes between calls (a bus that drops out is fed +0.0 and keeps its errors), a reverb, an EQ and a delay in
    front of the stage on both handles, timed events inside the fills, a rows buffer of 48 frames so that the stems arrive in slices"""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    (a, b), _ = _quiet(1024)
    for syn in (a, b):
        syn.set_bus_reverb(0, _ir(40, 3), 0.5, 0.5)
        syn.set_bus_delay(1, 100, 0.5, 0.25, 0.7, 0.3)
        syn.set_bus_eq(2, np.stack([s2.eq_design(s2.EQ_PEAK, 900.0, 6.0, 1.0, SR)]))
    m = Stage(20, "rect", _taps(5), seed=9)
    m.set(a)
    for fill, (nb, n) in enumerate([(8, 300), (2, 150), (5, 1024), (1, 99), (8, 101)]):
        _events((a, b), V, fill)
        for syn in (a, b):
            syn.note_events(np.array([(ON, 50 + fill, (n // 2) & ~15, 0.8)], dtype=s2.NOTE_EVENT_DTYPE))
        _pfill(a, b, m, n, nb, "fill %d: %d buses, %d frames" % (fill, nb, n), state=True)
        assert np.abs(m.pcm[nb:MASTER]).max(initial=0) <= 64    # (fed +0.0: the shaped dither alone)
    assert m.t == 1674


def test_checkpoint_in_the_middle_of_a_stream():
    """voices, pans, mix, sends and the stage — parameters, the 162 errors and t — into a third handle: the continuations are equal"""
    (a, b), _ = _quiet(512)
    m = Stage(12, "tpdf", _taps(9), seed=77)
    m.set(a)
    for fill, n in enumerate([400, 512, 333]):
        _events((a, b), V, fill)
        _pfill(a, b, m, n, 4, "before the checkpoint, fill %d" % fill)
    st, t = a.pcm_state()
    assert t == 1245
    bits, dither, taps, seed = a.get_master_pcm()
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    c = s2.Synth(V, max_frames=512, block_voices=64)
    c.set_patch_bank(_bank())
    c.import_state(state)
    c.set_voice_pans(pans)
    c.set_voice_mix(gains, buses)
    c.set_voice_sends(sends, sbuses)
    c.set_master_pcm(bits, dither, taps, seed)
    c.set_pcm_state(st, t)
    got_st, got_t = c.pcm_state()
    assert got_t == t
    assert_bits_equal_finite(got_st, st, "the restored state read back")
    for k, n in enumerate([100, 512, 155, 400]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        x, _ = _pfill(a, b, m, n, 4, "the checkpointed handle, fill %d" % k, state=k == 3)
        assert_bits_equal_finite(c.sample_master(n, SR, 4)[0], x, "the resumed handle, fill %d" % k)
        for p in range(P):
            assert np.array_equal(c.pcm(p), m.pcm[p]), "the resumed handle's integers, fill %d" % k
    assert_bits_equal_finite(c.pcm_state()[0], a.pcm_state()[0], "state at the end")
    assert np.array_equal(c.pcm_clips()[0], a.pcm_clips()[0])


def test_reset_clear_and_set_again():
    """reset: state, t and counts as after a set, the parameters kept.  clear: off, the handle's fills equal the twin's, every entry
    that needs the stage refuses; a bus fill or a panned fill between two master fills moves nothing; set again with another tap
    count starts from +0.0"""
    (a, b), _ = _quiet(1024)
    m = Stage(16, "tpdf", _taps(5), seed=3)
    m.set(a)
    L, h = a.L, a.h
    buf = np.zeros(2 * 1024, dtype=np.int32)
    bp, n_got = buf.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t()
    assert L.s2r_get_pcm(h, MASTER, bp, buf.size, C.byref(n_got)) == s2s.S2R_ERR_INVALID      # before any fill that ran the stage
    for fill, n in enumerate([500, 333]):
        _events((a, b), V, fill)
        _pfill(a, b, m, n, 8, "before the reset, fill %d" % fill)
    before = a.pcm_state()
    _events((a, b), V, 10)
    assert_bits_equal_finite(a.sample_buses(64, SR, 8), b.sample_buses(64, SR, 8), "a bus fill beside the stage")
    assert_bits_equal_finite(a.sample_panned(64, SR), b.sample_panned(64, SR), "a panned fill beside the stage")
    assert_bits_equal_finite(a.pcm_state()[0], before[0], "state after other fills")
    assert a.pcm_state()[1] == before[1] == 833 and np.array_equal(a.pcm(MASTER), m.pcm[MASTER])
    a.reset_master_pcm()
    m.reset()
    assert a.get_master_pcm()[0] == 16 and a.get_master_pcm()[2].size == 5
    st, t = a.pcm_state()
    assert t == 0 and not ubits(st).any() and not a.pcm_clips()[1].any()
    assert L.s2r_get_pcm(h, MASTER, bp, buf.size, C.byref(n_got)) == s2s.S2R_ERR_INVALID
    _events((a, b), V, 2)
    _pfill(a, b, m, 700, 8, "after the reset", state=True)
    a.clear_master_pcm()
    assert a.get_master_pcm()[0] == 0
    _events((a, b), V, 3)
    x, st_b = b.sample_master(300, SR, 8)
    got, st = a.sample_master(300, SR, 8)
    assert_bits_equal_finite(got, x, "after clear_master_pcm: master")
    assert_bits_equal_finite(st, st_b, "after clear_master_pcm: stems")
    z = np.zeros(s2.PCM_STATE, dtype=F)
    zp, u = z.ctypes.data_as(s2s._f32p), (C.c_uint32 * CH)()
    for rc in (L.s2r_get_pcm_state(h, zp, z.size, None), L.s2r_set_pcm_state(h, zp, z.size, 0), L.s2r_reset_master_pcm(h),
               L.s2r_get_pcm(h, MASTER, bp, buf.size, C.byref(n_got)), L.s2r_get_pcm_clips(h, u, u)):
        assert rc == s2s.S2R_ERR_INVALID
    m = Stage(24, "rect", _taps(9), seed=4)                      # off, then on with another tap count: the initial state
    m.set(a)
    _events((a, b), V, 4)
    _pfill(a, b, m, 300, 8, "set again", state=True)
    _pfill(a, b, m, 1024, 8, "set again, the second fill", state=True)
    assert m.t == 1324


def test_forty_calls_cut_three_ways_give_the_same_integers():
    """three handles with the stage render the same 10 240 frames in 40 calls each, of lengths mixed three ways (every cut at a
    multiple of 16 frames, where a split fill renders the same bits: the masters are compared first): the integers of every
    programme, the state, t and the held counts are equal"""
    hs, _ = _quiet(1024, n=3)
    cuts = ([256] * 40, [16, 496, 128, 384] * 10, [1008, 16, 272, 240, 64, 160, 144, 144] * 5)
    runs = []
    for syn, cut in zip(hs, cuts):
        syn.set_master_pcm(16, "tpdf", 5, 31)
        _events((syn,), V, 0)
        assert sum(cut) == 10240 and len(cut) == 40
        masters, pcms = [], []
        for n in cut:
            masters.append(syn.sample_master(n, SR, 8, stems=False)[0])
            pcms.append(np.stack([syn.pcm(p) for p in range(P)]))
        runs.append((np.concatenate(masters), np.concatenate(pcms, axis=1)))
    assert np.abs(runs[0][1]).max(axis=(1, 2)).all()
    for syn, (x, pcm) in zip(hs[1:], runs[1:]):
        assert_bits_equal_finite(x, runs[0][0], "the master, another cut")
        assert np.array_equal(pcm, runs[0][1])
        assert_bits_equal_finite(syn.pcm_state()[0], hs[0].pcm_state()[0], "state, another cut")
        assert syn.pcm_state()[1] == hs[0].pcm_state()[1] == 10240
        assert np.array_equal(syn.pcm_clips()[1], hs[0].pcm_clips()[1])


def test_refusals_change_nothing():
    """refused master fills and refused setters leave parameters, state, t, integers and counts as they were, and the next fill equals
    the reference as if they had not happened; a device-list handle refuses every entry"""
    (a, b), _ = _quiet(256)
    m = Stage(16, "tpdf", _taps(9), seed=8)
    m.set(a)
    for fill in range(2):
        _events((a, b), V, fill)
        _pfill(a, b, m, 250, 2, "before the refusals, fill %d" % fill)
    L, h = a.L, a.h
    out, st = np.full(2 * 300, 7.0, dtype=F), np.full(2 * 2 * 300, 7.0, dtype=F)
    op, sp = out.ctypes.data_as(s2s._f32p), st.ctypes.data_as(s2s._f32p)
    good = m.taps.copy()
    gp = good.ctypes.data_as(s2s._f32p)
    nan, big = good.copy(), good.copy()
    nan[3], big[8] = np.nan, 16.5
    zeros = np.zeros(s2.PCM_STATE + 1, dtype=F)
    zp = zeros.ctypes.data_as(s2s._f32p)
    wide = np.zeros(s2.PCM_STATE, dtype=F)
    wide[7] = 2.5
    bad = np.zeros(s2.PCM_STATE, dtype=F)
    bad[161] = np.nan
    buf = np.full(2 * 256, 7, dtype=np.int32)
    bp, n_got = buf.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(7)
    refusals = [
        ("no bus", lambda: L.s2r_fill_master(h, op, sp, st.size, 0, 64, SR), s2s.S2R_ERR_INVALID),
        ("nine buses", lambda: L.s2r_fill_master(h, op, sp, st.size, 9, 64, SR), s2s.S2R_ERR_INVALID),
        ("too many frames", lambda: L.s2r_fill_master(h, op, sp, st.size, 2, 257, SR), s2s.S2R_ERR_TOO_MANY_FRAMES),
        ("7 bits", lambda: L.s2r_set_master_pcm(h, 7, 2, gp, 9, 1), s2s.S2R_ERR_PATCH_RANGE),
        ("25 bits", lambda: L.s2r_set_master_pcm(h, 25, 2, gp, 9, 1), s2s.S2R_ERR_PATCH_RANGE),
        ("dither 3", lambda: L.s2r_set_master_pcm(h, 16, 3, gp, 9, 1), s2s.S2R_ERR_PATCH_RANGE),
        ("ten taps", lambda: L.s2r_set_master_pcm(h, 16, 2, gp, 10, 1), s2s.S2R_ERR_PATCH_RANGE),
        ("a NaN", lambda: L.s2r_set_master_pcm(h, 16, 2, nan.ctypes.data_as(s2s._f32p), 9, 1), s2s.S2R_ERR_PATCH_RANGE),
        ("a tap of 16.5", lambda: L.s2r_set_master_pcm(h, 16, 2, big.ctypes.data_as(s2s._f32p), 9, 1), s2s.S2R_ERR_PATCH_RANGE),
        ("null taps", lambda: L.s2r_set_master_pcm(h, 16, 2, None, 9, 1), s2s.S2R_ERR_INVALID),
        ("a short state", lambda: L.s2r_set_pcm_state(h, zp, s2.PCM_STATE - 1, 0), s2s.S2R_ERR_INVALID),
        ("a long state", lambda: L.s2r_set_pcm_state(h, zp, s2.PCM_STATE + 1, 0), s2s.S2R_ERR_INVALID),
        ("a null state", lambda: L.s2r_set_pcm_state(h, None, s2.PCM_STATE, 0), s2s.S2R_ERR_INVALID),
        ("an error of 2.5", lambda: L.s2r_set_pcm_state(h, wide.ctypes.data_as(s2s._f32p), s2.PCM_STATE, 0), s2s.S2R_ERR_PATCH_RANGE),
        ("an error that is a NaN", lambda: L.s2r_set_pcm_state(h, bad.ctypes.data_as(s2s._f32p), s2.PCM_STATE, 0), s2s.S2R_ERR_PATCH_RANGE),
        ("a small state buffer", lambda: L.s2r_get_pcm_state(h, zp, s2.PCM_STATE - 1, None), s2s.S2R_ERR_INVALID),
        ("programme 9", lambda: L.s2r_get_pcm(h, 9, bp, buf.size, C.byref(n_got)), s2s.S2R_ERR_PATCH_RANGE),
        ("a small sample buffer", lambda: L.s2r_get_pcm(h, MASTER, bp, 2 * 250 - 1, C.byref(n_got)), s2s.S2R_ERR_INVALID),
        ("a null sample buffer", lambda: L.s2r_get_pcm(h, MASTER, None, buf.size, C.byref(n_got)), s2s.S2R_ERR_INVALID),
    ]
    for fill, (name, call, status) in enumerate(refusals):
        assert call() == status, name
        assert (out == 7.0).all() and (st == 7.0).all() and not zeros.any() and (buf == 7).all() and n_got.value == 7, name
        m.check(a, name, state=True)
        got = a.get_master_pcm()
        assert (got[0], got[1], got[3]) == (16, 2, 8) and ubits(got[2]).tolist() == ubits(m.taps).tolist(), name
        if fill % 6 == 0:
            _events((a, b), V, fill + 3)
            _pfill(a, b, m, 250, 2, "after the refusal: " + name)
    a.sample_begin(64, SR)
    assert L.s2r_fill_master(h, op, sp, st.size, 2, 64, SR) == s2s.S2R_ERR_INVALID
    assert (out == 7.0).all()
    b.sample(np.empty(64, dtype=F), SR)
    a.sample_end(np.empty(64, dtype=F))
    _events((a, b), V, 40)
    _pfill(a, b, m, 64, 2, "after the fill in flight", state=True)
    # a device list refuses every entry
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    M, mh = multi.L, multi.h
    u, cl = C.c_uint32(), (C.c_uint32 * CH)()
    assert M.s2r_set_master_pcm(mh, 16, 2, gp, 9, 1) == s2s.S2R_ERR_INVALID
    assert M.s2r_clear_master_pcm(mh) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_master_pcm(mh, C.byref(u), C.byref(u), None, C.byref(u), C.byref(u)) == s2s.S2R_ERR_INVALID
    assert M.s2r_reset_master_pcm(mh) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_pcm(mh, 0, bp, buf.size, C.byref(n_got)) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_pcm_clips(mh, cl, cl) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_pcm_state(mh, zp, s2.PCM_STATE, C.byref(u)) == s2s.S2R_ERR_INVALID
    assert M.s2r_set_pcm_state(mh, zp, s2.PCM_STATE, 0) == s2s.S2R_ERR_INVALID
    assert M.s2r_set_master_pcm(mh, 7, 2, gp, 9, 1) == s2s.S2R_ERR_PATCH_RANGE                # the values are looked at first
    assert not zeros.any() and (buf == 7).all()


def test_timing_entry_and_a_handle_that_never_set_the_stage():
    """s2r_debug_pcm_ms: -1 without s2r_set_timing; under it the PCM kernel's time of the last master fill, 0 when that fill ran
    none.  A handle on which the stage was never set holds nothing of it after a master fill."""
    a = _handles(V)[0]
    ms, sms, alloc = a.L.s2r_debug_pcm_ms, a.L.s2r_debug_spectrum_ms, a.L.s2r_debug_pcm_allocated
    for f in (ms, sms):
        f.restype, f.argtypes = C.c_float, [C.c_void_p]
    alloc.restype, alloc.argtypes = C.c_int, [C.c_void_p]
    _events((a,), V, 0)
    a.sample_master(300, SR, 2)
    assert alloc(a.h) == 0
    a.set_master_pcm(16, "tpdf", 5)
    assert alloc(a.h) == 0                                       # (the first master fill that finds it set allocates)
    a.sample_master(300, SR, 2)
    assert alloc(a.h) == 1 and ms(a.h) == -1.0
    a.set_timing(True)
    a.sample_master(300, SR, 2)
    assert 0.0 < ms(a.h) < 100.0 and sms(a.h) == 0.0
    a.clear_master_pcm()
    a.sample_master(300, SR, 2)
    assert ms(a.h) == 0.0
