"""The sample-rate converter on the device.  Twin handles are fed the same events, one with the stage and one without:
the twin's sample_master gives the stems and the master, which the handle with the stage must return in the same bits (and the loudness
and spectrum rows, where those meters are on), and the expectation for the output frames of all nine programmes, the count, the state
and ph is s2r_resampler_reference over the twin's output, carried from call to call in numpy (tests/test_resampler_host.py holds that
function to a numpy model of the rule).  With the PCM stage behind it the integers, its state, t and clips are s2r_pcm_reference over
the resampler's expectation with eight buses.

Handles, events and the one-pole bank are tests/test_gpu_reverb.py's on 32-voice pools, max_frames 2048 at most; the levels are
tests/test_gpu_pcm.py's.  Every comparison is exact.  A workgroup of the kernel makes TILE = 64 output frames
(s2r_debug_resampler_tile): its edges are calls of about TILE * M / L input frames, one less and one more; the other edges are calls of 1,
2, T - 1 and T frames (the history), 2047 and 2048, and who copies the master to the pinned output (the resampler kernel, the loudness
kernel, the spectrum kernel)."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_gpu_buses import ubits
from test_gpu_panned import ON
from test_gpu_pcm import Stage, _limit, _quiet, _taps
from test_gpu_reverb import SR, _bank, _events, _ir

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
V = 32
P = s2.RESAMPLER_PROGRAMMES
CH = s2.RESAMPLER_CHANNELS
MASTER = s2.MAX_BUSES
TILE = 64


def same(got, want, what):
    """the bits, NaNs at the same places"""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaNs"
    assert np.array_equal(got.view(U)[~nan], want.view(U)[~nan]), what


class Res:
    """the resampler of a handle in numpy: parameters, the carried state and ph, the last call's outputs"""

    def __init__(self, L, M, table):
        self.L, self.M, self.table = L, M, np.ascontiguousarray(table, dtype=F)
        self.T = self.table.shape[1]
        self.reset()

    def reset(self):
        self.state, self.ph, self.out, self.made = np.zeros((CH, self.T - 1), dtype=F), 0, None, 0

    def set(self, *handles):
        for syn in handles:
            syn.set_master_resampler(self.L, self.M, self.table)
            L, M, table = syn.get_master_resampler()
            assert (L, M) == (self.L, self.M)
            assert_bits_equal_finite(table, self.table, "the table read back")
        self.reset()

    def load(self, syn, state, ph):
        syn.set_resampler_state(state, ph)
        self.state, self.ph = np.array(state, dtype=F).reshape(CH, self.T - 1), ph

    def expect(self, stems, x):
        assert s2.resampler_count(self.L, self.M, self.ph, x.shape[0]) <= s2.resampler_max_out(x.shape[0], self.L, self.M)
        self.out, self.state, self.ph = s2.resampler_reference(stems, x, self.L, self.M, self.table, self.state, self.ph)
        self.made += self.out.shape[1]

    def check(self, syn, what, state=False):
        for p in range(P):
            got = syn.resampled(p)
            assert got.dtype == F
            same(got, self.out[p], "%s: programme %d" % (what, p))
        if state:                                                # (a read fetches the state, and the next fill sends it back: not after every call)
            st, ph = syn.resampler_state()
            assert ph == self.ph, what
            same(st, self.state, what + ": state")


def _rfill(a, b, r, n, nb, what, stems=True, state=False, loudness=False, spectrum=False, pcm=None):
    """one call on both handles: the handle with the stage returns the twin's bits, and its outputs and (on request) state are the
    reference's over the twin's stems and master; `pcm`: the Stage behind it, fed the reference's outputs as eight buses"""
    x, st_b = b.sample_master(n, SR, nb)
    assert np.isfinite(x).all() and np.isfinite(st_b).all()
    r.expect(st_b, x)
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
    r.check(a, what, state)
    if pcm is not None:
        if r.out.shape[1]:
            pcm.expect(r.out[:MASTER], r.out[MASTER])
        else:                                                    # no frame: no PCM kernel, state, t and the held clips stay
            pcm.pcm, pcm.last = np.zeros((P, 0, 2), dtype=np.int32), np.zeros(CH, dtype=np.uint32)
        pcm.check(a, what + ": PCM behind", state)
    return x, st_b


def _edges(L, M, T):
    """call lengths: the history's, those that end about a tile of output frames, and the handle's most"""
    c = max(TILE * M // L, 2)
    return [n for n in (1, 2, T - 1, T, c - 1, c, c + 1, 2 * c + 1, 2047, 2048) if n >= 1]


def test_the_tile_is_the_one_named_here():
    tile = s2.load_library().s2r_debug_resampler_tile
    tile.restype, tile.argtypes = C.c_uint32, []
    assert tile() == TILE


# (L, M, T, buses, limiter, loudness, spectrum): the ratios, T 4 and both ends of the table budget; 1, 3 and 8 buses; each writer of the
# pinned master — the resampler kernel (no meter), the loudness kernel, the spectrum kernel without the loudness kernel — behind the
# master kernel and behind the limiter
MATRIX = [(1, 1, 4, 1, False, False, False), (2, 1, 32, 3, True, False, False), (1, 2, 64, 8, False, True, False), (4, 1, 8, 1, False, False, True),
          (1, 4, 16, 3, True, True, True), (2, 3, 48, 8, False, True, True), (147, 160, 32, 8, True, False, True), (160, 147, 32, 3, False, False, False),
          (147, 320, 64, 1, True, True, False), (192, 175, 128, 3, False, False, False), (320, 147, 76, 8, True, False, False)]


@pytest.mark.parametrize("L,M,T,nb,limiter,loudness,spectrum", MATRIX)
def test_outputs_count_state_and_position_are_the_reference(L, M, T, nb, limiter, loudness, spectrum):
    """the parity matrix, max_frames 2048: events between the calls, every other call without stems; master, stems, loudness rows and
    spectrum rows are the twin's bits"""
    (a, b), _ = _quiet(2048)
    if limiter:
        _limit((a, b), 2048)
    for syn in (a, b):
        if loudness:
            syn.set_master_loudness(SR, 48, 64)
        if spectrum:
            syn.set_master_spectrum(256, 64, "hann", 8)
    r = Res(L, M, s2.resampler_design(L, M, T))
    r.set(a)
    what = "%d/%d, T %d, %d buses, limiter %s, loudness %s, spectrum %s" % (L, M, T, nb, limiter, loudness, spectrum)
    calls = _edges(L, M, T)
    for fill, c in enumerate(calls):
        _events((a, b), V, fill)
        _rfill(a, b, r, c, nb, "%s, fill %d of %d frames" % (what, fill, c), stems=fill % 2 == 0, state=fill in (3, len(calls) - 1),
               loudness=loudness, spectrum=spectrum)
    total = sum(calls) * L
    assert r.made == (total + M - 1) // M and r.ph == r.made * M - total
    assert np.abs(r.out[:nb]).max(axis=(1, 2)).all() and not np.array_equal(r.out[MASTER, :, 0], r.out[MASTER, :, 1])
    assert not ubits(r.out[nb:MASTER]).any() and ubits(r.state[:2 * nb]).any() and not ubits(r.state[2 * nb:16]).any()


def test_single_frames_at_a_quarter_and_at_four():
    """1/4 fed single frames makes a frame every fourth call and none in between (s2r_get_resampled answers 0 frames); 4/1 makes four
    frames of every one"""
    (a, b), _ = _quiet(64)
    r = Res(1, 4, s2.resampler_design(1, 4, 16))
    r.set(a)
    _events((a, b), V, 0)
    counts = []
    for fill in range(13):
        _rfill(a, b, r, 1, 3, "1/4, frame %d" % fill, state=fill % 5 == 4)
        counts.append(r.out.shape[1])
    assert counts == [1, 0, 0, 0] * 3 + [1]
    r = Res(4, 1, s2.resampler_design(4, 1, 8))
    r.set(a)
    for fill in range(9):
        _rfill(a, b, r, 1, 3, "4/1, frame %d" % fill, state=fill == 8)
        assert r.out.shape[1] == 4
    _rfill(a, b, r, 64, 3, "4/1, 64 frames", state=True)
    assert r.out.shape[1] == 256


@pytest.mark.parametrize("L,M,T", [(147, 160, 48), (2, 3, 8), (160, 147, 32), (1, 4, 128)])
def test_loaded_histories_at_the_last_position(L, M, T):
    """set_resampler_state loads random histories with ph = M - 1: the first outputs read them through every tap"""
    (a, b), _ = _quiet(512)
    r = Res(L, M, s2.resampler_design(L, M, T))
    r.set(a)
    rng = np.random.default_rng(T)
    for fill, n in enumerate((300, 1, T - 2)):
        st = rng.uniform(-0.5, 0.5, (CH, T - 1)).astype(F)
        r.load(a, st, M - 1)
        got, ph = a.resampler_state()
        assert ph == M - 1
        assert_bits_equal_finite(got, st, "the loaded state read back")
        _events((a, b), V, fill)
        _rfill(a, b, r, n, 4, "%d/%d, history %d" % (L, M, fill), state=True)
        assert ubits(r.out[4:MASTER]).any() or r.out.shape[1] == 0      # (a bus past the call's still rings its history out)


def test_the_identity_table_returns_the_stems_and_the_master():
    """{1, 0, 0, 0} at 1/1: every programme comes back in the twin's bits, with no model in the loop"""
    (a, b), _ = _quiet(1024)
    a.set_master_resampler(1, 1, np.array([[1.0, 0.0, 0.0, 0.0]], dtype=F))
    for fill, n in enumerate((1, 63, 64, 65, 1000)):
        _events((a, b), V, fill)
        x, st = b.sample_master(n, SR, 8)
        got, _ = a.sample_master(n, SR, 8)
        assert_bits_equal_finite(got, x, "master")
        for p in range(8):                                       # (x + 0.0: a -0.0 comes back as +0.0, every other value as itself)
            assert_bits_equal_finite(a.resampled(p), st[p] + F(0.0), "bus %d of fill %d" % (p, fill))
        assert_bits_equal_finite(a.resampled(MASTER), x + F(0.0), "the master of fill %d" % fill)
    assert np.abs(a.resampled(MASTER)).max() > 0.0 and np.abs(a.resampled(7)).max() > 0.0


def test_non_finite_and_denormal_histories():
    """NaN, infinities, denormals and -0.0 loaded through set_resampler_state: the outputs that read them are the reference's, the
    master and the stems stay the twin's, and the history rings out"""
    (a, b), _ = _quiet(256)
    L, M, T = 2, 3, 16
    r = Res(L, M, s2.resampler_design(L, M, T))
    r.set(a)
    rng = np.random.default_rng(3)
    st = rng.uniform(-0.5, 0.5, (CH, T - 1)).astype(F)
    st[0, 2], st[3, 0], st[16, 5], st[17, 14] = np.nan, np.inf, -np.inf, np.nan
    st[4] = (rng.integers(1, 1 << 22, T - 1).astype(U) | U(0x80000000)).view(F)
    st[5] = -0.0
    r.load(a, st, 1)
    got, ph = a.resampler_state()
    same(got, st, "the loaded state read back")
    _events((a, b), V, 0)
    with np.errstate(invalid="ignore"):
        _rfill(a, b, r, 100, 8, "non-finite history", state=True)
    assert np.isnan(r.out[0, :, 0]).any() and not np.isfinite(r.out[MASTER, :12]).all() and np.isfinite(r.out[:, 40:]).all()
    _rfill(a, b, r, 100, 8, "after it", state=True)
    assert np.isfinite(r.out).all() and np.isfinite(r.state).all()


@pytest.mark.parametrize("K,L,M,T", [(9, 147, 160, 48), (0, 160, 147, 32), (9, 1, 4, 16)])
def test_the_pcm_stage_behind_it(K, L, M, T):
    """integers, PCM state, t and clips against the composed references, at nine taps and at none; at 1/4 a call of one frame that
    makes no output lies between two that do: no PCM kernel runs, its state and t stay and s2r_get_pcm answers 0 frames"""
    (a, b), _ = _quiet(1024)
    loud = (L, M) != (160, 147)                                  # (without a meter the resampler kernel copies the master out, and the PCM kernel must not)
    for syn in (a, b):
        if loud:
            syn.set_master_loudness(SR, 48, 64)
    r = Res(L, M, s2.resampler_design(L, M, T))
    m = Stage(16, "tpdf", _taps(K), seed=40 + K)
    r.set(a)
    m.set(a)
    calls = [300, 1, 1, 1, 1023, 64, 1024] if (L, M) == (1, 4) else [300, 1, TILE * M // L + 1, 1024, 7]
    zero = 0
    for fill, n in enumerate(calls):
        _events((a, b), V, fill)
        _rfill(a, b, r, n, 8 if fill % 2 else 3, "%d/%d with %d taps behind, fill %d" % (L, M, K, fill), state=True, loudness=loud, pcm=m)
        zero += r.out.shape[1] == 0
        assert m.t == r.made
    assert zero == (2 if (L, M) == (1, 4) else 0)
    assert np.unique(m.pcm[MASTER]).size > 4
    # the resampler off again: the PCM stage goes on from its state over the stems and the master themselves
    a.clear_master_resampler()
    _events((a, b), V, 9)
    x, st_b = b.sample_master(500, SR, 3)
    m.expect(st_b, x)
    assert_bits_equal_finite(a.sample_master(500, SR, 3)[0], x, "master")
    m.check(a, "the PCM stage alone again", state=True)


@pytest.mark.parametrize("then", ["clear", "a smaller ratio"])
def test_the_pcm_samples_stay_readable_when_their_converter_goes(then):
    """a fill of max_frames behind 4/1 leaves the PCM stage four times max_frames samples; the converter is then cleared, or replaced
    by 1/2, and until the next master fill pcm() still returns those samples, of every programme (s2r.h: they are held; Synth.pcm
    once sized its buffer by the converter that is set now and was refused — found by the post-mix walks, seeds 500030 and 500211)"""
    (a, b), _ = _quiet(64)
    r = Res(4, 1, s2.resampler_design(4, 1, 8))
    m = Stage(16, "tpdf", _taps(5), seed=3)
    r.set(a)
    m.set(a)
    _events((a, b), V, 0)
    _rfill(a, b, r, 64, 3, "in front of the %s" % then, pcm=m)
    assert m.pcm.shape == (P, 256, 2)
    if then == "clear":
        a.clear_master_resampler()
    else:
        a.set_master_resampler(1, 2, s2.resampler_design(1, 2, 8))
    m.check(a, "behind the %s" % then, state=True)
    assert_bits_equal_finite(a.sample_buses(64, SR, 3), b.sample_buses(64, SR, 3), "a bus fill behind the %s" % then)
    m.check(a, "behind the %s and a bus fill" % then)


def test_bus_count_stages_events_and_slices(monkeypatch):
    """a bus count that changes between calls (a bus that drops out is fed +0.0 and its history rings out), a reverb, an EQ and a delay
    in front of the stage on both handles, timed events inside the fills, a rows buffer of 48 frames so that the stems arrive in slices"""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    (a, b), _ = _quiet(1024)
    for syn in (a, b):
        syn.set_bus_reverb(0, _ir(40, 3), 0.5, 0.5)
        syn.set_bus_delay(1, 100, 0.5, 0.25, 0.7, 0.3)
        syn.set_bus_eq(2, np.stack([s2.eq_design(s2.EQ_PEAK, 900.0, 6.0, 1.0, SR)]))
    r = Res(147, 160, s2.resampler_design(147, 160, 32))
    r.set(a)
    for fill, (nb, n) in enumerate([(8, 300), (2, 20), (5, 1024), (1, 99), (8, 101)]):
        _events((a, b), V, fill)
        for syn in (a, b):
            syn.note_events(np.array([(ON, 50 + fill, (n // 2) & ~15, 0.8)], dtype=s2.NOTE_EVENT_DTYPE))
        _rfill(a, b, r, n, nb, "fill %d: %d buses, %d frames" % (fill, nb, n), state=True)
        if fill == 1:
            assert ubits(r.out[2:MASTER]).any()                  # the buses that dropped out ring out through the 31 frames of history
    assert r.made == (1544 * 147 + 159) // 160


def test_checkpoint_reset_clear_and_set_again():
    """parameters, history and ph into a third handle in the middle of a stream: the continuations are equal.  reset: state and ph as
    after a set, the parameters kept.  clear: off, every entry that needs the stage refuses; a bus fill or a panned fill between two
    master fills moves nothing; set again with more taps and a larger ratio regrows the buffers and starts from +0.0"""
    (a, b), _ = _quiet(512)
    r = Res(2, 3, s2.resampler_design(2, 3, 24))
    r.set(a)
    L, h = a.L, a.h
    buf = np.zeros(2 * 4096, dtype=F)
    bp, n_got = buf.ctypes.data_as(s2s._f32p), C.c_size_t()
    assert L.s2r_get_resampled(h, MASTER, bp, buf.size, C.byref(n_got)) == s2s.S2R_ERR_INVALID       # before any fill that ran the stage
    for fill, n in enumerate([400, 511, 333]):
        _events((a, b), V, fill)
        _rfill(a, b, r, n, 4, "before the checkpoint, fill %d" % fill)
    st, ph = a.resampler_state()
    assert ph == r.ph == (-(1244 * 2)) % 3
    rl, rm, table = a.get_master_resampler()
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    c = s2.Synth(V, max_frames=512, block_voices=64)
    c.set_patch_bank(_bank())
    c.import_state(state)
    c.set_voice_pans(pans)
    c.set_voice_mix(gains, buses)
    c.set_voice_sends(sends, sbuses)
    c.set_master_resampler(rl, rm, table)
    c.set_resampler_state(st, ph)
    for k, n in enumerate([100, 512, 1]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        x, _ = _rfill(a, b, r, n, 4, "the checkpointed handle, fill %d" % k, state=k == 2)
        assert_bits_equal_finite(c.sample_master(n, SR, 4)[0], x, "the resumed handle, fill %d" % k)
        for p in range(P):
            assert_bits_equal_finite(c.resampled(p), r.out[p], "the resumed handle's outputs, fill %d" % k)
    assert_bits_equal_finite(c.resampler_state()[0], a.resampler_state()[0], "state at the end")
    before = a.resampler_state()
    _events((a, b), V, 10)
    assert_bits_equal_finite(a.sample_buses(64, SR, 8), b.sample_buses(64, SR, 8), "a bus fill beside the stage")
    assert_bits_equal_finite(a.sample_panned(64, SR), b.sample_panned(64, SR), "a panned fill beside the stage")
    assert_bits_equal_finite(a.resampler_state()[0], before[0], "state after other fills")
    assert a.resampler_state()[1] == before[1]
    assert_bits_equal_finite(a.resampled(MASTER), r.out[MASTER], "the last outputs after other fills")
    a.reset_master_resampler()
    r.reset()
    assert a.get_master_resampler()[:2] == (2, 3)
    st, ph = a.resampler_state()
    assert ph == 0 and not ubits(st).any()
    assert L.s2r_get_resampled(h, MASTER, bp, buf.size, C.byref(n_got)) == s2s.S2R_ERR_INVALID
    _events((a, b), V, 2)
    _rfill(a, b, r, 500, 8, "after the reset", state=True)
    a.clear_master_resampler()
    assert a.get_master_resampler() == (0, 0, None)
    _events((a, b), V, 3)
    x, st_b = b.sample_master(300, SR, 8)
    got, st = a.sample_master(300, SR, 8)
    assert_bits_equal_finite(got, x, "after clear_master_resampler: master")
    assert_bits_equal_finite(st, st_b, "after clear_master_resampler: stems")
    z = np.zeros(CH * 127, dtype=F)
    zp = z.ctypes.data_as(s2s._f32p)
    for rc in (L.s2r_get_resampler_state(h, zp, z.size, None), L.s2r_set_resampler_state(h, zp, CH * 23, 0), L.s2r_reset_master_resampler(h),
               L.s2r_get_resampled(h, MASTER, bp, buf.size, C.byref(n_got))):
        assert rc == s2s.S2R_ERR_INVALID
    r = Res(4, 1, s2.resampler_design(4, 1, 128))                # off, then on with more taps and four times the frames: the initial state
    r.set(a)
    _events((a, b), V, 4)
    _rfill(a, b, r, 300, 8, "set again", state=True)
    _rfill(a, b, r, 512, 8, "set again, the second fill", state=True)
    assert r.out.shape[1] == 2048 and r.made == 4 * 812


def test_forty_calls_cut_three_ways_give_the_same_outputs():
    """three handles with the stage render the same 10 240 frames in 40 calls each, of lengths mixed three ways (every cut at a
    multiple of 16 frames, where a split fill renders the same bits: the masters are compared first): the outputs of every programme,
    the state and ph are equal"""
    hs, _ = _quiet(1024, n=3)
    cuts = ([256] * 40, [16, 496, 128, 384] * 10, [1008, 16, 272, 240, 64, 160, 144, 144] * 5)
    table = s2.resampler_design(147, 160, 32)
    runs = []
    for syn, cut in zip(hs, cuts):
        syn.set_master_resampler(147, 160, table)
        _events((syn,), V, 0)
        assert sum(cut) == 10240 and len(cut) == 40
        masters, outs = [], []
        for n in cut:
            masters.append(syn.sample_master(n, SR, 8, stems=False)[0])
            outs.append(np.stack([syn.resampled(p) for p in range(P)]))
        runs.append((np.concatenate(masters), np.concatenate(outs, axis=1)))
    assert runs[0][1].shape == (P, 9408, 2) and np.abs(runs[0][1]).max(axis=(1, 2)).all()
    for syn, (x, out) in zip(hs[1:], runs[1:]):
        assert_bits_equal_finite(x, runs[0][0], "the master, another cut")
        assert_bits_equal_finite(out, runs[0][1], "the outputs, another cut")
        assert_bits_equal_finite(syn.resampler_state()[0], hs[0].resampler_state()[0], "state, another cut")
        assert syn.resampler_state()[1] == hs[0].resampler_state()[1] == 0


def test_refusals_change_nothing():
    """refused master fills and refused setters leave parameters, state, ph and the outputs as they were, and the next fill equals
    the reference as if they had not happened; a device-list handle refuses every entry"""
    (a, b), _ = _quiet(256)
    r = Res(2, 3, s2.resampler_design(2, 3, 8))
    r.set(a)
    for fill in range(2):
        _events((a, b), V, fill)
        _rfill(a, b, r, 250, 2, "before the refusals, fill %d" % fill)
    L, h = a.L, a.h
    out, st = np.full(2 * 300, 7.0, dtype=F), np.full(2 * 2 * 300, 7.0, dtype=F)
    op, sp = out.ctypes.data_as(s2s._f32p), st.ctypes.data_as(s2s._f32p)
    good = np.zeros(320 * 128, dtype=F)
    gp = good.ctypes.data_as(s2s._f32p)
    nan, big = np.zeros(16, dtype=F), np.zeros(16, dtype=F)
    nan[3], big[15] = np.nan, 4.5
    zeros = np.zeros(CH * 7 + 1, dtype=F)
    zp = zeros.ctypes.data_as(s2s._f32p)
    buf = np.full(2 * 256, 7.0, dtype=F)
    bp, n_got = buf.ctypes.data_as(s2s._f32p), C.c_size_t(7)
    R, I = s2s.S2R_ERR_PATCH_RANGE, s2s.S2R_ERR_INVALID
    refusals = [
        ("no bus", lambda: L.s2r_fill_master(h, op, sp, st.size, 0, 64, SR), I),
        ("nine buses", lambda: L.s2r_fill_master(h, op, sp, st.size, 9, 64, SR), I),
        ("too many frames", lambda: L.s2r_fill_master(h, op, sp, st.size, 2, 257, SR), s2s.S2R_ERR_TOO_MANY_FRAMES),
        ("L 0", lambda: L.s2r_set_master_resampler(h, 0, 1, 8, gp), R),
        ("M 0", lambda: L.s2r_set_master_resampler(h, 1, 0, 8, gp), R),
        ("L 321", lambda: L.s2r_set_master_resampler(h, 321, 320, 8, gp), R),
        ("M 321", lambda: L.s2r_set_master_resampler(h, 320, 321, 8, gp), R),
        ("a common factor", lambda: L.s2r_set_master_resampler(h, 4, 6, 8, gp), R),
        ("a ratio of 5", lambda: L.s2r_set_master_resampler(h, 5, 1, 8, gp), R),
        ("a ratio of 1/5", lambda: L.s2r_set_master_resampler(h, 1, 5, 8, gp), R),
        ("no taps", lambda: L.s2r_set_master_resampler(h, 2, 3, 0, gp), R),
        ("six taps", lambda: L.s2r_set_master_resampler(h, 2, 3, 6, gp), R),
        ("132 taps", lambda: L.s2r_set_master_resampler(h, 2, 3, 132, gp), R),
        ("a table of 24 704", lambda: L.s2r_set_master_resampler(h, 193, 175, 128, gp), R),
        ("a NaN", lambda: L.s2r_set_master_resampler(h, 2, 3, 8, nan.ctypes.data_as(s2s._f32p)), R),
        ("an entry of 4.5", lambda: L.s2r_set_master_resampler(h, 2, 3, 8, big.ctypes.data_as(s2s._f32p)), R),
        ("a null table", lambda: L.s2r_set_master_resampler(h, 2, 3, 8, None), I),
        ("a short state", lambda: L.s2r_set_resampler_state(h, zp, CH * 7 - 1, 0), I),
        ("a long state", lambda: L.s2r_set_resampler_state(h, zp, CH * 7 + 1, 0), I),
        ("a null state", lambda: L.s2r_set_resampler_state(h, None, CH * 7, 0), I),
        ("ph at M", lambda: L.s2r_set_resampler_state(h, zp, CH * 7, 3), R),
        ("a small state buffer", lambda: L.s2r_get_resampler_state(h, zp, CH * 7 - 1, None), I),
        ("programme 9", lambda: L.s2r_get_resampled(h, 9, bp, buf.size, C.byref(n_got)), R),
        ("a small output buffer", lambda: L.s2r_get_resampled(h, MASTER, bp, 2 * r.out.shape[1] - 1, C.byref(n_got)), I),
        ("a null output buffer", lambda: L.s2r_get_resampled(h, MASTER, None, buf.size, C.byref(n_got)), I),
    ]
    for fill, (name, call, status) in enumerate(refusals):
        assert call() == status, name
        assert (out == 7.0).all() and (st == 7.0).all() and not zeros.any() and (buf == 7.0).all() and n_got.value == 7, name
        r.check(a, name, state=True)
        got = a.get_master_resampler()
        assert got[:2] == (2, 3) and ubits(got[2]).tolist() == ubits(r.table).tolist(), name
        if fill % 8 == 0:
            _events((a, b), V, fill + 3)
            _rfill(a, b, r, 250, 2, "after the refusal: " + name)
    a.sample_begin(64, SR)
    assert L.s2r_fill_master(h, op, sp, st.size, 2, 64, SR) == I
    assert (out == 7.0).all()
    b.sample(np.empty(64, dtype=F), SR)
    a.sample_end(np.empty(64, dtype=F))
    _events((a, b), V, 40)
    _rfill(a, b, r, 64, 2, "after the fill in flight", state=True)
    # a device list refuses every entry
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    Ml, mh = multi.L, multi.h
    u = C.c_uint32()
    assert Ml.s2r_set_master_resampler(mh, 2, 3, 8, gp) == I
    assert Ml.s2r_clear_master_resampler(mh) == I
    assert Ml.s2r_get_master_resampler(mh, C.byref(u), C.byref(u), C.byref(u), None) == I
    assert Ml.s2r_reset_master_resampler(mh) == I
    assert Ml.s2r_get_resampled(mh, 0, bp, buf.size, C.byref(n_got)) == I
    assert Ml.s2r_get_resampler_state(mh, zp, CH * 7, C.byref(u)) == I
    assert Ml.s2r_set_resampler_state(mh, zp, CH * 7, 0) == I
    assert Ml.s2r_set_master_resampler(mh, 0, 3, 8, gp) == R     # the values are looked at first
    assert not zeros.any() and (buf == 7.0).all() and not good.any()


def test_timing_entry_and_a_handle_that_never_set_the_stage():
    """s2r_debug_resampler_ms: -1 without s2r_set_timing; under it the resampler kernel's time of the last master fill, 0 when that
    fill ran none.  A handle on which the stage was never set holds nothing of it after a master fill."""
    (a, _), _ = _quiet(512)
    ms, pms, alloc = a.L.s2r_debug_resampler_ms, a.L.s2r_debug_pcm_ms, a.L.s2r_debug_resampler_allocated
    for f in (ms, pms):
        f.restype, f.argtypes = C.c_float, [C.c_void_p]
    alloc.restype, alloc.argtypes = C.c_int, [C.c_void_p]
    _events((a,), V, 0)
    a.sample_master(300, SR, 2)
    assert alloc(a.h) == 0
    a.set_master_resampler(1, 4, s2.resampler_design(1, 4, 16))
    assert alloc(a.h) == 0                                       # (the first master fill that finds it set allocates)
    a.sample_master(301, SR, 2)
    assert alloc(a.h) == 1 and ms(a.h) == -1.0
    a.set_timing(True)
    a.set_master_pcm(16, "tpdf", 5)
    a.sample_master(1, SR, 2)                                    # ph is 3: no output, so no PCM kernel
    assert a.resampled().shape == (0, 2) and a.pcm().shape == (0, 2)
    assert 0.0 < ms(a.h) < 100.0 and pms(a.h) == 0.0
    a.sample_master(300, SR, 2)
    assert 0.0 < ms(a.h) < 100.0 and 0.0 < pms(a.h) < 100.0 and a.pcm().shape == a.resampled().shape == (75, 2)
    a.clear_master_resampler()
    a.sample_master(300, SR, 2)
    assert ms(a.h) == 0.0 and a.pcm().shape == (300, 2)
