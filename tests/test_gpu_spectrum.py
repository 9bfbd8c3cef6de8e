"""The spectrum meters on the device.  Twin handles are fed the same events, one with the meter and one without: the
twin's sample_master gives the stems and the master, which the metered handle must return in the same bits, and the expectation for
the rows and the state is s2r_spectrum_reference over the twin's output, with state, position and rows carried from call to call in
numpy (tests/test_spectrum_host.py holds that function to a numpy model of the rule).

Handles, events and the one-pole bank are tests/test_gpu_reverb.py's on 32-voice pools, max_frames 1024 or 2048.  Every comparison is
on bits with no NaN allowance.  The kernel runs one workgroup per row and programme, whatever the call's length, so its edges are the
hop's (a call that ends one frame before, on and after one), the size's (a row that lies in the history alone, across both sources,
in the call alone) and the passes': every log2 N of 8 .. 13, whose layers the kernel splits into passes of 4 4 | 3 3 3 | 4 3 3 |
4 4 3 | 4 4 4 | 4 3 3 3 — N = 1024 alone runs with 128 threads, N = 4096 alone with 512 and alone runs a pass of four layers at
s0 = 8.  The matrix, the crafted histories and the walk from size to size on one handle run all six; tests/test_gpu_post_fuzz.py
sets, replaces and checkpoints meters of all six behind a chain in mid-state."""
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
P = s2.SPECTRUM_PROGRAMMES
MASTER = s2.MAX_BUSES


def _window(kind, n):
    if kind == "random":
        return np.random.default_rng(n).uniform(-1, 1, n).astype(F)
    return s2.spectrum_window(kind, n)


class Meter:
    """the meter of a handle in numpy: parameters, the carried state and position, the window of rows"""

    def __init__(self, n, hop, window="hann", max_rows=8):
        self.n, self.hop, self.max_rows = n, hop, max_rows
        self.w = _window(window, n) if isinstance(window, str) else np.asarray(window, dtype=F)
        self.reset()

    def reset(self):
        self.state, self.pos = np.zeros((P, self.n, 2), dtype=F), 0
        self.rows = np.zeros((0, P, self.n // 2 + 1), dtype=F)
        self.made = 0

    def set(self, *handles):
        for syn in handles:
            syn.set_master_spectrum(self.n, self.hop, self.w, self.max_rows)
            n, hop, max_rows, k, w = syn.get_master_spectrum()
            assert (n, hop, max_rows, k) == (self.n, self.hop, self.max_rows, 0)
            assert_bits_equal_finite(w, self.w, "the window read back")
        self.reset()

    def expect(self, stems, x):
        rows, self.state, self.pos = s2.spectrum_reference(self.n, self.hop, self.w, stems, x, self.state, self.pos)
        assert np.isfinite(rows).all()
        self.made += len(rows)
        self.rows = np.concatenate([self.rows, rows])[-self.max_rows:]

    def check(self, syn, what, state=False):
        assert syn.get_master_spectrum()[3] == len(self.rows), what
        assert_bits_equal_finite(syn.spectrum_rows(), self.rows, what + ": rows")
        if state:                                                # (a read fetches the state, and the next fill sends it back: not after every call)
            st, pos = syn.spectrum_state()
            assert pos == self.pos, what
            assert_bits_equal_finite(st, self.state, what + ": state")


def _mfill(a, b, m, n, nb, what, stems=True, state=False):
    """one call on both handles: the metered handle returns the twin's bits, and its rows and (on request) state are the reference's
    over the twin's stems and master"""
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


@pytest.mark.parametrize("loudness", [False, True])
@pytest.mark.parametrize("limiter", [False, True])
def test_output_is_unchanged(limiter, loudness):
    """master and stems of the metered handle are the twin's bits — with and without a limiter, with and without the loudness meter,
    with and without stems —, and with the loudness meter on both its hop rows, state and true peak are the same bits"""
    a, b = _handles(V, max_frames=1024)
    if limiter:
        c = _handles(V, max_frames=1024)[1]                      # (a ceiling the limiter has to work for, from a handle of its own)
        _events((c,), V, 0)
        ceiling = float(np.abs(c.sample_master(1024, SR, 8)[0]).max()) * 0.25
        for syn in (a, b):
            syn.set_master_limiter(ceiling, 48, 100)
    if loudness:
        for syn in (a, b):
            syn.set_master_loudness(SR, 48, 32)
    m = Meter(512, 128)
    m.set(a)
    for fill, n in enumerate([300, 1024, 17, 256, 1000]):
        _events((a, b), V, fill)
        _mfill(a, b, m, n, 8, "limiter %s, loudness %s, fill %d of %d frames" % (limiter, loudness, fill, n), stems=fill % 2 == 0, state=fill in (1, 4))
        if loudness:
            assert_bits_equal_finite(a.loudness_hops(), b.loudness_hops(), "loudness rows beside the spectrum")
            assert_bits_equal_finite(a.true_peak()[1], b.true_peak()[1], "true peak beside the spectrum")
    if loudness:
        assert_bits_equal_finite(a.loudness_state()[0], b.loudness_state()[0], "loudness state beside the spectrum")
        assert len(a.loudness_hops()) >= 30
    assert m.made >= 20 and (m.rows[-1] > 0.0).all()
    if limiter:
        assert a.limiter_meters()[0] < 1.0


# every log2 N of 8 .. 13: N = 1024 is the one size of 128 threads and passes 4, 3, 3; N = 4096 the one of 512 threads and passes 4, 4, 4
MATRIX = [(1, 256, 32), (2, 512, 384), (2, 1024, 128), (3, 2048, 512), (3, 4096, 512), (8, 8192, 1024), (2, 256, 1000)]


@pytest.mark.parametrize("window", ["hann", "random"])
@pytest.mark.parametrize("nb,n,hop", MATRIX)
def test_rows_and_state_are_the_reference(nb, n, hop, window):
    """the parity matrix, max_frames 2048: calls of 1 to 5 frames, of hop - 1, hop and hop + 1, of N - 1, N and N + 1 (where 2048
    allows), of 1023, 1024, 2047 and 2048 frames; events between the calls, every other call without stems; the pans of
    _handles differ per program, so L != R"""
    a, b = _handles(V, max_frames=2048)
    m = Meter(n, hop, window)
    m.set(a)
    what = "%d buses, N %d, hop %d, %s" % (nb, n, hop, window)
    calls = [1, 2, 3, 4, 5, hop - 1, hop, hop + 1] + [c for c in (n - 1, n, n + 1) if c <= 2048] + [1023, 1024, 2047, 2048]
    for fill, c in enumerate(calls):
        _events((a, b), V, fill)
        x, st = _mfill(a, b, m, c, nb, "%s, fill %d of %d frames" % (what, fill, c), stems=fill % 2 == 0, state=fill in (4, 7, len(calls) - 1))
    assert not np.array_equal(x[:, 0], x[:, 1]) and m.made >= 2
    last = m.rows[-1]
    assert (last[:nb] > 0.0).any(axis=1).all() and not ubits(m.rows[:, nb:MASTER]).any() and (last[MASTER] > 0.0).any()


@pytest.mark.parametrize("n,hop", [(256, 64), (1024, 128), (2048, 512), (4096, 512), (8192, 1024)])
def test_crafted_histories(n, hop):
    """set_spectrum_state loads a unit impulse at several positions of several programmes, then random finite values, then denormals;
    one silent frame completes a hop.  Rows are the reference's bits; an impulse of 1 on L at frame i of the row reads
    p[k] = window[i]^2 in every bin, checked without the reference: the impulse passes at most log2 N twiddle products, each off by at
    most 3 ulps in magnitude with the twiddle's own rounding, the power doubles that and adds three operations —
    (6 log2 N + 3) * 2^-24 < 1e-5 relative."""
    a, b = _handles(V, max_frames=1024)                          # (no events: every programme is silent)
    m = Meter(n, hop, "random")
    m.set(a)
    rng = np.random.default_rng(n)
    L = n.bit_length() - 1
    assert (6 * L + 3) * 2.0 ** -24 < 1e-5
    for i in (1, 2, n // 2 + 1, n - 2, n - 1):
        st = np.zeros((P, n, 2), dtype=F)
        for p in (0, 2, MASTER):
            st[p, i, 0] = 1.0
        a.set_spectrum_state(st, hop - 1)
        m.state, m.pos = st.copy(), hop - 1
        x, _ = _mfill(a, b, m, 1, 3, "impulse at %d" % i, state=True)
        assert not ubits(x).any() or not x.any()
        row = a.spectrum_rows()[-1]
        w2 = float(m.w[i - 1]) ** 2
        for p in (0, 2, MASTER):
            np.testing.assert_allclose(row[p].astype(np.float64), w2, rtol=1e-5, atol=0)
        assert not ubits(row[1]).any()
    for scale, name in ((1.0, "random"), (2.0 ** -130, "denormal")):
        st = (rng.uniform(-1, 1, (P, n, 2)) * scale).astype(F)
        if scale < 1:
            assert (np.abs(st) < np.finfo(F).tiny).all() and st.any()
        a.set_spectrum_state(st, hop - 1)
        m.state, m.pos = st.copy(), hop - 1
        _mfill(a, b, m, 1, 8, name + " history", state=True)
        _mfill(a, b, m, hop, 8, name + " history, the next hop", state=True)
    assert m.made == 9


def test_bus_count_stages_events_and_slices(monkeypatch):
    """a bus count that changes between calls (a bus that drops out is fed +0.0 and keeps its history), a reverb, an EQ and a delay in
    front of the meter on both handles, timed events inside the fills, a rows buffer of 48 frames so that the stems arrive in slices,
    and buses past n_buses read +0.0 rows"""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    a, b = _handles(V, max_frames=1024)
    for syn in (a, b):
        syn.set_bus_reverb(0, _ir(40, 3), 0.5, 0.5)
        syn.set_bus_delay(1, 100, 0.5, 0.25, 0.7, 0.3)
        syn.set_bus_eq(2, np.stack([s2.eq_design(s2.EQ_PEAK, 900.0, 6.0, 1.0, SR)]))
    m = Meter(256, 100, "random")
    m.set(a)
    for fill, (nb, n) in enumerate([(8, 300), (2, 150), (5, 1024), (1, 99), (8, 101)]):
        _events((a, b), V, fill)
        for syn in (a, b):
            syn.note_events(np.array([(ON, 50 + fill, (n // 2) & ~15, 0.8)], dtype=s2.NOTE_EVENT_DTYPE))
        _mfill(a, b, m, n, nb, "fill %d: %d buses, %d frames" % (fill, nb, n), state=True)
        if len(m.rows):
            assert not ubits(m.rows[-1, nb:MASTER]).any()
    assert m.made == 16


def test_checkpoint_in_the_middle_of_a_hop():
    """voices, pans, mix, sends and the meter — parameters, state and position in the middle of a hop, the stored rows — into a third
    handle: the continuations are equal on bits, equal to the reference, and read the same spectrum"""
    a, b = _handles(V, max_frames=512)
    m = Meter(512, 200, "hann", 6)
    m.set(a)
    for fill, n in enumerate([400, 512, 333]):
        _events((a, b), V, fill)
        _mfill(a, b, m, n, 4, "before the checkpoint, fill %d" % fill)
    st, pos = a.spectrum_state()
    rows = a.spectrum_rows()
    assert pos == 45 and len(rows) == 6
    n_fft, hop, max_rows, _, w = a.get_master_spectrum()
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    c = s2.Synth(V, max_frames=512, block_voices=64)
    c.set_patch_bank(_bank())
    c.import_state(state)
    c.set_voice_pans(pans)
    c.set_voice_mix(gains, buses)
    c.set_voice_sends(sends, sbuses)
    c.set_master_spectrum(n_fft, hop, w, max_rows)
    c.set_spectrum_state(st, pos)
    c.set_spectrum_rows(rows)
    got_st, got_pos = c.spectrum_state()
    assert got_pos == pos
    assert_bits_equal_finite(got_st, st, "the restored state read back")
    assert_bits_equal_finite(c.spectrum_rows(), rows, "the restored rows read back")
    for k, n in enumerate([100, 512, 155, 400]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        x, _ = _mfill(a, b, m, n, 4, "the checkpointed handle, fill %d" % k, state=k == 3)
        assert_bits_equal_finite(c.sample_master(n, SR, 4)[0], x, "the resumed handle, fill %d" % k)
        assert_bits_equal_finite(c.spectrum_rows(), m.rows, "the resumed handle's rows, fill %d" % k)
    for p in (0, 3, MASTER):
        assert np.array_equal(c.spectrum(p, 2), a.spectrum(p, 2))
        assert np.array_equal(a.spectrum(p, 2), s2.spectrum_readings(m.rows, m.w, p, 2))
    assert_bits_equal_finite(c.spectrum_state()[0], a.spectrum_state()[0], "state at the end")


def test_reset_and_clear():
    """reset: state and rows as after a set, the parameters kept.  clear: off, the handle's fills equal the twin's, every entry that
    needs a meter refuses; a bus fill or a panned fill between two master fills moves nothing; set again starts from +0.0"""
    a, b = _handles(V, max_frames=1024)
    m = Meter(256, 48)
    m.set(a)
    for fill, n in enumerate([500, 333]):
        _events((a, b), V, fill)
        _mfill(a, b, m, n, 8, "before the reset, fill %d" % fill)
    before = (a.spectrum_rows(), a.spectrum_state())
    _events((a, b), V, 10)
    assert_bits_equal_finite(a.sample_buses(64, SR, 8), b.sample_buses(64, SR, 8), "a bus fill beside the meter")
    assert_bits_equal_finite(a.sample_panned(64, SR), b.sample_panned(64, SR), "a panned fill beside the meter")
    assert_bits_equal_finite(a.spectrum_rows(), before[0], "rows after other fills")
    assert_bits_equal_finite(a.spectrum_state()[0], before[1][0], "state after other fills")
    assert a.spectrum_state()[1] == before[1][1]
    a.reset_master_spectrum()
    m.reset()
    assert a.get_master_spectrum()[:4] == (256, 48, 8, 0)
    st, pos = a.spectrum_state()
    assert pos == 0 and not ubits(st).any()
    _events((a, b), V, 2)
    _mfill(a, b, m, 700, 8, "after the reset", state=True)
    a.clear_master_spectrum()
    assert a.get_master_spectrum()[:4] == (0, 0, 0, 0)
    _events((a, b), V, 3)
    x, st_b = b.sample_master(300, SR, 8)
    got, st = a.sample_master(300, SR, 8)
    assert_bits_equal_finite(got, x, "after clear_master_spectrum: master")
    assert_bits_equal_finite(st, st_b, "after clear_master_spectrum: stems")
    L, h, z = a.L, a.h, np.zeros(16, dtype=F)
    zp, d = z.ctypes.data_as(s2s._f32p), (C.c_double * 16)()
    for rc in (L.s2r_get_spectrum_state(h, zp, 16, None), L.s2r_get_spectrum_rows(h, zp, 16, None), L.s2r_reset_master_spectrum(h),
               L.s2r_get_spectrum(h, 0, 1, d, 16), L.s2r_get_spectrum_bands(h, 0, 1, 48000.0, 3, d, None, 16, C.byref(C.c_size_t())),
               L.s2r_set_spectrum_state(h, zp, 16, 0), L.s2r_set_spectrum_rows(h, zp, 0, 0)):
        assert rc == s2s.S2R_ERR_INVALID
    m = Meter(2048, 256, "hamming", 3)                           # off, then on with a larger size: the initial state, larger buffers
    m.set(a)
    _events((a, b), V, 4)
    _mfill(a, b, m, 300, 8, "set again", state=True)
    _mfill(a, b, m, 1024, 8, "set again, the second fill", state=True)
    assert m.made == 5 and len(m.rows) == 3


def test_a_larger_size_and_the_smaller_one_again():
    """the state's two device copies are sized by the first fill, regrown by the fill behind a set at a larger size and used as they
    are behind a set at the smaller size again: sizes 256 (hop 32), 512 (hop 64), 1024 (hop 128), 4096 (hop 512), 1024 and 256 on one
    handle, two master fills of two buses each — so the two sizes whose split into passes no other size shares (4 3 3 and 4 4 4) run
    on copies that were sized for another transform, growing and as they are.  Every set leaves no rows and a state of +0.0 at
    position 0; every fill returns the bits of a twin that never had a meter, and rows and state are the reference's bits, compared
    as in test_rows_and_state_are_the_reference.  601 frames make 18 and 9 rows at the two small sizes, which fill the window of 8,
    4 at 1024 and one at 4096."""
    a, b = _handles(V, max_frames=512)
    fill = 0
    for n, hop in ((256, 32), (512, 64), (1024, 128), (4096, 512), (1024, 128), (256, 32)):
        m = Meter(n, hop)
        m.set(a)
        assert a.spectrum_rows().size == 0
        st, pos = a.spectrum_state()
        assert pos == 0 and st.size == 2 * P * n and not ubits(st).any()
        for frames in (300, 301):
            _events((a, b), V, fill)
            _mfill(a, b, m, frames, 2, "N %d, fill %d of %d frames" % (n, fill, frames), stems=fill % 2 == 0, state=True)
            fill += 1
        assert m.made == 601 // hop >= 1 and len(m.rows) == min(8, m.made) and (m.rows[-1, [0, 1, MASTER]] > 0.0).any(axis=1).all()
        assert n > 512 or len(m.rows) == 8


def test_refusals_change_nothing():
    """refused master fills and refused setters leave parameters, state, rows and readings as they were, and the next fill equals the
    reference as if they had not happened; a device-list handle refuses every entry"""
    a, b = _handles(V, max_frames=256)
    m = Meter(256, 32, "hann", 4)
    m.set(a)
    for fill in range(2):
        _events((a, b), V, fill)
        _mfill(a, b, m, 250, 2, "before the refusals, fill %d" % fill)
    L, h = a.L, a.h
    out, st = np.full(2 * 300, 7.0, dtype=F), np.full(2 * 2 * 300, 7.0, dtype=F)
    op, sp = out.ctypes.data_as(s2s._f32p), st.ctypes.data_as(s2s._f32p)
    good = m.w.copy()
    gp = good.ctypes.data_as(s2s._f32p)
    nan = good.copy(); nan[3] = np.nan
    inf = good.copy(); inf[255] = np.inf
    row = 9 * 129
    zeros = np.zeros(max(18 * 256 + 1, 5 * row), dtype=F)
    zp = zeros.ctypes.data_as(s2s._f32p)
    d = (C.c_double * 129)()
    nbands = C.c_size_t()
    refusals = [
        ("no bus", lambda: L.s2r_fill_master(h, op, sp, st.size, 0, 64, SR), s2s.S2R_ERR_INVALID),
        ("nine buses", lambda: L.s2r_fill_master(h, op, sp, st.size, 9, 64, SR), s2s.S2R_ERR_INVALID),
        ("too many frames", lambda: L.s2r_fill_master(h, op, sp, st.size, 2, 257, SR), s2s.S2R_ERR_TOO_MANY_FRAMES),
        ("size 128", lambda: L.s2r_set_master_spectrum(h, 128, 32, gp, 4), s2s.S2R_ERR_PATCH_RANGE),
        ("size 16384", lambda: L.s2r_set_master_spectrum(h, 16384, 2048, gp, 4), s2s.S2R_ERR_PATCH_RANGE),
        ("size 384", lambda: L.s2r_set_master_spectrum(h, 384, 64, gp, 4), s2s.S2R_ERR_PATCH_RANGE),
        ("hop 31", lambda: L.s2r_set_master_spectrum(h, 256, 31, gp, 4), s2s.S2R_ERR_PATCH_RANGE),
        ("hop past the range", lambda: L.s2r_set_master_spectrum(h, 256, (1 << 20) + 1, gp, 4), s2s.S2R_ERR_PATCH_RANGE),
        ("no rows", lambda: L.s2r_set_master_spectrum(h, 256, 32, gp, 0), s2s.S2R_ERR_PATCH_RANGE),
        ("257 rows", lambda: L.s2r_set_master_spectrum(h, 256, 32, gp, 257), s2s.S2R_ERR_PATCH_RANGE),
        ("a NaN", lambda: L.s2r_set_master_spectrum(h, 256, 32, nan.ctypes.data_as(s2s._f32p), 4), s2s.S2R_ERR_PATCH_RANGE),
        ("an infinity", lambda: L.s2r_set_master_spectrum(h, 256, 32, inf.ctypes.data_as(s2s._f32p), 4), s2s.S2R_ERR_PATCH_RANGE),
        ("a null window", lambda: L.s2r_set_master_spectrum(h, 256, 32, None, 4), s2s.S2R_ERR_INVALID),
        ("a short state", lambda: L.s2r_set_spectrum_state(h, zp, 18 * 256 - 1, 0), s2s.S2R_ERR_INVALID),
        ("a long state", lambda: L.s2r_set_spectrum_state(h, zp, 18 * 256 + 1, 0), s2s.S2R_ERR_INVALID),
        ("a null state", lambda: L.s2r_set_spectrum_state(h, None, 18 * 256, 0), s2s.S2R_ERR_INVALID),
        ("a position at the hop", lambda: L.s2r_set_spectrum_state(h, zp, 18 * 256, 32), s2s.S2R_ERR_PATCH_RANGE),
        ("rows of the wrong size", lambda: L.s2r_set_spectrum_rows(h, zp, 2, 2 * row - 1), s2s.S2R_ERR_INVALID),
        ("null rows", lambda: L.s2r_set_spectrum_rows(h, None, 2, 2 * row), s2s.S2R_ERR_INVALID),
        ("rows past the window", lambda: L.s2r_set_spectrum_rows(h, zp, 5, 5 * row), s2s.S2R_ERR_PATCH_RANGE),
        ("a small state buffer", lambda: L.s2r_get_spectrum_state(h, zp, 18 * 256 - 1, None), s2s.S2R_ERR_INVALID),
        ("a small rows buffer", lambda: L.s2r_get_spectrum_rows(h, zp, 4 * row - 1, None), s2s.S2R_ERR_INVALID),
        ("a small window buffer", lambda: L.s2r_get_master_spectrum(h, None, None, None, None, zp, 255), s2s.S2R_ERR_INVALID),
        ("programme 9", lambda: L.s2r_get_spectrum(h, 9, 1, d, 129), s2s.S2R_ERR_PATCH_RANGE),
        ("no rows to average", lambda: L.s2r_get_spectrum(h, 0, 0, d, 129), s2s.S2R_ERR_PATCH_RANGE),
        ("more rows than stored", lambda: L.s2r_get_spectrum(h, 0, 5, d, 129), s2s.S2R_ERR_PATCH_RANGE),
        ("a small reading buffer", lambda: L.s2r_get_spectrum(h, 0, 1, d, 128), s2s.S2R_ERR_INVALID),
        ("five bands per octave", lambda: L.s2r_get_spectrum_bands(h, 0, 1, 48000.0, 5, d, None, 129, C.byref(nbands)), s2s.S2R_ERR_PATCH_RANGE),
        ("a small band buffer", lambda: L.s2r_get_spectrum_bands(h, 0, 1, 48000.0, 3, d, None, 3, C.byref(nbands)), s2s.S2R_ERR_INVALID),
    ]
    assert len(m.rows) == 4
    for fill, (name, call, status) in enumerate(refusals):
        reading = a.spectrum(MASTER, 4)
        assert call() == status, name
        assert (out == 7.0).all() and (st == 7.0).all() and not zeros.any(), name
        m.check(a, name, state=True)
        assert np.array_equal(a.spectrum(MASTER, 4), reading), name
        assert a.get_master_spectrum()[:4] == (256, 32, 4, 4), name
        if fill % 6 == 0:
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
    u, z = C.c_uint32(), C.c_size_t()
    assert M.s2r_set_master_spectrum(mh, 256, 32, gp, 4) == s2s.S2R_ERR_INVALID
    assert M.s2r_clear_master_spectrum(mh) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_master_spectrum(mh, C.byref(u), C.byref(u), C.byref(u), C.byref(z), None, 0) == s2s.S2R_ERR_INVALID
    assert M.s2r_reset_master_spectrum(mh) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_spectrum(mh, 0, 1, d, 129) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_spectrum_bands(mh, 0, 1, 48000.0, 3, d, None, 129, C.byref(nbands)) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_spectrum_state(mh, zp, 18 * 256, C.byref(u)) == s2s.S2R_ERR_INVALID
    assert M.s2r_set_spectrum_state(mh, zp, 18 * 256, 0) == s2s.S2R_ERR_INVALID
    assert M.s2r_get_spectrum_rows(mh, zp, zeros.size, C.byref(z)) == s2s.S2R_ERR_INVALID
    assert M.s2r_set_spectrum_rows(mh, zp, 0, 0) == s2s.S2R_ERR_INVALID
    assert M.s2r_set_master_spectrum(mh, 128, 32, gp, 4) == s2s.S2R_ERR_PATCH_RANGE          # the values are looked at first
    assert not zeros.any()


def test_a_long_run_cut_three_ways_reads_the_same():
    """three metered handles render the same 12 288 frames in calls of 1024, of 1008, 16, 272 and 752, and of 16 and 2032 frames (every
    cut at a multiple of 16 frames, where a split fill renders the same bits: the masters are compared first): rows, state and the
    readings of every programme are the same bits, and spectrum() is spectrum_readings over spectrum_rows()"""
    hs = _handles(V, max_frames=2048, n=3)
    cuts = ([1024] * 12, [1008, 16, 272, 752] * 6, [16, 2032] * 6)
    masters = []
    for syn, cut in zip(hs, cuts):
        syn.set_master_spectrum(1024, 700, "blackman-harris", 12)
        _events((syn,), V, 0)
        assert sum(cut) == 12288
        masters.append(np.concatenate([syn.sample_master(n, SR, 8, stems=False)[0] for n in cut]))
    rows = hs[0].spectrum_rows()
    w = hs[0].get_master_spectrum()[4]
    assert rows.shape == (12, 9, 513) and (rows[-1] > 0.0).all()
    for syn, x in zip(hs[1:], masters[1:]):
        assert_bits_equal_finite(x, masters[0], "the master, another cut")
        assert_bits_equal_finite(syn.spectrum_rows(), rows, "rows, another cut")
        assert_bits_equal_finite(syn.spectrum_state()[0], hs[0].spectrum_state()[0], "state, another cut")
        assert syn.spectrum_state()[1] == hs[0].spectrum_state()[1] == 12288 % 700
    for p in range(P):
        r = hs[0].spectrum(p, 12)
        assert np.isfinite(r).all(), p
        assert np.array_equal(hs[1].spectrum(p, 12), r) and np.array_equal(hs[2].spectrum(p, 12), r)
        assert np.array_equal(r, s2.spectrum_readings(rows, w, p, 12))
        db, fc = hs[0].spectrum_bands(p, SR, 3, 12)
        want = s2.spectrum_band_readings(rows, w, p, SR, 3, 12)
        assert np.array_equal(db, want[0]) and np.array_equal(fc, want[1]) and len(db) > 20


def test_timing_entry():
    """s2r_debug_spectrum_ms: -1 without s2r_set_timing; under it the spectrum kernel's time of the last master fill, 0 when that
    fill ran none — as s2r_debug_loudness_ms reads with its meter off"""
    a = _handles(V)[0]
    ms, lms = a.L.s2r_debug_spectrum_ms, a.L.s2r_debug_loudness_ms
    for f in (ms, lms):
        f.restype, f.argtypes = C.c_float, [C.c_void_p]
    _events((a,), V, 0)
    a.set_master_spectrum(2048, 512)
    a.sample_master(300, SR, 2)
    assert ms(a.h) == -1.0 and lms(a.h) == -1.0
    a.set_timing(True)
    a.sample_master(300, SR, 2)
    assert 0.0 < ms(a.h) < 100.0 and lms(a.h) == 0.0
    a.clear_master_spectrum()
    a.sample_master(300, SR, 2)
    assert ms(a.h) == 0.0 and lms(a.h) == 0.0
