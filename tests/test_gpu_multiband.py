"""The master multiband compressor on the device.  Twin handles are fed the same events, one with the stage and one
without; the twin's sample_master output is x — the master behind the fader — and the expectation is always s2r_multiband_reference
over x with the state carried from call to call on the host (tests/test_multiband_host.py holds that reference to an independent numpy
loop).  Every comparison is on bits with no NaN allowance (helpers.assert_bits_equal_finite).

Handles, events and the one-pole bank are tests/test_gpu_reverb.py's at 32 voices.  The crossover splits at 200 / 1500 / 6000 Hz; the
bands' thresholds come from a first pass of the host model with unit curves over the twin's first call: half of each band's peak, so
that every band is driven through its knee in both directions.  Before anything is compared the host model alone must show that every
band takes both the attack and the release branch and that every minimum gain is below 1."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_gpu_buses import ubits
from test_gpu_dyn import _level, _targets
from test_gpu_reverb import SR, _bank, _events, _handles

pytestmark = pytest.mark.gpu
F = np.float32
V = 32
T = 128                                                          # S2R_MULTIBAND_TILE (csrc/s2r_device.h); test_the_tile_is_the_kernels holds it to the library
MAXF = 2048
SPLITS = [200.0, 1500.0, 6000.0]
# the first call gives the thresholds; then the calls around the crossover tree's depth, around the kernel's tile, and the longest
CALLS = [1024, 1, 2, 3, 5, 6, 7, 8, 9, T - 1, T, T + 1, 2 * T + 1, MAXF]
# retention coefficients of 1 ms and 50 ms, as s2r_dynamics_coef makes them (computed here: nothing loads the library while the
# suite is collected)
ATT, REL = float(F(np.exp(-1.0 / (1.0 * 0.001 * SR)))), float(F(np.exp(-1.0 / (50.0 * 0.001 * SR))))
RATIOS = [(4.0, 6.0), (float("inf"), 0.0), (2.0, 12.0), (8.0, 3.0)]


def _coeffs(B):
    return s2.multiband_design(float(SR), SPLITS[:B - 1]) if B > 1 else None


def _unit(B):
    return np.ones((B, s2.DYN_CURVE_POINTS), dtype=F)


def _curves(B, x):
    """a curve per band whose threshold is half the band's peak over x, by the host model with unit curves"""
    bands = s2.multiband_reference(_coeffs(B), _unit(B), [0.0] * B, [0.0] * B, x, want_bands=True)[3]
    out = []
    for j in range(B):
        peak = float(np.abs(bands[j]).max())
        assert peak > 2.0 ** -20, "band %d of %d is all but silent in the first call" % (j, B)
        ratio, knee = RATIOS[j]
        out.append(s2.dynamics_curve(20.0 * np.log10(peak / 2.0), ratio, knee, 0.0))
    return np.stack(out)


class Mb:
    """the stage of a handle on the host: its parameters, the carried state, the last call's minima, and what the parity conditions
    count per band: frames of either branch of the ballistics"""

    def __init__(self, B, curves, att=None, rel=None, coeffs="design"):
        self.B, self.coeffs, self.curves = B, _coeffs(B) if isinstance(coeffs, str) else coeffs, np.array(curves, dtype=F)
        self.att, self.rel = [ATT] * B if att is None else att, [REL] * B if rel is None else rel
        self.reset()
        self.n_att, self.n_rel, self.least = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64), np.full(B, np.inf)

    def reset(self):
        self.state = np.zeros(s2.multiband_state_floats(self.B), dtype=F)
        self.state[-self.B:] = self.curves[:, 0]
        self.mn = None

    def set(self, syn, params=False):
        (syn.set_master_multiband_params if params else syn.set_master_multiband)(self.curves, self.att, self.rel, coeffs=self.coeffs)
        got = syn.get_master_multiband()
        assert got["n_bands"] == self.B and np.array_equal(ubits(got["curves"]), ubits(self.curves))
        if self.B > 1:
            for name, want in zip(("lp", "hp", "ap"), self.coeffs):
                assert np.array_equal(ubits(got[name]), ubits(want)), name
        if not params:
            self.reset()

    def expect(self, x):
        y0 = self.state[-self.B:].copy()
        out, self.state, self.mn, bands = s2.multiband_reference(self.coeffs, self.curves, self.att, self.rel, x, self.state, want_bands=True)
        for j in range(self.B):                                  # the gains themselves: the dynamics' rule over a signal of ones, keyed by the band
            ys = s2.dynamics_reference(self.curves[j], self.att[j], self.rel[j], bands[j], np.ones_like(bands[j]), y0[j])[0][:, 0]
            assert ubits(ys[-1:])[0] == ubits(self.state[-self.B + j:][:1])[0] and ubits(ys.min(keepdims=True))[0] == ubits(self.mn[j:j + 1])[0]
            before = np.concatenate([[y0[j]], ys[:-1]])
            t = _targets(self.curves[j], _level(bands[j]))
            self.n_att[j] += int((t < before).sum()); self.n_rel[j] += int((t >= before).sum())
            self.least[j] = min(self.least[j], float(ys.min()))
        return out

    def check(self, syn, what, state=False):
        assert_bits_equal_finite(syn.multiband_meters(), self.mn, what + ": meters")
        if state:                                                # (a read fetches the state, and the next fill sends it back: not after every call)
            assert_bits_equal_finite(syn.multiband_state(), self.state, what + ": state")

    def both_branches(self, what):
        print("%s: attack frames %s, release frames %s, least gains %s" % (what, self.n_att, self.n_rel, self.least))
        assert (self.n_att > 0).all() and (self.n_rel > 0).all(), "%s: a band takes one branch only: %s attack, %s release" % (what, self.n_att, self.n_rel)
        assert (self.least < 1.0).all(), "%s: a band's gain never falls below 1: %s" % (what, self.least)


def _pair(max_frames=MAXF, n=2, fader=0.7):
    hs = _handles(V, max_frames=max_frames, n=n)
    for syn in hs:
        for bus in range(s2.MAX_BUSES):
            syn.set_bus_return(bus, 1.0 - bus / 16.0)
        syn.set_master_fader(fader)
        syn.snap_master()
    return hs


def _mfill(a, b, m, n, nb, what, stems=True, state=False):
    """one call on both handles: the twin's sample_master gives x, its stems and its meters; the handle with the stage returns the
    host rule over x, the twin's stems and the twin's master-section meters"""
    x, st_b = b.sample_master(n, SR, nb)
    assert np.isfinite(x).all() and ubits(x).any(), what
    want = m.expect(x)
    got, st = a.sample_master(n, SR, nb, stems=stems)
    assert_bits_equal_finite(got, want, what + ": master")
    if stems:
        assert_bits_equal_finite(st, st_b, what + ": stems")
    else:
        assert st is None
    for g, w, name in zip(a.meters(), b.meters(), ("peaks", "energies")):
        assert_bits_equal_finite(g, w, what + ": master section " + name)
    m.check(a, what, state)
    return x, got


def _first_call(nb, fader=0.7, max_frames=MAXF):
    """the twin's first call, from a handle of its own"""
    p = _pair(max_frames, fader=fader)[1]
    _events((p,), V, 0)
    return p.sample_master(min(CALLS[0], max_frames), SR, nb)[0]


def _model_alone(B, calls, nb, max_frames, what, twin=None, curves_of=None):
    """the host model over a twin alone, in front of any comparison with the device: the twin's masters of `calls`, the curves from the
    first of them, and the assertion that every band takes both branches of the ballistics and that every minimum gain is below 1"""
    p = twin() if twin else _pair(max_frames)[1]
    xs = []
    for fill, n in enumerate(calls):
        _events((p,), V, fill)
        xs.append(p.sample_master(n, SR, nb)[0])
    curves = curves_of(xs[0]) if curves_of else _curves(B, xs[0])
    probe = Mb(B, curves)
    for x in xs:
        probe.expect(x)
    probe.both_branches(what + ", the model alone")
    return curves, xs


def test_the_tile_is_the_kernels():
    tile = s2.load_library().s2r_debug_multiband_tile
    tile.restype, tile.argtypes = C.c_uint32, []
    assert tile() == T


@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_multiband_is_the_rule_over_the_twins_master(B):
    """1 .. 4 bands on 2 buses: consecutive calls on one handle with the state carried, of 1 .. 9 frames around the tree's depth, around
    the kernel's tile and of max_frames, events between them, every other call without stems"""
    nb = 2
    # the model first, over a twin alone: every band must work in both directions before the device is asked anything
    p = _pair()[1]
    xs = []
    for fill, n in enumerate(CALLS):
        _events((p,), V, fill)
        xs.append(p.sample_master(n, SR, nb)[0])
    curves = _curves(B, xs[0])
    probe = Mb(B, curves)
    for x in xs:
        probe.expect(x)
    probe.both_branches("%d bands, the model alone" % B)
    # ... then both handles from the start
    a, b = _pair()
    m = Mb(B, curves)
    m.set(a)
    changed = False
    for fill, n in enumerate(CALLS):
        _events((a, b), V, fill)
        x, got = _mfill(a, b, m, n, nb, "%d bands, fill %d of %d frames" % (B, fill, n), stems=fill % 2 == 0, state=fill in (4, len(CALLS) - 1))
        assert_bits_equal_finite(x, xs[fill], "the second twin")
        changed = changed or not np.array_equal(ubits(got), ubits(x))
    assert changed, "the stage changes no bit"
    m.both_branches("%d bands" % B)


@pytest.mark.parametrize("stems", [True, False])
@pytest.mark.parametrize("loudness", [False, True])
@pytest.mark.parametrize("limiter", ["off", "sample", "true"])
def test_every_route_behind_the_stage(limiter, loudness, stems):
    """3 bands in front of every reader of the master: the limiter off, with the sample-peak and with the true-peak detector, the
    loudness meter off and on, with and without stems.  The expectation is the host rule over the twin's master and the limiter's host
    rule over that; the stems, and the buses' loudness rows, are the twin's in every bit (the twin runs the same meter, on its own
    master: the master's two columns differ by design)."""
    B, nb = 3, 2
    calls = [300, 7, T + 1, 512]
    curves, xs = _model_alone(B, calls, nb, 512, "limiter %s, loudness %s, stems %s" % (limiter, loudness, stems))
    a, b = _pair(512)
    m = Mb(B, curves)
    m.set(a)
    L, H = 48, 20
    ceiling = float(np.abs(xs[0]).max()) * 0.25
    if limiter != "off":
        a.set_master_limiter(ceiling, L, H, true_peak=limiter == "true")
    if loudness:
        for syn in (a, b):
            syn.set_master_loudness(SR, hop=64)
    xh = gh = None
    ref = s2.limiter_tp_reference if limiter == "true" else s2.limiter_reference
    for fill, n in enumerate(calls):
        _events((a, b), V, fill)
        what = "limiter %s, loudness %s, stems %s, fill %d" % (limiter, loudness, stems, fill)
        x, st_b = b.sample_master(n, SR, nb)
        assert_bits_equal_finite(x, xs[fill], what + ": the second twin")
        want = m.expect(x)
        if limiter != "off":
            want, gain, xh, gh = ref(want, ceiling, L, H, xh, gh)
        got, st = a.sample_master(n, SR, nb, stems=stems)
        assert_bits_equal_finite(got, want, what + ": master")
        if stems:
            assert_bits_equal_finite(st, st_b, what + ": stems")
        else:
            assert st is None
        m.check(a, what)
        if loudness:
            ra, rb = a.loudness_hops(), b.loudness_hops()
            assert ra.shape == rb.shape and ra.shape[0] > 0
            assert_bits_equal_finite(ra[:, :2 * nb], rb[:, :2 * nb], what + ": the buses' loudness rows")
    m.both_branches("limiter %s" % limiter)


def test_params_keep_the_state_and_a_set_resets_it():
    """s2r_set_master_multiband_params changes curves and coefficients in the middle of a stream and the filters and gains go on from
    where they were; s2r_set_master_multiband and s2r_reset_master_multiband start them afresh; the meters are the reference's minima"""
    B, nb = 4, 2
    x0 = _first_call(nb, max_frames=512)
    curves = _curves(B, x0)
    a, b = _pair(512)
    m = Mb(B, curves)
    m.set(a)
    for fill in range(2):
        _events((a, b), V, fill)
        _mfill(a, b, m, 200, nb, "before the new parameters, fill %d" % fill)
    carried = m.state.copy()
    assert ubits(carried[:-B]).any() and not np.array_equal(ubits(carried[-B:]), ubits(curves[:, 0]))
    m.curves, m.att, m.rel = np.ascontiguousarray(curves[::-1]), [0.0, ATT, REL, 0.5], [REL, 0.0, ATT, 0.25]
    m.coeffs = s2.multiband_design(float(SR), [300.0, 1000.0, 5000.0])
    m.set(a, params=True)
    assert_bits_equal_finite(a.multiband_state(), carried, "the state behind new parameters")
    _events((a, b), V, 2)
    _mfill(a, b, m, 333, nb, "behind the new parameters", state=True)
    m.set(a)                                                     # a set: from the initial state
    assert_bits_equal_finite(a.multiband_state(), m.state, "the state behind a set")
    assert not ubits(m.state[:-B]).any()
    _events((a, b), V, 3)
    _mfill(a, b, m, 129, nb, "behind a set", state=True)
    a.reset_master_multiband()
    m.reset()
    with pytest.raises(s2.S2rError):                             # no call has run the stage since
        a.multiband_meters()
    _events((a, b), V, 4)
    _mfill(a, b, m, 64, nb, "behind a reset", state=True)
    with pytest.raises(s2.S2rError):                             # another band count is a set's business
        a.set_master_multiband_params(curves[:2], [ATT] * 2, [REL] * 2, coeffs=_coeffs(2))
    _events((a, b), V, 5)
    _mfill(a, b, m, 64, nb, "behind a refused change of the band count", state=True)


def test_checkpoint_in_the_middle_of_a_stream():
    """the state read from one handle and set into a fresh one, with the voices' state beside it, continues on bits"""
    B, nb = 3, 2
    curves = _curves(B, _first_call(nb, max_frames=512))
    a, b = _pair(512)
    m = Mb(B, curves)
    m.set(a)
    for fill, n in enumerate([300, 5]):
        _events((a, b), V, fill)
        _mfill(a, b, m, n, nb, "in front of the checkpoint, fill %d" % fill)
    st = a.multiband_state()
    assert_bits_equal_finite(st, m.state, "the state checked out")
    c = s2.Synth(V, max_frames=512, block_voices=64)
    c.set_patch_bank(_bank())
    c.import_state(a.export_state())
    c.set_voice_pans(a.voice_pans())
    c.set_voice_mix(*a.voice_mix())
    c.set_voice_sends(*a.voice_sends())
    for bus in range(s2.MAX_BUSES):
        c.set_bus_return(bus, 1.0 - bus / 16.0)
    c.set_master_fader(0.7)
    c.snap_master()
    m.set(c)
    m.state = st.copy()
    c.set_multiband_state(st)
    bad = st.copy(); bad[-1] = -1.0
    with pytest.raises(s2.S2rError):
        c.set_multiband_state(bad)
    with pytest.raises(s2.S2rError):
        c.set_multiband_state(st[:-1])
    for fill, n in enumerate([T + 3, 64], start=2):
        for syn in (a, b, c):
            syn.note_off(40 + fill)
        x, st_b = b.sample_master(n, SR, nb)
        want = m.expect(x)
        for syn, name in ((a, "the handle that went on"), (c, "the handle restored")):
            assert_bits_equal_finite(syn.sample_master(n, SR, nb)[0], want, "%s, fill %d" % (name, fill))
            m.check(syn, name, state=True)


def test_off_never_set_and_the_other_fills():
    """after a clear the master is the twin's on bits; the bus fill ignores the stage; a handle on which it was never set holds nothing
    of it; device-list and NULL handles are refused"""
    B, nb = 2, 2
    curves = _curves(B, _first_call(nb, max_frames=256))
    a, b = _pair(256)
    L = a.L
    L.s2r_debug_multiband_allocated.restype, L.s2r_debug_multiband_allocated.argtypes = C.c_int, [C.c_void_p]
    L.s2r_debug_multiband_ms.restype, L.s2r_debug_multiband_ms.argtypes = C.c_float, [C.c_void_p]
    m = Mb(B, curves)
    m.set(a)
    assert not L.s2r_debug_multiband_allocated(a.h), "a set allocates nothing: the first master fill does"
    _events((a, b), V, 0)
    assert_bits_equal_finite(a.sample_buses(100, SR, nb), b.sample_buses(100, SR, nb), "a bus fill with the stage set")
    assert not L.s2r_debug_multiband_allocated(a.h), "a bus fill allocates nothing of the stage's"
    assert_bits_equal_finite(m.state, a.multiband_state(), "a bus fill leaves the state alone")
    for syn in (a, b):
        syn.set_timing(True)
    _events((a, b), V, 1)
    _mfill(a, b, m, 200, nb, "the stage on")
    assert L.s2r_debug_multiband_allocated(a.h) and not L.s2r_debug_multiband_allocated(b.h)
    assert L.s2r_debug_multiband_ms(a.h) > 0.0 and L.s2r_debug_multiband_ms(b.h) == 0.0
    a.clear_master_multiband()
    assert a.get_master_multiband() is None
    for fill in (2, 3):
        _events((a, b), V, fill)
        (x, st_b), (got, st) = b.sample_master(131, SR, nb), a.sample_master(131, SR, nb)
        assert_bits_equal_finite(got, x, "the master behind a clear, fill %d" % fill)
        assert_bits_equal_finite(st, st_b, "the stems behind a clear, fill %d" % fill)
    assert L.s2r_debug_multiband_ms(a.h) == 0.0
    with pytest.raises(s2.S2rError):
        a.multiband_state()
    # refusals: the values first, then the handle
    lp, hp, ap = _coeffs(3)
    c3, att, rel = _unit(3), np.zeros(3, dtype=F), np.zeros(3, dtype=F)
    p = lambda v: v.ctypes.data_as(s2s._f32p)
    call = lambda h, n, lp_=lp, hp_=hp, ap_=ap, cv=c3, at=att, rl=rel: L.s2r_set_master_multiband(h, n, p(lp_), p(hp_), p(ap_) if ap_ is not None else None, p(cv), p(at), p(rl))
    nan, wild = lp.copy(), hp.copy()
    nan[1, 2] = np.nan
    wild[0, 4] = 1.0                                             # a2 = 1: on the stability triangle's edge
    big = c3.copy(); big[2, 100] = 300.0
    one = np.ones(3, dtype=F)
    for name, rc, want in (("no band", call(a.h, 0), s2s.S2R_ERR_PATCH_RANGE), ("five bands", call(a.h, 5), s2s.S2R_ERR_PATCH_RANGE),
                           ("a NaN coefficient", call(a.h, 3, lp_=nan), s2s.S2R_ERR_PATCH_RANGE), ("an unstable section", call(a.h, 3, hp_=wild), s2s.S2R_ERR_PATCH_RANGE),
                           ("a curve entry of 300", call(a.h, 3, cv=big), s2s.S2R_ERR_PATCH_RANGE), ("a retention coefficient of 1", call(a.h, 3, at=one), s2s.S2R_ERR_PATCH_RANGE),
                           ("null allpass rows at three bands", call(a.h, 3, ap_=None), s2s.S2R_ERR_INVALID), ("a NULL handle", call(None, 3), s2s.S2R_ERR_INVALID),
                           ("a NULL handle's clear", L.s2r_clear_master_multiband(None), s2s.S2R_ERR_INVALID)):
        assert rc == want, "%s: %d, not %d" % (name, rc, want)
    assert a.get_master_multiband() is None, "a refused set sets nothing"
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    u = C.c_uint32()
    assert call(multi.h, 3) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_clear_master_multiband(multi.h) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_master_multiband(multi.h, C.byref(u), None, None, None, None, None, None) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_reset_master_multiband(multi.h) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_multiband_state(multi.h, p(att), 3) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_multiband_state(multi.h, p(att), 3) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_multiband_meters(multi.h, p(att), 3) == s2s.S2R_ERR_INVALID
    # ... and the handle that was refused works on as the twin
    _events((a, b), V, 4)
    assert_bits_equal_finite(a.sample_master(64, SR, nb)[0], b.sample_master(64, SR, nb)[0], "behind the refusals")


def test_a_refused_fill_leaves_the_state():
    """a master fill refused for its frame count changes neither state nor meters, and the next one goes on as if it had not happened"""
    B, nb = 4, 2
    curves = _curves(B, _first_call(nb, max_frames=256))
    a, b = _pair(256)
    m = Mb(B, curves)
    m.set(a)
    _events((a, b), V, 0)
    _mfill(a, b, m, 100, nb, "in front of the refusal", state=True)
    with pytest.raises(s2.S2rError):
        a.sample_master(257, SR, nb)
    m.check(a, "behind the refusal", state=True)
    _events((a, b), V, 1)
    _mfill(a, b, m, 256, nb, "the fill behind the refusal", state=True)


def test_denormal_filter_states():
    """a master fader of 2^-120 puts the master, and with it every section's state, into the denormal range: parity still holds, and
    the states read back are denormal, not zero"""
    B, nb = 4, 2
    fader = 2.0 ** -120
    x0 = _first_call(nb, fader=fader, max_frames=512)
    assert 0.0 < np.abs(x0).max() < 2.0 ** -100
    a, b = _pair(512, fader=fader)
    m = Mb(B, _unit(B) * F(0.5), att=[0.0] * B, rel=[0.5] * B)
    m.set(a)
    for fill, n in enumerate([300, 9, T + 1]):
        _events((a, b), V, fill)
        _mfill(a, b, m, n, nb, "fader 2^-120, fill %d" % fill, state=True)
    filt = np.abs(m.state[:-B])
    assert ((filt > 0.0) & (filt < np.finfo(F).tiny)).any(), "no section's state is denormal"


def test_one_band_is_the_bus_dynamics():
    """on a one-bus handle with unit return and fader, one band gives the values of the same curve set as the bus's dynamics (==: the
    master kernel's sum may differ from the bus in the sign of a zero)"""
    calls = [512, 7, T + 1]
    curve = _model_alone(1, calls, 1, 512, "one band", twin=lambda: _handles(V, max_frames=512)[0],
                         curves_of=lambda x0: s2.dynamics_curve(20.0 * np.log10(float(np.abs(x0).max()) / 2.0), 4.0, 6.0, 0.0)[None])[0][0]
    a, b, c = _handles(V, max_frames=512, n=3)
    a.set_master_multiband(curve[None], [ATT], [REL])
    c.set_bus_dynamics(0, 0, curve, ATT, REL)
    m = Mb(1, curve[None], coeffs=None)
    for fill, n in enumerate(calls):
        _events((a, b, c), V, fill)
        x = b.sample_master(n, SR, 1)[0]
        got, want = a.sample_master(n, SR, 1)[0], c.sample_master(n, SR, 1)[0]
        assert_bits_equal_finite(got, m.expect(x), "one band, fill %d" % fill)
        assert np.isfinite(want).all() and (got == want).all(), "one band against the bus dynamics, fill %d" % fill
        assert ubits(a.multiband_meters())[0] == ubits(np.array([c.bus_dynamics_meter(0)], dtype=F))[0]
    assert m.least[0] < 1.0 and m.n_att[0] > 0 and m.n_rel[0] > 0
