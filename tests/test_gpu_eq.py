"""The per-bus parametric EQ on the device.  Twin handles are fed the same events, one with EQs and one without; the
twin's bus output is x, what the bus combine writes, and the expectation is the rule on the host (s2.eq_reference, which
tests/test_eq_host.py holds to a numpy float32 model on bits) over x with the state carried from call to call (EqModel); behind it
come the models of the stages that follow: the chorus's (test_gpu_chorus.ChorusModel), the delay's (test_gpu_delay.DelayModel), the
reverb's (test_gpu_reverb.Model), the master section's (test_gpu_master.Master), the limiter's (test_gpu_limiter.Lim).

The kernel is systolic — band k works on frame t - k at step t — and stages its input by tiles of T frames (s2r_debug_eq_tile), so the
call lengths are 1 to 5 frames (shorter than, as long as and just longer than the pipeline is deep), T - 1, T, T + 1 and 2T + 1, and
max_frames.  Handles, events and the one-pole bank are tests/test_gpu_reverb.py's.  Every comparison is on bits with no NaN allowance
(helpers.assert_bits_equal_finite)."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_eq_host import _bands, bits, check_ranges
from test_gpu_buses import ubits
from test_gpu_chorus import SHAPES, ChorusModel
from test_gpu_delay import DelayModel
from test_gpu_limiter import Lim
from test_gpu_master import Master
from test_gpu_reverb import SR, V, Model, _bank, _events, _handles, _ir, _timed
from test_master_host import np_meters

pytestmark = pytest.mark.gpu
F = np.float32


T = 64                                                           # S2R_EQ_TILE (csrc/s2r_device.h); test_the_tile_is_the_kernels holds it to the library


def _tile():
    L = s2.load_library()
    L.s2r_debug_eq_tile.restype, L.s2r_debug_eq_tile.argtypes = C.c_uint32, []
    return int(L.s2r_debug_eq_tile())


FRAMES = [1024, 1, 2, 3, 4, 5, T - 1, T, T + 1, 2 * T + 1, 3, 1, 1024]
# (n_buses, bands per bus; 0: no EQ on that bus): every band count, one wave full of EQs, and buses without one among them
MATRIX = [(1, (4,)), (1, (1,)), (2, (1, 3)), (3, (2, 0, 4)), (8, (4, 1, 3, 2, 4, 1, 3, 2)), (8, (4, 1, 3, 2, 0, 2, 0, 1))]


def _coeffs(n_bands, seed):
    """n_bands bands of tests/test_eq_host._bands — peaks, shelves, a high-pass, a low-pass, gains up to 18 dB — and, for every third
    seed, a last band given as raw numbers, with a zero among them: nothing is skipped for a zero coefficient"""
    c = _bands(n_bands, seed).copy()
    if seed % 3 == 0:
        c[-1] = (0.75, 0.0, -0.5, -1.25, 0.5)
    return c


class EqModel:
    """the EQs of a handle on the host: per bus the coefficients [n_bands, 5] and the carried state [n_bands, 4]"""

    def __init__(self):
        self.e = {}

    def set(self, bus, coeffs):
        c = np.array(coeffs, dtype=F).reshape(-1, 5)
        self.e[bus] = dict(c=c, st=np.zeros((c.shape[0], 4), dtype=F))

    def expect(self, x):
        """what the EQ makes of a call whose combined buses are x [n_buses, N, 2]; the states of its buses move on"""
        want = x.copy()
        for b, f in self.e.items():
            if b >= x.shape[0]:
                continue                                         # idle in this call
            want[b], f["st"] = s2.eq_reference(f["c"], x[b], f["st"])
        return want


def _set(a, model, bus, coeffs):
    a.set_bus_eq(bus, coeffs)
    assert np.array_equal(bits(a.get_bus_eq(bus)), bits(np.asarray(coeffs, dtype=F).reshape(-1, 5)))
    model.set(bus, coeffs)


def _fill(a, b, model, n, nb, what):
    """one call on both handles: the buses with an EQ against the model over the twin's, the others against the twin's"""
    x = b.sample_buses(n, SR, nb)
    assert np.isfinite(x).all()
    want = model.expect(x)
    got = a.sample_buses(n, SR, nb)
    assert_bits_equal_finite(got, want, what)
    for bus in range(nb):
        if bus in model.e:
            assert ubits(x[bus]).any(), "%s: bus %d is silent" % (what, bus)
            assert not np.array_equal(ubits(got[bus]), ubits(x[bus])), "%s: the EQ on bus %d changes no bit" % (what, bus)
        else:
            assert_bits_equal_finite(got[bus], x[bus], "%s: bus %d, which carries no EQ" % (what, bus))
    return x, got


def _states(a, model, what):
    for bus, f in model.e.items():
        assert_bits_equal_finite(a.bus_eq_state(bus), f["st"], "%s: state of bus %d" % (what, bus))


def test_the_tile_is_the_kernels():
    assert _tile() == T


@pytest.mark.parametrize("n_buses,bands", MATRIX)
def test_eq_is_the_rule_over_the_dry_bus(n_buses, bands):
    """the parity matrix: calls of max_frames, then 1 to 5 frames, T - 1, T, T + 1, 2T + 1, 3, 1 and max_frames again on one pair of
    handles, the state carried through all of them and read back after each; the buses without an EQ must equal the twin's on bits"""
    a, b = _handles()
    model = EqModel()
    for bus, nb in enumerate(bands):
        if nb:
            _set(a, model, bus, _coeffs(nb, bus + n_buses))
    for fill, n in enumerate(FRAMES):
        _events((a, b), V, fill)
        what = "%d buses, bands %s, fill %d of %d frames" % (n_buses, bands, fill, n)
        _fill(a, b, model, n, n_buses, what)
        _states(a, model, what)
    assert all(ubits(f["st"]).any() for f in model.e.values())


def test_a_run_of_short_calls_is_one_long_call():
    """no model in the loop: four handles, two with the same EQs; one of each kind renders the same frames in a run of calls, the other
    in one call.  The render kernels work in chunks of 16 frames counted from the start of a call, so the mixdown itself is one
    stream only where calls are cut at multiples of 16 — which is asserted on the handles without an EQ — and the cuts here are such:
    16, 48, T, T + 16, 2T + 16 and more.  (Calls of 1 to 5 frames are in the test below, and in the matrix against the rule.)  On
    bits, the two handles with the EQs agree, outputs and states"""
    a, b, c, d = _handles() + _handles()
    for syn in (a, c):
        for bus, nb in enumerate((4, 3, 0, 1)):
            if nb:
                syn.set_bus_eq(bus, _coeffs(nb, bus))
    cuts = [16, 48, 16, T, T + 16, 2 * T + 16, 16, 32, 208]
    total = sum(cuts)
    assert total <= 1024 and all(n % 16 == 0 for n in cuts)
    _events((a, b, c, d), V, 0)
    short_eq = np.concatenate([a.sample_buses(n, SR, 4) for n in cuts], axis=1)
    short_dry = np.concatenate([b.sample_buses(n, SR, 4) for n in cuts], axis=1)
    long_eq, long_dry = c.sample_buses(total, SR, 4), d.sample_buses(total, SR, 4)
    assert_bits_equal_finite(short_dry, long_dry, "without an EQ: the mixdown in short calls and in one")
    assert_bits_equal_finite(short_eq, long_eq, "with the EQs: short calls and one long call")
    assert_bits_equal_finite(short_eq[2], long_dry[2], "the bus without an EQ")
    for bus in (0, 1, 3):
        assert not np.array_equal(ubits(long_eq[bus]), ubits(long_dry[bus]))
        assert_bits_equal_finite(a.bus_eq_state(bus), c.bus_eq_state(bus), "the state of bus %d after both" % bus)


@pytest.mark.parametrize("n_bands", [1, 2, 3, 4])
def test_a_cascade_of_delays_is_the_twin_late_across_short_calls(n_bands):
    """no model in the loop: a band (0, 0, 1, 0, 0) is a delay of two frames — y = s1, s1' = s2, s2' = x — so n_bands of them are the
    twin's bus 2 * n_bands frames late, across the boundaries of calls of 1 to 5 frames, T - 1, T, T + 1 and 2T + 1: what a call leaves
    in the lanes of the wave is what the next one starts from.  Values, not bits: 0 * x + s1 gives up the sign of a zero."""
    a, b = _handles()
    a.set_bus_eq(1, np.tile(np.array([0.0, 0.0, 1.0, 0.0, 0.0], dtype=F), (n_bands, 1)))
    late = 2 * n_bands
    stream = [np.zeros((late, 2), dtype=F)]
    at = 0
    for fill, n in enumerate([1, 2, 3, 4, 5, 1, 1, 2, T - 1, T, T + 1, 2 * T + 1, 3, 300]):
        _events((a, b), V, fill)
        x = b.sample_buses(n, SR, 3)
        got = a.sample_buses(n, SR, 3)
        stream.append(x[1])
        want = np.concatenate(stream, axis=0)[at:at + n]
        at += n
        assert np.isfinite(got).all()
        assert np.array_equal(got[1], want), "%d delays, fill %d of %d frames" % (n_bands, fill, n)
        assert_bits_equal_finite(got[[0, 2]], x[[0, 2]], "the buses beside it")
    heard = np.concatenate(stream, axis=0)
    assert (np.abs(heard[late:late + 16]).max(axis=1) > 0.0).sum() >= 12      # (frame 0 of the first call is silent; the short calls are not)


def test_an_eq_beside_a_bus_without_one_and_an_idle_one():
    """four bands on bus 0 and one on bus 2 of three buses: bus 1 between them is the twin's; an EQ on bus 5 is idle in these calls, and
    its crafted state, read back, is unchanged; a later call of eight buses goes on from it"""
    a, b = _handles()
    model = EqModel()
    _set(a, model, 0, _coeffs(4, 1))
    _set(a, model, 2, _coeffs(1, 2))
    _set(a, model, 5, _coeffs(3, 4))
    idle = (np.random.default_rng(5).standard_normal((3, 4)) * 0.125).astype(F)
    a.set_bus_eq_state(5, idle)
    model.e[5]["st"] = idle.copy()
    for fill, n in enumerate([300, 2, T + 1, 17]):
        _events((a, b), V, fill)
        x, got = _fill(a, b, model, n, 3, "EQs on buses 0 and 2 of three, fill %d" % fill)
        assert_bits_equal_finite(got[1], x[1], "the bus between them, fill %d" % fill)
    _states(a, model, "two EQs and an idle one")
    assert_bits_equal_finite(a.bus_eq_state(5), idle, "the idle EQ's state")
    _events((a, b), V, 4)
    _fill(a, b, model, 100, 8, "eight buses: the idle EQ wakes from its crafted state")
    _states(a, model, "after the call of eight buses")
    assert not np.array_equal(ubits(a.bus_eq_state(5)), ubits(idle))


@pytest.mark.parametrize("frames", [250, 64])
def test_events_inside_a_fill_and_sliced_rows(frames, monkeypatch):
    """note_ons at frames 16 and 48 split the call into segments and a rows buffer of 48 frames slices them further: the EQ sees the
    call as one stream"""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    a, b = _handles(max_frames=256)
    model = EqModel()
    _set(a, model, 0, _coeffs(3, 0))
    _set(a, model, 3, _coeffs(4, 1))
    for fill in range(3):
        _events((a, b), V, fill)
        _timed((a, b), fill)
        _fill(a, b, model, frames, 4, "events at 16 and 48, slices of 48, %d frames, fill %d" % (frames, fill))
    _states(a, model, "events and slices")
    a.L.s2r_debug_pan_slice.restype = C.c_uint32
    a.L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    assert a.L.s2r_debug_pan_slice(a.h) == 48


def test_a_send_only_bus_with_an_eq_while_a_fader_ramps():
    """bus 6 of eight sounds through program 0's send alone and carries the EQ; program 0's fader moves across the second and third
    call — on both handles, so the twin's bus 6 is x under the same sends and ramps"""
    a, b = _handles()
    model = EqModel()
    _set(a, model, 6, _coeffs(4, 2))
    walk = [(1.0, 0.0), (0.25, 1.0), (0.7, -0.5), (0.7, -0.5)]
    for fill, n in enumerate([300, 1000, 17, 64]):
        _events((a, b), V, fill)
        for syn in (a, b):
            syn.set_program_fader(0, *walk[fill])
        _fill(a, b, model, n, 8, "send-only bus under a fader ramp, fill %d" % fill)
        f = a.get_program_fader(0)
        assert f == b.get_program_fader(0) and f[:2] == f[2:]    # committed on both
    _states(a, model, "under the ramps")


def test_every_route_with_the_eq_on():
    """Handle `a` walks all 24 rows of s2r_post_route's table with EQs on all three buses, 64 frames a call — a bus fill, a master fill
    and a master fill under the limiter, each with every subset of chorus, delay and reverb, master fills with and without stems —;
    its twin `b` makes a plain bus fill of the same frames every time, so its stems are x.  The EQ stands in front of each of chorus
    (buses 1 and 2), delay (bus 2) and reverb (bus 1), and of all three.  Every step's expectation is the chain of the models: EQ,
    chorus, delay, reverb, master section, limiter; the meters after a master fill are np_meters over the model's stems and master.
    Everything the device returns is collected first, then compared."""
    a, b = _handles()
    eq, ch, dl, rv, mm = EqModel(), ChorusModel(), DelayModel(), Model(), Master()
    for bus, nb in enumerate((2, 4, 1)):
        _set(a, eq, bus, _coeffs(nb, bus + 1))
    ir = _ir(40, 77, True)
    steps, lims = [], []
    state = {"lim": None, "c": None, "on": (False, False, False)}

    def stages(chorus, delay, reverb):
        was = state["on"]
        if chorus != was[0]:
            if chorus:
                for bus, args in ((2, (3,) + SHAPES[145] + (89478 * 20, 0x40000000, 0.5, 0.25)), (1, (2,) + SHAPES[3] + (1 << 22, 5, 0.75, 0.5))):
                    a.set_bus_chorus(bus, *args)
                    ch.set(bus, *args)
            else:
                for bus in (1, 2):
                    a.clear_bus_chorus(bus)
                    del ch.c[bus]
        if delay != was[1]:
            if delay:
                a.set_bus_delay(2, 200, 0.5, -0.5, 0.5, 1.0)
                dl.set(2, 200, 0.5, -0.5, 0.5, 1.0)
            else:
                a.clear_bus_delay(2)
                del dl.d[2]
        if reverb != was[2]:
            if reverb:
                a.set_bus_reverb(1, ir, 0.25, 1.0)
                rv.set(1, ir, 0.25, 1.0)
            else:
                a.clear_bus_reverb(1)
                del rv.fx[1]
        state["on"] = (chorus, delay, reverb)

    def chain(n, nb=3):
        x = b.sample_buses(n, SR, nb)
        y = eq.expect(x)
        assert all(not np.array_equal(ubits(y[q]), ubits(x[q])) for q in range(nb))
        return rv.expect(dl.expect(ch.expect(y)))

    def bus_fill(what, n):
        y = chain(n)
        steps.append((what, {"buses": (a.sample_buses(n, SR, 3), y)}))

    def master_fill(what, n, stems):
        y = chain(n)
        m = mm.expect(y)
        if state["c"] is None:
            state["c"] = float(np.abs(m).max()) / 2.0            # the ceiling of the limiter below: half the first master's peak
        want = state["lim"].expect(m)[0] if state["lim"] else m
        got, st = a.sample_master(n, SR, 3, stems=stems)
        peak, energy = a.meters()
        wp, we = np_meters(y, m)
        cmp = {"master": (got, want), "peaks": (peak, wp), "energies": (energy, we)}
        if stems:
            cmp["stems"] = (st, y)
        steps.append((what, cmp))

    combos = [(False, False, False), (True, False, False), (True, True, False), (False, True, False), (False, True, True), (True, True, True),
              (True, False, True), (False, False, True)]
    k = 0
    for kind in ("bus fill", "master fill", "master fill under the limiter"):
        if kind == "master fill under the limiter":
            state["lim"] = Lim(48, 0, state["c"])
            state["lim"].set((a,), state["c"])
            lims.append(state["lim"])
        for j, on in enumerate(combos if kind != "master fill" else combos[::-1]):
            _events((a, b), V, k)
            stages(*on)
            what = "%d: %s, EQ on, chorus %s, delay %s, reverb %s" % ((k + 1, kind) + tuple("on" if o else "off" for o in on))
            if kind == "bus fill":
                bus_fill(what, 64)
            else:
                master_fill(what, 64, stems=j % 2 == 0)
            k += 1
    assert k == 24 and len(lims) == 1 and lims[0].limited() > 0.0       # on the model, before anything is compared: the walk limits
    for what, cmp in steps:
        for name, (got, want) in cmp.items():
            assert_bits_equal_finite(got, want, "%s: %s" % (what, name))
    mm.check_committed(a)
    _states(a, eq, "after the walk")
    for bus, f in ch.c.items():
        assert_bits_equal_finite(a.bus_chorus_state(bus)[0], f["hist"], "the chorus's history after the walk")
    for bus, f in dl.d.items():
        assert_bits_equal_finite(a.bus_delay_history(bus), f["hist"], "the delay's history after the walk")


def test_moving_a_band_keeps_the_state_and_setting_zeroes_it():
    a, b = _handles()
    model = EqModel()
    _set(a, model, 1, _coeffs(3, 1))
    _events((a, b), V, 0)
    _fill(a, b, model, 300, 2, "before the band moves")
    st = a.bus_eq_state(1)
    assert ubits(st).any()
    moved = model.e[1]["c"].copy()
    moved[1] = s2.eq_design(s2.EQ_PEAK, 2500.0, -9.0, 2.0, SR)
    a.set_bus_eq_coeffs(1, moved)
    model.e[1]["c"] = moved
    assert_bits_equal_finite(a.bus_eq_state(1), st, "the state under new coefficients")
    assert np.array_equal(bits(a.get_bus_eq(1)), bits(moved))
    _events((a, b), V, 1)
    _fill(a, b, model, 300, 2, "after s2r_set_bus_eq_coeffs")
    _states(a, model, "after the band moved")
    _set(a, model, 1, moved)                                     # setting the EQ again zeroes its state
    assert not ubits(a.bus_eq_state(1)).any()
    _events((a, b), V, 2)
    _fill(a, b, model, 64, 2, "after s2r_set_bus_eq")
    _states(a, model, "from a zero state")


def test_checkpoint_carries_the_state():
    """state, pans, mix, sends and the EQ's coefficients and state into a fresh handle: the next fills are equal"""
    a, b = _handles(max_frames=512)
    model = EqModel()
    _set(a, model, 1, _coeffs(4, 3))
    _events((a, b), V, 0)
    _fill(a, b, model, 200, 2, "before the checkpoint")
    st = a.bus_eq_state(1)
    assert st.shape == (4, 4) and ubits(st).any()
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    c = s2.Synth(V, max_frames=512, block_voices=64)
    c.set_patch_bank(_bank())
    c.import_state(state)
    c.set_voice_pans(pans)
    c.set_voice_mix(gains, buses)
    c.set_voice_sends(sends, sbuses)
    c.set_bus_eq(1, a.get_bus_eq(1))
    c.set_bus_eq_state(1, st)
    for k, n in enumerate([100, 400]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        _, got = _fill(a, b, model, n, 2, "the checkpointed handle, fill %d" % k)
        assert_bits_equal_finite(c.sample_buses(n, SR, 2), got, "the resumed handle, fill %d" % k)
    assert_bits_equal_finite(c.bus_eq_state(1), a.bus_eq_state(1), "both states after them")
    # the EQ is the bus's: a new bank, a program change and an imported state leave it and its state alone
    keep = a.bus_eq_state(1)
    a.set_patch_bank(_bank())
    a.program_change(3)
    a.import_state(state)
    assert np.array_equal(bits(a.get_bus_eq(1)), bits(model.e[1]["c"]))
    assert_bits_equal_finite(a.bus_eq_state(1), keep, "the EQ's state under a bank, a program change and an import")


def test_refusals_removal_and_the_other_fills():
    """a fill refused before any launch — a capacity too small, too many buses, too many frames — leaves the state untouched, in a bus
    fill and in a master fill; a wrong state size is refused; the panned, mono and stereo fills ignore EQs; after a removal the bus is
    the twin's on bits again; a device-list handle refuses all five entries and renders on"""
    a, b = _handles(max_frames=256)
    model = EqModel()
    _set(a, model, 0, _coeffs(3, 5))
    _events((a, b), V, 0)
    _fill(a, b, model, 100, 2, "before the refusals")
    before = a.bus_eq_state(0)
    assert ubits(before).any()
    L, h = a.L, a.h
    out, lr = np.empty(2 * 2 * 300, dtype=F), np.empty(2 * 300, dtype=F)
    p, q = out.ctypes.data_as(s2s._f32p), lr.ctypes.data_as(s2s._f32p)
    assert L.s2r_fill_buses(h, p, 2 * 2 * 100 - 1, 2, 100, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_buses(h, p, out.size, 9, 16, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_buses(h, p, out.size, 0, 16, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_buses(h, p, out.size, 2, 257, SR) == s2s.S2R_ERR_TOO_MANY_FRAMES
    assert L.s2r_fill_master(h, q, p, 2 * 2 * 100 - 1, 2, 100, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_master(h, q, p, out.size, 9, 16, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_master(h, q, p, out.size, 2, 257, SR) == s2s.S2R_ERR_TOO_MANY_FRAMES
    assert_bits_equal_finite(a.bus_eq_state(0), before, "the state after the refused fills")
    buf = np.zeros(32, dtype=F)
    bp = buf.ctypes.data_as(s2s._f32p)
    for count in (0, 11, 13, 8):
        assert L.s2r_set_bus_eq_state(h, 0, bp, count) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_eq_state(h, 0, bp, 11) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_eq_state(h, 1, bp, buf.size) == s2s.S2R_ERR_INVALID         # no EQ there
    assert L.s2r_set_bus_eq_coeffs(h, 1, 3, bp) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_eq_coeffs(h, 0, 2, bp) == s2s.S2R_ERR_INVALID               # another number of bands
    with pytest.raises(s2.S2rError) as err:
        a.set_bus_eq_state(0, np.zeros((4, 4), dtype=F))
    assert err.value.status == s2s.S2R_ERR_INVALID
    assert_bits_equal_finite(a.bus_eq_state(0), before, "the state after the refused setters")
    # the other fills
    assert_bits_equal_finite(a.sample_panned(100, SR), b.sample_panned(100, SR), "panned fill beside an EQ")
    assert_bits_equal_finite(a.sample(np.empty(64, dtype=F), SR), b.sample(np.empty(64, dtype=F), SR), "mono fill beside an EQ")
    assert_bits_equal_finite(a.sample_stereo(33, SR), b.sample_stereo(33, SR), "stereo copy beside an EQ")
    assert_bits_equal_finite(a.bus_eq_state(0), before, "the state after the other fills")
    _events((a, b), V, 1)
    _fill(a, b, model, 64, 2, "after the refusals and the other fills")
    # removal
    a.clear_bus_eq(0)
    del model.e[0]
    assert a.get_bus_eq(0).shape == (0, 5)
    _events((a, b), V, 2)
    x = b.sample_buses(64, SR, 2)
    assert_bits_equal_finite(a.sample_buses(64, SR, 2), x, "no EQ left: the twin's")
    # a device list
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    one = s2.Synth(512, max_frames=64, mix_groups=2)
    for syn in (multi, one):
        for v in range(512):
            syn.note_on(36 + v % 61)
    n = C.c_uint32()
    unit = np.array([1.0, 0.0, 0.0, 0.0, 0.0], dtype=F)
    up = unit.ctypes.data_as(s2s._f32p)
    assert multi.L.s2r_set_bus_eq(multi.h, 0, 1, up) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_eq(multi.h, 0, 0, None) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_eq_coeffs(multi.h, 0, 1, up) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_eq(multi.h, 0, C.byref(n), None, 0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_eq_state(multi.h, 0, bp, buf.size) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_eq_state(multi.h, 0, bp, 4) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        multi.set_bus_eq(0, unit)
    assert err.value.status == s2s.S2R_ERR_INVALID
    x, y = multi.sample(np.empty(64, dtype=F), SR), one.sample(np.empty(64, dtype=F), SR)
    assert np.abs(y).max() > 0.0
    assert_bits_equal_finite(x, y, "the device-list handle after the refused EQ calls")


def test_a_unit_band_over_silence_gives_up_the_sign_of_a_zero():
    """no voice is started, so every bus is silent; a unit band (1, 0, 0, 0, 0) whose state is set to -0.0 gives fl(fl(1 * x) + -0.0) at
    frame 0 and the sums of signed zeros behind it: the device follows the reference on bits, +0.0 and -0.0 told apart, and the
    buses without an EQ are the twin's"""
    a, b = _handles()
    model = EqModel()
    unit = np.array([[1.0, 0.0, 0.0, 0.0, 0.0], [-1.0, 0.0, 0.0, 0.0, 0.0]], dtype=F)
    _set(a, model, 1, unit)
    st = np.array([[-0.0, 0.0, -0.0, -0.0], [-0.0, -0.0, 0.0, -0.0]], dtype=F)
    a.set_bus_eq_state(1, st)
    model.e[1]["st"] = st.copy()
    for fill, n in enumerate([1, 5, 16]):
        x = b.sample_buses(n, SR, 3)
        assert not x.any()
        want = model.expect(x)
        got = a.sample_buses(n, SR, 3)
        assert_bits_equal_finite(got, want, "unit bands over a silent bus, fill %d" % fill)
        assert_bits_equal_finite(got[[0, 2]], x[[0, 2]], "the buses without an EQ")
        _states(a, model, "the unit bands, fill %d" % fill)


def test_range_checks_on_a_handle():
    check_ranges(s2.Synth(8, max_frames=64))


def test_a_handle_that_never_had_an_eq_and_the_timing_entry():
    """s2r_debug_bus_eq_ms: -1 without s2r_set_timing; under it 0 after a bus fill and a master fill of a handle that never had an EQ,
    whose outputs are the twin's and which holds no staging buffer for one; and the EQ kernel's time once an EQ is set"""
    a, b = _handles()
    ms, alloc = a.L.s2r_debug_bus_eq_ms, a.L.s2r_debug_bus_eq_allocated
    ms.restype, ms.argtypes = C.c_float, [C.c_void_p]
    alloc.restype, alloc.argtypes = C.c_int, [C.c_void_p]
    _events((a, b), V, 0)
    assert_bits_equal_finite(a.sample_buses(300, SR, 3), b.sample_buses(300, SR, 3), "no EQ, timing off")
    assert ms(a.h) == -1.0
    a.set_timing(True)
    _events((a, b), V, 1)
    assert_bits_equal_finite(a.sample_buses(300, SR, 3), b.sample_buses(300, SR, 3), "no EQ, bus fill under timing")
    assert ms(a.h) == 0.0
    _events((a, b), V, 2)
    (ma, sa), (mb, sb) = a.sample_master(300, SR, 3), b.sample_master(300, SR, 3)
    assert_bits_equal_finite(ma, mb, "no EQ, master fill under timing")
    assert_bits_equal_finite(sa, sb, "no EQ, the stems of a master fill")
    assert ms(a.h) == 0.0 and alloc(a.h) == 0
    a.set_bus_eq(1, _coeffs(4, 1))
    assert alloc(a.h) == 1
    a.sample_buses(300, SR, 3)
    assert 0.0 < ms(a.h) < 100.0
    a.sample_buses(300, SR, 1)                                   # the EQ idle: no kernel
    assert ms(a.h) == 0.0
