"""The per-bus dynamics on the device.  Twin handles are fed the same events, one with dynamics and one without; the
twin's bus output is what enters the dynamics stage, for the bus and for its key bus, and the expectation is the rule on the host
(s2.dynamics_reference, which tests/test_dyn_host.py holds to a numpy float32 model on bits) with the gain carried from call to call
(DynModel); in front of it comes the EQ's model (test_gpu_eq.EqModel) and behind it the models of the stages that follow.

The kernel is a pipeline of three stages a tile of T frames apart (s2r_debug_dyn_tile), so the call lengths are 1, 2 and 3 frames, T - 1,
T, T + 1, 2T + 1, 3T (as many tiles as the pipeline is deep) and max_frames.  Handles, events and the one-pole bank are
tests/test_gpu_reverb.py's.  Every comparison is on bits with no NaN allowance (helpers.assert_bits_equal_finite)."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_dyn_host import LO, P, bits, check_ranges
from test_gpu_buses import ubits
from test_gpu_chorus import SHAPES, ChorusModel
from test_gpu_delay import DelayModel
from test_gpu_eq import EqModel, _coeffs
from test_gpu_limiter import Lim
from test_gpu_master import Master
from test_gpu_reverb import SR, V, Model, _bank, _events, _handles, _ir, _timed
from test_master_host import np_meters

pytestmark = pytest.mark.gpu
F = np.float32

T = 256                                                          # S2R_DYN_TILE (csrc/s2r_device.h); test_the_tile_is_the_kernels holds it to the library
FRAMES = [1024, 1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 3 * T, 3, 1, 1024]
# (n_buses, key bus per bus; None: no dynamics on that bus): compressors (the bus keys itself) and duckers mixed, buses without among them,
# and in the last row buses 6 and 7, which sound through sends alone, as keys and as keyed
MATRIX = [(1, (0,)), (2, (1, None)), (3, (0, None, 0)), (8, (0, 3, None, 3, 6, None, 7, 1))]
UNDER_ONE = float(np.nextafter(F(1.0), F(0.0)))
# (attack, release) by name, made when a test asks (a test module must not load the library while it is imported)
COEFS = {"zero": lambda: (0.0, 0.0), "1ms-100ms": lambda: (float(s2.dynamics_coef(1.0, SR)), float(s2.dynamics_coef(100.0, SR))),
         "under-one": lambda: (UNDER_ONE, float(np.nextafter(F(UNDER_ONE), F(0.0))))}
# (ratio, knee_db, makeup_db) by bus; every makeup moves the gain at silence off 1, so that a bus with dynamics differs from the twin's in any call
RATIOS = [(4.0, 6.0, 3.0), (float("inf"), 0.0, -1.5), (2.0, 12.0, 6.0), (8.0, 3.0, -3.0)]


def _tile():
    L = s2.load_library()
    L.s2r_debug_dyn_tile.restype, L.s2r_debug_dyn_tile.argtypes = C.c_uint32, []
    return int(L.s2r_debug_dyn_tile())


def _level(x):
    """p[n] of a bus [N, 2]"""
    return np.abs(x).max(axis=1)


def _targets(curve, p):
    """the rule's step 2 over an array of levels, in float32 operations: the same three roundings per level as the rule"""
    p = np.asarray(p, dtype=F)
    u = np.clip(p.view(np.uint32).astype(np.int64) - LO, 0, (512 << 19) - 1)
    i, f = (u >> 19).astype(np.int64), (u & 0x7FFFF).astype(F) * F(2.0 ** -19)
    t = curve[i] + f * (curve[i + 1] - curve[i])
    return np.where(p >= F(2.0 ** -24), np.where(p >= F(256.0), curve[P - 1], t), curve[0]).astype(F)


def _curve_at_the_median(x_key, bus, slow=False):
    """the threshold at the median of the key's level over the twin's first call: half of that call's frames lie above it.  `slow`, for
    coefficients just under 1: the gain then all but stays at curve[0], the attack branch is taken by every frame the curve compresses
    at all and the release branch by the others alone, so the median rule leaves the release branch whatever lies under the knee —
    9 % of the frames when it was tried; there the knee BEGINS at the 60th percentile instead: six frames in ten are not compressed"""
    p = _level(x_key)
    ratio, knee, makeup = RATIOS[bus % len(RATIOS)]
    at = float(np.percentile(p, 60.0)) if slow else float(np.median(p))
    assert at > 2.0 ** -20, "the key bus is all but silent in the first call"
    return s2.dynamics_curve(20.0 * np.log10(at) + (knee / 2.0 if slow else 0.0), ratio, knee, makeup)


class DynModel:
    """the dynamics of a handle on the host: per bus the key, the table, the coefficients and the carried gain; and what the parity
    conditions count: frames, frames whose target lies below curve[0], frames of either branch of the ballistics"""

    def __init__(self):
        self.d = {}

    def set(self, bus, key, curve, a_att, a_rel):
        self.d[bus] = dict(key=key, curve=np.array(curve, dtype=F), a=(F(a_att), F(a_rel)), y=F(curve[0]), mn=F(1.0), n=0, below=0, att=0, rel=0)

    def runs(self, bus, n_buses):
        return bus in self.d and bus < n_buses and self.d[bus]["key"] < n_buses

    def expect(self, x):
        """what the stage makes of a call whose buses enter it as x [n_buses, N, 2]; the gains of its buses move on"""
        want = x.copy()
        for b, f in self.d.items():
            if not self.runs(b, x.shape[0]):
                continue                                         # idle in this call
            key = x[f["key"]]
            ys = s2.dynamics_reference(f["curve"], f["a"][0], f["a"][1], key, np.ones_like(key), f["y"])[0][:, 0]     # x = 1: the gains themselves
            t = _targets(f["curve"], _level(key))
            before = np.concatenate([[f["y"]], ys[:-1]])
            f["n"] += key.shape[0]; f["below"] += int((t < f["curve"][0]).sum()); f["att"] += int((t < before).sum()); f["rel"] += int((t >= before).sum())
            want[b], f["y"], f["mn"] = s2.dynamics_reference(f["curve"], f["a"][0], f["a"][1], key, x[b], f["y"])
            assert bits(f["y"]) == bits(ys[-1]) and bits(f["mn"]) == bits(ys.min())
        return want


def _set(a, model, bus, key, curve, a_att, a_rel):
    a.set_bus_dynamics(bus, key, curve, a_att, a_rel)
    got = a.get_bus_dynamics(bus)
    assert got[0] == key and np.array_equal(bits(got[1]), bits(curve)) and bits(got[2]) == bits(F(a_att)) and bits(got[3]) == bits(F(a_rel))
    model.set(bus, key, curve, a_att, a_rel)


def _fill(a, b, model, n, nb, what, differs=True):
    """one call on both handles: the buses with dynamics against the model over the twin's, the others against the twin's"""
    x = b.sample_buses(n, SR, nb)
    assert np.isfinite(x).all()
    want = model.expect(x)
    got = a.sample_buses(n, SR, nb)
    assert_bits_equal_finite(got, want, what)
    for bus in range(nb):
        if model.runs(bus, nb):
            assert ubits(x[bus]).any(), "%s: bus %d is silent" % (what, bus)
            if differs:
                assert not np.array_equal(ubits(got[bus]), ubits(x[bus])), "%s: the dynamics on bus %d change no bit" % (what, bus)
        else:
            assert_bits_equal_finite(got[bus], x[bus], "%s: bus %d, which runs no dynamics" % (what, bus))
    return x, got


def _states(a, model, what):
    for bus, f in model.d.items():
        assert bits(a.bus_dynamics_state(bus)) == bits(f["y"]), "%s: gain of bus %d: %r, not %r" % (what, bus, a.bus_dynamics_state(bus), f["y"])
        assert bits(a.bus_dynamics_meter(bus)) == bits(f["mn"]), "%s: meter of bus %d: %r, not %r" % (what, bus, a.bus_dynamics_meter(bus), f["mn"])


def test_the_tile_is_the_kernels():
    assert _tile() == T


@pytest.mark.parametrize("coefs", list(COEFS))
@pytest.mark.parametrize("n_buses,keys", MATRIX)
def test_dynamics_are_the_rule_over_the_twins_buses(n_buses, keys, coefs):
    """the parity matrix: calls of max_frames, then 1, 2, 3, T - 1, T, T + 1, 2T + 1, 3T, 3, 1 frames and max_frames again on one pair
    of handles, gain and meter read back after each.  The thresholds come from the twin's first call — the median of each key's level —
    and are set before the other handle's first call."""
    a, b = _handles()
    model = DynModel()
    a_att, a_rel = COEFS[coefs]()
    steps = []
    for fill, n in enumerate(FRAMES):
        _events((a, b), V, fill)
        what = "%d buses, keys %s, %s, fill %d of %d frames" % (n_buses, keys, coefs, fill, n)
        x = b.sample_buses(n, SR, n_buses)
        if fill == 0:
            for bus, key in enumerate(keys):
                if key is not None:
                    _set(a, model, bus, key, _curve_at_the_median(x[key], bus, slow=coefs == "under-one"), a_att, a_rel)
        want = model.expect(x)
        got = a.sample_buses(n, SR, n_buses)
        gains = [(bus, a.bus_dynamics_state(bus), f["y"], a.bus_dynamics_meter(bus), f["mn"]) for bus, f in model.d.items()]
        steps.append((what, x, want, got, gains))
    if coefs != "zero":                                          # on the model, before anything is compared
        for bus, f in model.d.items():
            print("%d buses, %s, bus %d: %d frames, %d below curve[0], %d attack, %d release" % (n_buses, coefs, bus, f["n"], f["below"], f["att"], f["rel"]))
        for bus, f in model.d.items():
            assert 4 * f["below"] >= f["n"], "bus %d: fewer than a quarter of the frames are compressed" % bus
            assert 10 * f["att"] >= f["n"] and 10 * f["rel"] >= f["n"], "bus %d: a branch of the ballistics takes under a tenth of the frames" % bus
    for what, x, want, got, gains in steps:
        assert np.isfinite(x).all()
        assert_bits_equal_finite(got, want, what)
        for bus in range(n_buses):
            if bus in model.d:
                assert ubits(x[bus]).any(), "%s: bus %d is silent" % (what, bus)
                assert not np.array_equal(ubits(got[bus]), ubits(x[bus])), "%s: the dynamics on bus %d change no bit" % (what, bus)
            else:
                assert_bits_equal_finite(got[bus], x[bus], "%s: bus %d, which carries no dynamics" % (what, bus))
        for bus, y, y_want, mn, mn_want in gains:
            assert bits(y) == bits(y_want), "%s: gain of bus %d: %r, not %r" % (what, bus, y, y_want)
            assert bits(mn) == bits(mn_want), "%s: meter of bus %d: %r, not %r" % (what, bus, mn, mn_want)


def test_a_curve_of_ones_passes_every_bit():
    """no model in the loop: a constant curve of 1.0 keeps y = 1 whatever the key and the coefficients, and x * 1 is x in every bit —
    over sounding buses and, on a pair of handles that never start a voice, over silence, the sign of a zero included"""
    ones = np.ones(P, dtype=F)
    for sounding in (True, False):
        a, b = _handles()
        a.set_bus_dynamics(0, 0, ones, 0.9, 0.999)
        a.set_bus_dynamics(1, 2, ones, 0.0, 0.0)
        for fill, n in enumerate([300, 1, T + 1]):
            if sounding:
                _events((a, b), V, fill)
            x = b.sample_buses(n, SR, 3)
            assert ubits(x).any() if sounding else not x.any()
            assert_bits_equal_finite(a.sample_buses(n, SR, 3), x, "a curve of ones, fill %d, sounding %s" % (fill, sounding))
            assert a.bus_dynamics_state(0) == 1.0 and a.bus_dynamics_meter(1) == 1.0


def test_a_curve_of_halves_with_zero_coefficients_halves_the_twin():
    a, b = _handles()
    half = np.full(P, 0.5, dtype=F)
    a.set_bus_dynamics(1, 1, half, 0.0, 0.0)
    a.set_bus_dynamics(2, 0, half, 0.0, 0.0)
    for fill, n in enumerate([300, 2, 3 * T]):
        _events((a, b), V, fill)
        x = b.sample_buses(n, SR, 3)
        got = a.sample_buses(n, SR, 3)
        assert_bits_equal_finite(got[1:], x[1:] * F(0.5), "half the twin, fill %d" % fill)
        assert_bits_equal_finite(got[0], x[0], "the bus beside them")
        assert ubits(x[1:]).any() and a.bus_dynamics_meter(2) == 0.5


def test_a_ducker_follows_the_send_that_feeds_its_key():
    """bus 0 ducked by bus 6, which sounds through program 0's send alone: on a second pair of handles the send is a tenth, bus 0
    enters the stage the same and leaves it different"""
    a, b, c, d = _handles() + _handles()
    for syn in (c, d):
        syn.set_program_send(0, 0.05, 6)
    ma, mc = DynModel(), DynModel()
    _events((a, b, c, d), V, 0)
    xb, xd = b.sample_buses(600, SR, 7), d.sample_buses(600, SR, 7)
    assert_bits_equal_finite(xb[0], xd[0], "bus 0 in front of the stage, under either send")
    assert not np.array_equal(ubits(xb[6]), ubits(xd[6])) and ubits(xd[6]).any()
    curve = _curve_at_the_median(xb[6], 0)
    _set(a, ma, 0, 6, curve, *COEFS["1ms-100ms"]())
    _set(c, mc, 0, 6, curve, *COEFS["1ms-100ms"]())
    ga, gc = a.sample_buses(600, SR, 7), c.sample_buses(600, SR, 7)
    assert_bits_equal_finite(ga, ma.expect(xb), "ducked by the send at 0.5")
    assert_bits_equal_finite(gc, mc.expect(xd), "ducked by the send at 0.05")
    assert not np.array_equal(ubits(ga[0]), ubits(gc[0])) and a.bus_dynamics_meter(0) < c.bus_dynamics_meter(0)
    assert_bits_equal_finite(ga[6], xb[6], "the key bus itself passes")


def _compressors(a, b, model, layout, first=600, nb=None, coefs="1ms-100ms"):
    """a first call on the twin alone gives the thresholds; `a` renders the same frames without dynamics (and must equal the twin), then
    takes the dynamics of `layout`: {bus: key}"""
    nb = nb or max(max(layout), max(layout.values())) + 1
    _events((a, b), V, 0)
    x = b.sample_buses(first, SR, nb)
    assert_bits_equal_finite(a.sample_buses(first, SR, nb), x, "before any dynamics")
    for bus, key in layout.items():
        _set(a, model, bus, key, _curve_at_the_median(x[key], bus), *COEFS[coefs]())
    return x


def test_a_run_of_short_calls_is_one_long_call():
    """no model in the loop: four handles, two with the same dynamics; one of each kind renders the same frames in a run of calls, the
    other in one call.  The render kernels work in chunks of 16 frames counted from the start of a call, so the mixdown itself is one
    stream only where calls are cut at multiples of 16 — which is asserted on the handles without dynamics — and the cuts here are
    such.  On bits, the two handles with the dynamics agree, outputs and gains; the meter of the long call is the least of the short ones'"""
    a, b, c, d = _handles() + _handles()
    curve = s2.dynamics_curve(-30.0, 4.0, 6.0, 3.0)
    for syn in (a, c):
        syn.set_bus_dynamics(0, 0, curve, *COEFS["1ms-100ms"]())
        syn.set_bus_dynamics(1, 3, curve, *COEFS["under-one"]())
        syn.set_bus_dynamics(3, 1, curve, *COEFS["zero"]())
    cuts = [16, 48, 16, T, T + 16, 16, 32, T - 16, 64]
    total = sum(cuts)
    assert total <= 1024 and all(n % 16 == 0 for n in cuts)
    _events((a, b, c, d), V, 0)
    short_dyn, meters = [], []
    for n in cuts:
        short_dyn.append(a.sample_buses(n, SR, 4))
        meters.append([a.bus_dynamics_meter(q) for q in (0, 1, 3)])
    short_dyn = np.concatenate(short_dyn, axis=1)
    short_dry = np.concatenate([b.sample_buses(n, SR, 4) for n in cuts], axis=1)
    long_dyn, long_dry = c.sample_buses(total, SR, 4), d.sample_buses(total, SR, 4)
    assert_bits_equal_finite(short_dry, long_dry, "without dynamics: the mixdown in short calls and in one")
    assert_bits_equal_finite(short_dyn, long_dyn, "with the dynamics: short calls and one long call")
    assert_bits_equal_finite(short_dyn[2], long_dry[2], "the bus without dynamics")
    for k, bus in enumerate((0, 1, 3)):
        assert not np.array_equal(ubits(long_dyn[bus]), ubits(long_dry[bus]))
        assert bits(a.bus_dynamics_state(bus)) == bits(c.bus_dynamics_state(bus)), "the gain of bus %d after both" % bus
        assert bits(min(m[k] for m in meters)) == bits(c.bus_dynamics_meter(bus))


@pytest.mark.parametrize("frames", [250, 64])
def test_events_inside_a_fill_and_sliced_rows(frames, monkeypatch):
    """note_ons at frames 16 and 48 split the call into segments and a rows buffer of 48 frames slices them further: the stage sees the
    call as one stream"""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    a, b = _handles(max_frames=256)
    model = DynModel()
    _compressors(a, b, model, {0: 0, 3: 1}, first=256)
    for fill in range(1, 4):
        _events((a, b), V, fill)
        _timed((a, b), fill)
        _fill(a, b, model, frames, 4, "events at 16 and 48, slices of 48, %d frames, fill %d" % (frames, fill))
    _states(a, model, "events and slices")
    a.L.s2r_debug_pan_slice.restype = C.c_uint32
    a.L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    assert a.L.s2r_debug_pan_slice(a.h) == 48


def test_a_send_only_bus_with_dynamics_while_a_fader_ramps():
    """bus 6 of eight sounds through program 0's send alone and carries a compressor; program 0's fader moves across the second and
    third call — on both handles, so the twin's bus 6 enters the stage under the same sends and ramps"""
    a, b = _handles()
    model = DynModel()
    _compressors(a, b, model, {6: 6}, nb=8)
    walk = [(1.0, 0.0), (0.25, 1.0), (0.7, -0.5), (0.7, -0.5)]
    for fill, n in enumerate([300, 1000, 17, 64]):
        _events((a, b), V, fill + 1)
        for syn in (a, b):
            syn.set_program_fader(0, *walk[fill])
        _fill(a, b, model, n, 8, "send-only bus under a fader ramp, fill %d" % fill)
        f = a.get_program_fader(0)
        assert f == b.get_program_fader(0) and f[:2] == f[2:]    # committed on both
    _states(a, model, "under the ramps")


def test_every_route_with_the_eq_and_the_dynamics_on():
    """Handle `a` walks all 24 rows of s2r_post_route's table with EQs and dynamics on all three buses (bus 1 ducked by bus 0), T frames
    a call — a bus fill, a master fill and a master fill under the limiter, each with every subset of chorus, delay and reverb, master
    fills with and without stems —; its twin `b` makes a plain bus fill of the same frames every time.  Every step's expectation is
    the chain of the models: EQ, dynamics, chorus, delay, reverb, master section, limiter.  Everything the device returns is
    collected first, then compared."""
    a, b = _handles()
    eq, dy, ch, dl, rv, mm = EqModel(), DynModel(), ChorusModel(), DelayModel(), Model(), Master()
    for bus, nb in enumerate((2, 4, 1)):
        c = _coeffs(nb, bus + 1)
        a.set_bus_eq(bus, c)
        eq.set(bus, c)
    curve = s2.dynamics_curve(-30.0, 4.0, 6.0, 3.0)
    for bus, key in enumerate((0, 0, 2)):
        _set(a, dy, bus, key, curve, *COEFS["1ms-100ms"]())
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
        z = dy.expect(y)
        assert all(not np.array_equal(ubits(z[q]), ubits(y[q])) for q in range(nb))
        return rv.expect(dl.expect(ch.expect(z)))

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
        cmp["gains"] = (np.array([a.bus_dynamics_state(q) for q in range(3)], dtype=F), np.array([dy.d[q]["y"] for q in range(3)], dtype=F))
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
            what = "%d: %s, EQ and dynamics on, chorus %s, delay %s, reverb %s" % ((k + 1, kind) + tuple("on" if o else "off" for o in on))
            if kind == "bus fill":
                bus_fill(what, T)
            else:
                master_fill(what, T, stems=j % 2 == 0)
            k += 1
    assert k == 24 and len(lims) == 1 and lims[0].limited() > 0.0       # on the model, before anything is compared: the walk limits
    for what, cmp in steps:
        for name, (got, want) in cmp.items():
            assert_bits_equal_finite(got, want, "%s: %s" % (what, name))
    mm.check_committed(a)
    _states(a, dy, "after the walk")
    for bus, f in eq.e.items():
        assert_bits_equal_finite(a.bus_eq_state(bus), f["st"], "the EQ's state after the walk")


def test_a_key_past_the_calls_buses_idles_the_dynamics():
    """bus 1 is keyed by bus 5: in calls of three buses it passes, its crafted gain stays and its meter too; bus 0 beside it runs; a
    call of eight buses goes on from the crafted gain.  Dynamics on bus 6 are idle in the short calls as well"""
    a, b = _handles()
    model = DynModel()
    _compressors(a, b, model, {0: 0, 1: 5, 6: 6}, nb=8)
    a.set_bus_dynamics_state(1, 0.375)
    a.set_bus_dynamics_state(6, 0.625)
    model.d[1]["y"], model.d[6]["y"] = F(0.375), F(0.625)
    for fill, n in enumerate([300, 2, T + 1, 17]):
        _events((a, b), V, fill + 1)
        x, got = _fill(a, b, model, n, 3, "a key past the call's buses, fill %d" % fill)
        assert_bits_equal_finite(got[1], x[1], "the bus whose key is not in the call, fill %d" % fill)
    _states(a, model, "two idle, one running")
    assert a.bus_dynamics_state(1) == F(0.375) and a.bus_dynamics_state(6) == F(0.625) and a.bus_dynamics_meter(1) == 1.0
    _events((a, b), V, 5)
    _fill(a, b, model, 100, 8, "eight buses: the idle dynamics wake from their crafted gains")
    _states(a, model, "after the call of eight buses")
    assert a.bus_dynamics_state(1) != F(0.375) and a.bus_dynamics_meter(1) < 1.0


def test_new_parameters_keep_the_gain_and_a_set_resets_it():
    a, b = _handles()
    model = DynModel()
    _compressors(a, b, model, {1: 1}, nb=2)
    _events((a, b), V, 1)
    _fill(a, b, model, 300, 2, "before the threshold moves")
    y = a.bus_dynamics_state(1)
    assert y < model.d[1]["curve"][0]                            # compressing
    moved = s2.dynamics_curve(-50.0, 8.0, 0.0, 0.0)
    a.set_bus_dynamics_params(1, 0, moved, 0.5, 0.75)
    f = model.d[1]
    f["key"], f["curve"], f["a"] = 0, moved, (F(0.5), F(0.75))
    assert bits(a.bus_dynamics_state(1)) == bits(y), "the gain under new parameters"
    got = a.get_bus_dynamics(1)
    assert got[0] == 0 and np.array_equal(bits(got[1]), bits(moved)) and (got[2], got[3]) == (F(0.5), F(0.75))
    _events((a, b), V, 2)
    _fill(a, b, model, 300, 2, "after s2r_set_bus_dynamics_params")
    _states(a, model, "after the threshold moved")
    _set(a, model, 1, 1, moved, 0.5, 0.75)                       # setting them again resets the gain to curve[0]
    assert bits(a.bus_dynamics_state(1)) == bits(moved[0]) and a.bus_dynamics_meter(1) == 1.0
    _events((a, b), V, 3)
    _fill(a, b, model, 64, 2, "after s2r_set_bus_dynamics")
    _states(a, model, "from the gain at silence")


def test_checkpoint_in_the_middle_of_a_release():
    """a ducker whose key has just fallen silent is releasing; state, pans, mix, sends, the dynamics' parameters and gain go into a
    fresh handle: the next fills are equal"""
    a, b = _handles(max_frames=512)
    model = DynModel()
    _compressors(a, b, model, {1: 1, 0: 1}, first=400, nb=2)
    _events((a, b), V, 1)
    _fill(a, b, model, 200, 2, "before the checkpoint")
    quiet = np.full(P, 1.0, dtype=F)                             # from here on the target is 1: both gains release towards it
    for bus in (0, 1):
        a.set_bus_dynamics_params(bus, 1, quiet, *COEFS["1ms-100ms"]())
        model.d[bus]["curve"] = quiet
    _events((a, b), V, 2)
    _fill(a, b, model, 100, 2, "the release begins")
    y = a.bus_dynamics_state(1)
    assert y < 1.0 and a.bus_dynamics_meter(1) < y               # in mid-release: rising, not there yet
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    c = s2.Synth(V, max_frames=512, block_voices=64)
    c.set_patch_bank(_bank())
    c.import_state(state)
    c.set_voice_pans(pans)
    c.set_voice_mix(gains, buses)
    c.set_voice_sends(sends, sbuses)
    for bus in (0, 1):
        c.set_bus_dynamics(bus, *a.get_bus_dynamics(bus))
        c.set_bus_dynamics_state(bus, a.bus_dynamics_state(bus))
    for k, n in enumerate([100, 400]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        _, got = _fill(a, b, model, n, 2, "the checkpointed handle, fill %d" % k)
        assert_bits_equal_finite(c.sample_buses(n, SR, 2), got, "the resumed handle, fill %d" % k)
    for bus in (0, 1):
        assert bits(c.bus_dynamics_state(bus)) == bits(a.bus_dynamics_state(bus))
    assert a.bus_dynamics_state(1) > y                           # still rising
    # the dynamics are the bus's: a new bank, a program change and an imported state leave them and their gain alone
    keep = a.bus_dynamics_state(1)
    a.set_patch_bank(_bank())
    a.program_change(3)
    a.import_state(state)
    assert np.array_equal(bits(a.get_bus_dynamics(1)[1]), bits(quiet)) and bits(a.bus_dynamics_state(1)) == bits(keep)


def test_refusals_removal_and_the_other_fills():
    """a fill refused before any launch leaves gain and meter untouched, in a bus fill and in a master fill; the panned, mono and stereo
    fills ignore dynamics; after a removal the bus is the twin's on bits again; a device-list handle refuses every entry and renders on"""
    a, b = _handles(max_frames=256)
    model = DynModel()
    _compressors(a, b, model, {0: 1}, first=256)
    _events((a, b), V, 1)
    _fill(a, b, model, 100, 2, "before the refusals")
    before, meter = a.bus_dynamics_state(0), a.bus_dynamics_meter(0)
    assert before != model.d[0]["curve"][0] and meter < 1.5
    L, h = a.L, a.h
    out, lr = np.empty(2 * 2 * 300, dtype=F), np.empty(2 * 300, dtype=F)
    p, q = out.ctypes.data_as(s2s._f32p), lr.ctypes.data_as(s2s._f32p)
    assert L.s2r_fill_buses(h, p, 2 * 2 * 100 - 1, 2, 100, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_buses(h, p, out.size, 9, 16, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_buses(h, p, out.size, 2, 257, SR) == s2s.S2R_ERR_TOO_MANY_FRAMES
    assert L.s2r_fill_master(h, q, p, 2 * 2 * 100 - 1, 2, 100, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_master(h, q, p, out.size, 2, 257, SR) == s2s.S2R_ERR_TOO_MANY_FRAMES
    assert bits(a.bus_dynamics_state(0)) == bits(before) and bits(a.bus_dynamics_meter(0)) == bits(meter)
    # the other fills
    assert_bits_equal_finite(a.sample_panned(100, SR), b.sample_panned(100, SR), "panned fill beside dynamics")
    assert_bits_equal_finite(a.sample(np.empty(64, dtype=F), SR), b.sample(np.empty(64, dtype=F), SR), "mono fill beside dynamics")
    assert_bits_equal_finite(a.sample_stereo(33, SR), b.sample_stereo(33, SR), "stereo copy beside dynamics")
    assert bits(a.bus_dynamics_state(0)) == bits(before) and bits(a.bus_dynamics_meter(0)) == bits(meter)
    _events((a, b), V, 2)
    _fill(a, b, model, 64, 2, "after the refusals and the other fills")
    # removal
    a.clear_bus_dynamics(0)
    del model.d[0]
    assert a.get_bus_dynamics(0) is None and a.bus_dynamics_meter(0) == 1.0
    _events((a, b), V, 3)
    x = b.sample_buses(64, SR, 2)
    assert_bits_equal_finite(a.sample_buses(64, SR, 2), x, "no dynamics left: the twin's")
    # a device list
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    one = s2.Synth(512, max_frames=64, mix_groups=2)
    for syn in (multi, one):
        for v in range(512):
            syn.note_on(36 + v % 61)
    ones = np.ones(P, dtype=F)
    op, n = ones.ctypes.data_as(s2s._f32p), C.c_uint32()
    assert multi.L.s2r_set_bus_dynamics(multi.h, 0, 0, op, 0.5, 0.5) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_clear_bus_dynamics(multi.h, 0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_dynamics_params(multi.h, 0, 0, op, 0.5, 0.5) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_dynamics(multi.h, 0, C.byref(n), None, None, 0, None, None) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_dynamics_state(multi.h, 0, op, 1) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_dynamics_state(multi.h, 0, op, 1) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_dynamics_meter(multi.h, 0, op) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        multi.set_bus_dynamics(0, 0, ones, 0.5, 0.5)
    assert err.value.status == s2s.S2R_ERR_INVALID
    x, y = multi.sample(np.empty(64, dtype=F), SR), one.sample(np.empty(64, dtype=F), SR)
    assert np.abs(y).max() > 0.0
    assert_bits_equal_finite(x, y, "the device-list handle after the refused dynamics calls")


def test_a_master_fill_applies_the_dynamics():
    """stems and master of s2r_fill_master against the models: the dynamics, then the master section"""
    a, b = _handles()
    model, mm = DynModel(), Master()
    _compressors(a, b, model, {0: 2, 2: 2}, nb=3)
    for fill, n in enumerate([T + 1, 1, 3 * T]):
        _events((a, b), V, fill + 1)
        y = model.expect(b.sample_buses(n, SR, 3))
        got, st = a.sample_master(n, SR, 3, stems=True)
        assert_bits_equal_finite(st, y, "the stems of a master fill, fill %d" % fill)
        assert_bits_equal_finite(got, mm.expect(y), "the master, fill %d" % fill)
        _states(a, model, "master fill %d" % fill)


def test_range_checks_on_a_handle():
    check_ranges(s2.Synth(8, max_frames=64))


def test_a_handle_that_never_had_dynamics_and_the_timing_entry():
    """s2r_debug_dyn_ms: -1 without s2r_set_timing; under it 0 after a bus fill and a master fill of a handle that never had dynamics,
    whose outputs are the twin's and which holds nothing for them; and the kernel's time once dynamics are set"""
    a, b = _handles()
    ms, alloc = a.L.s2r_debug_dyn_ms, a.L.s2r_debug_dyn_allocated
    ms.restype, ms.argtypes = C.c_float, [C.c_void_p]
    alloc.restype, alloc.argtypes = C.c_int, [C.c_void_p]
    _events((a, b), V, 0)
    assert_bits_equal_finite(a.sample_buses(300, SR, 3), b.sample_buses(300, SR, 3), "no dynamics, timing off")
    assert ms(a.h) == -1.0
    a.set_timing(True)
    _events((a, b), V, 1)
    assert_bits_equal_finite(a.sample_buses(300, SR, 3), b.sample_buses(300, SR, 3), "no dynamics, bus fill under timing")
    assert ms(a.h) == 0.0
    _events((a, b), V, 2)
    (ma, sa), (mb, sb) = a.sample_master(300, SR, 3), b.sample_master(300, SR, 3)
    assert_bits_equal_finite(ma, mb, "no dynamics, master fill under timing")
    assert_bits_equal_finite(sa, sb, "no dynamics, the stems of a master fill")
    assert ms(a.h) == 0.0 and alloc(a.h) == 0
    a.set_bus_dynamics(1, 2, s2.dynamics_curve(-30.0, 4.0), 0.9, 0.99)
    assert alloc(a.h) == 1
    a.sample_buses(300, SR, 3)
    assert 0.0 < ms(a.h) < 100.0
    a.sample_buses(300, SR, 2)                                   # the key is past the call's buses: idle, no kernel
    assert ms(a.h) == 0.0
