"""The per-bus drive on the device.  Twin handles on pools of 32 voices are fed the same events, one with drives and
one without; the twin's bus output is what enters the chain, and the expectation is the rule on the host (s2.drive_reference, which
tests/test_drive_host.py holds to a numpy float32 model on bits) with the history carried from call to call (DriveModel), behind the
models of the stages in front of it.

The kernel spreads a call over tiles of T output frames (s2r_debug_drive_tile), each with the 32 input frames in front of it, so the
call lengths are 1, 2, 15, 16, 17, 31, 32, 33 — around the latency and the history —, T - 1, T, T + 1, 2T + 5 and 1024 = max_frames.
In every parity call `pre` is chosen from the twin's bus — one over the median magnitude of the oversampled samples the call computes —
so that both branches of the clamp run: the model must show at least a tenth of those samples clamped and a tenth not (tune).
Handles, events and the one-pole bank are tests/test_gpu_reverb.py's.  Every comparison is on bits with no NaN allowance
(helpers.assert_bits_equal_finite)."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_drive_host import KINDS, check_ranges, random_table
from test_room_host import FLAT, SMALL, bits
from test_gpu_buses import ubits
from test_gpu_chorus import SHAPES, ChorusModel
from test_gpu_delay import DelayModel
from test_gpu_dyn import DynModel
from test_gpu_eq import EqModel, _coeffs
from test_gpu_limiter import Lim
from test_gpu_master import Master
from test_gpu_reverb import SR, Model, _bank, _events, _handles as _reverb_handles, _ir, _timed
from test_gpu_room import LEVELS as ROOM_LEVELS, RoomModel
from test_master_host import np_meters

pytestmark = pytest.mark.gpu
F = np.float32

V = 32                                                           # voices of a pool
T = 240                                                          # S2R_DRIVE_TILE (csrc/s2r_device.h); test_the_tile_is_the_kernels holds it to the library
H, LAT = s2.DRIVE_HISTORY, s2.DRIVE_LATENCY
FRAMES = [1024, 1, 2, 15, 16, 17, 31, 32, 33, T - 1, T, T + 1, 2 * T + 5, 1024]
# (n_buses, what each bus carries: a curve by name with (dry, wet), or None); in the last row buses 6 and 7 sound through sends alone
MATRIX = [(1, ("tanh:wet",)), (2, (None, "random:mix")), (3, ("hard:mix", None, "fold:wet")),
          (8, ("cubic:wet", "linear:mix", None, "random:wet", "tanh:mix", None, "fold:mix", "hard:wet"))]
MIX = {"wet": (0.0, 1.0), "mix": (0.5, 0.75)}


def _curve(name):
    return random_table() if name == "random" else s2.drive_curve(*[k for k in KINDS if k[0] == name][0][1:])


def _handles(max_frames=1024):
    return _reverb_handles(voices=V, max_frames=max_frames)


def _tile():
    L = s2.load_library()
    L.s2r_debug_drive_tile.restype, L.s2r_debug_drive_tile.argtypes = C.c_uint32, []
    return int(L.s2r_debug_drive_tile())


def oversampled(x, hist):
    """u of the rule in float32 for the frames a call of x [N, 2] computes, -16 .. N - 1: [2, 4 * (N + 16)]"""
    g = F(4.0) * s2.drive_taps()
    nf = x.shape[0] + LAT
    out = np.zeros((2, nf, 4), dtype=F)
    for c in range(2):
        xs = np.concatenate([hist[:, c], x[:, c]]).astype(F)
        for p in range(4):
            u = np.zeros(nf, dtype=F)
            for j in range((64 - p) // 4 + 1):
                u = u + g[p + 4 * j] * xs[LAT - j:LAT - j + nf]
            out[c, :, p] = u
    return out.reshape(2, -1)


class DriveModel:
    """the drives of a handle on the host: per bus the table, the levels and the carried history"""

    def __init__(self):
        self.d = {}

    def set(self, bus, curve, pre, dry, wet):
        self.d[bus] = dict(curve=np.array(curve, dtype=F), pre=F(pre), dry=F(dry), wet=F(wet), hist=np.zeros((H, 2), dtype=F))

    def tune(self, a, x, what):
        """pre of every drive among the call's buses from the bus as it enters, x [n_buses, N, 2], on the handle and here: a condition on
        the inputs, met before the device runs"""
        for b, f in self.d.items():
            if b >= x.shape[0]:
                continue
            au = np.abs(oversampled(x[b], f["hist"]))
            assert (au > 0.0).mean() > 0.5, "%s: bus %d is silent" % (what, b)
            pre = F(min(1024.0, 1.0 / float(np.median(au))))
            clamped = float((np.abs(pre * au) >= 1.0).mean())
            assert 0.1 <= clamped <= 0.9, "%s: bus %d: %.3f of the oversampled samples clamped at pre %r" % (what, b, clamped, pre)
            a.set_bus_drive_params(b, None, pre, f["dry"], f["wet"])
            f["pre"] = pre

    def expect(self, x):
        """what the stage makes of a call whose buses enter it as x [n_buses, N, 2]; the histories of its buses move on"""
        want = x.copy()
        for b, f in self.d.items():
            if b >= x.shape[0]:
                continue                                         # idle in this call
            want[b], f["hist"] = s2.drive_reference(f["curve"], f["pre"], f["dry"], f["wet"], x[b], f["hist"])
        return want


def _set(a, model, bus, curve, pre, dry, wet):
    a.set_bus_drive(bus, curve, pre, dry, wet)
    got = a.get_bus_drive(bus)
    assert np.array_equal(bits(got[0]), bits(np.asarray(curve, dtype=F)))
    assert np.array_equal(bits(np.array(got[1:], dtype=F)), bits(np.array((pre, dry, wet), dtype=F)))
    model.set(bus, curve, pre, dry, wet)
    assert not a.bus_drive_history(bus).any() and a.bus_drive_history(bus).shape == (H, 2)


def _set_named(a, model, bus, name):
    c, m = name.split(":")
    _set(a, model, bus, _curve(c), 1.0, *MIX[m])


def _check(x, want, got, model, what):
    assert np.isfinite(x).all()
    assert_bits_equal_finite(got, want, what)
    for bus in range(x.shape[0]):
        if bus in model.d:
            if not np.array_equal(ubits(want[bus]), ubits(x[bus])):
                assert not np.array_equal(ubits(got[bus]), ubits(x[bus])), "%s: the drive on bus %d changes no bit" % (what, bus)
        else:
            assert_bits_equal_finite(got[bus], x[bus], "%s: bus %d, which carries no drive" % (what, bus))


def _fill(a, b, model, n, nb, what, tune=True):
    """one call on both handles: the buses with a drive against the model over the twin's, the others against the twin's"""
    x = b.sample_buses(n, SR, nb)
    if tune:
        model.tune(a, x, what)
    want = model.expect(x)
    got = a.sample_buses(n, SR, nb)
    _check(x, want, got, model, what)
    assert any(not np.array_equal(ubits(want[bus]), ubits(x[bus])) for bus in model.d if bus < nb), "%s: the model changes nothing" % what
    return x, got


def _histories(a, model, what):
    for bus, f in model.d.items():
        assert_bits_equal_finite(a.bus_drive_history(bus), f["hist"], "%s: history of bus %d" % (what, bus))


def test_the_tile_is_the_kernels():
    assert _tile() == T and T > 2 * H


@pytest.mark.parametrize("n_buses,drives", MATRIX)
def test_drives_are_the_rule_over_the_twins_buses(n_buses, drives):
    """the parity matrix: calls of max_frames, then 1, 2, 15, 16, 17, 31, 32, 33, T - 1, T, T + 1, 2T + 5 frames and max_frames again
    on one pair of handles, every curve kind and a random asymmetric table among the rows; the history is read back at the end and
    once in the middle.  Everything the device returns is collected first, then compared."""
    a, b = _handles()
    model = DriveModel()
    for bus, name in enumerate(drives):
        if name is not None:
            _set_named(a, model, bus, name)
    steps = []
    for fill, n in enumerate(FRAMES):
        _events((a, b), V, fill)
        what = "%d buses, %s, fill %d of %d frames" % (n_buses, drives, fill, n)
        x = b.sample_buses(n, SR, n_buses)
        model.tune(a, x, what)
        want = model.expect(x)
        got = a.sample_buses(n, SR, n_buses)
        st = {bus: (a.bus_drive_history(bus), f["hist"].copy()) for bus, f in model.d.items()} if fill in (4, len(FRAMES) - 1) else {}
        steps.append((what, x, want, got, st))
    for what, x, want, got, st in steps:
        _check(x, want, got, model, what)
        for bus, (g, w) in st.items():
            assert_bits_equal_finite(g, w, "%s: history of bus %d" % (what, bus))


def test_a_crafted_history_is_read_from_the_first_frame():
    """a history with nothing regular about it goes in, comes back, and the first call of one frame reads all 32 frames of it"""
    a, b = _handles()
    model = DriveModel()
    _set(a, model, 1, random_table(), 1.0, 0.25, 1.0)
    _events((a, b), V, 0)
    _fill(a, b, model, 300, 2, "before the history is crafted")
    hist = (np.random.default_rng(3).standard_normal((H, 2)) * 0.25).astype(F)
    a.set_bus_drive_history(1, hist)
    model.d[1]["hist"] = hist.copy()
    assert_bits_equal_finite(a.bus_drive_history(1), hist, "the history set and read back")
    for fill, n in enumerate([1, 2, 17, T + 1], start=1):
        _events((a, b), V, fill)
        _fill(a, b, model, n, 2, "from a crafted history, fill %d" % fill)
        _histories(a, model, "from a crafted history, fill %d" % fill)


def test_a_run_of_short_calls_is_one_long_call():
    """no model in the loop: four handles, two with the same drives; one of each kind renders the same frames in a run of calls, the
    other in one call.  The mixdown itself is one stream only where calls are cut at multiples of 16 — asserted on the handles
    without drives —, and the cuts here are such: the limit is the mixdown's, not this stage's"""
    a, b, c, d = _handles() + _handles()
    for syn in (a, c):
        syn.set_bus_drive(0, _curve("tanh"), 6.0, 0.0, 1.0)
        syn.set_bus_drive(2, random_table(), 3.0, 0.5, 0.5)
    cuts = [16, 48, 16, 32, T, 16, 64, T + 16, 96]
    total = sum(cuts)
    assert total <= 1024 and all(n % 16 == 0 for n in cuts)
    _events((a, b, c, d), V, 0)
    short_drive = np.concatenate([a.sample_buses(n, SR, 3) for n in cuts], axis=1)
    short_dry = np.concatenate([b.sample_buses(n, SR, 3) for n in cuts], axis=1)
    long_drive, long_dry = c.sample_buses(total, SR, 3), d.sample_buses(total, SR, 3)
    assert_bits_equal_finite(short_dry, long_dry, "without drives: the mixdown in short calls and in one")
    assert_bits_equal_finite(short_drive, long_drive, "with the drives: short calls and one long call")
    assert_bits_equal_finite(short_drive[1], long_dry[1], "the bus without a drive")
    for bus in (0, 2):
        assert not np.array_equal(ubits(long_drive[bus]), ubits(long_dry[bus]))
        assert_bits_equal_finite(a.bus_drive_history(bus), c.bus_drive_history(bus), "the history of bus %d after both" % bus)
        assert_bits_equal_finite(a.bus_drive_history(bus), long_dry[bus][-H:], "the history is the bus's last 32 frames")


@pytest.mark.parametrize("frames", [250, 64])
def test_events_inside_a_fill_and_sliced_rows(frames, monkeypatch):
    """note_ons at frames 16 and 48 split the call into segments and a rows buffer of 48 frames slices them further: the stage sees the
    call as one stream"""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    a, b = _handles(max_frames=256)
    model = DriveModel()
    _set(a, model, 0, _curve("cubic"), 1.0, 0.0, 1.0)
    _set(a, model, 3, random_table(), 1.0, 0.5, 0.5)
    for fill in range(3):
        _events((a, b), V, fill)
        _timed((a, b), fill)
        _fill(a, b, model, frames, 4, "events at 16 and 48, slices of 48, %d frames, fill %d" % (frames, fill))
    _histories(a, model, "events and slices")
    a.L.s2r_debug_pan_slice.restype = C.c_uint32
    a.L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    assert a.L.s2r_debug_pan_slice(a.h) == 48


def test_a_send_only_bus_with_a_drive_while_a_fader_ramps():
    """bus 6 of eight sounds through program 0's send alone and carries a drive; program 0's fader moves across the second and third
    call — on both handles, so the twin's bus 6 enters the stage under the same sends and ramps"""
    a, b = _handles()
    model = DriveModel()
    _set(a, model, 6, _curve("fold"), 1.0, 0.25, 1.0)
    walk = [(1.0, 0.0), (0.25, 1.0), (0.7, -0.5), (0.7, -0.5)]
    for fill, n in enumerate([300, 1000, 17, 64]):
        _events((a, b), V, fill)
        for syn in (a, b):
            syn.set_program_fader(0, *walk[fill])
        _fill(a, b, model, n, 8, "send-only bus under a fader ramp, fill %d" % fill)
        f = a.get_program_fader(0)
        assert f == b.get_program_fader(0) and f[:2] == f[2:]    # committed on both
    _histories(a, model, "under the ramps")


def test_the_drive_behind_an_eq_and_dynamics_and_in_front_of_the_rest_of_the_bus():
    """one bus with everything: the drive reads what the dynamics wrote, and the chorus, the delay, the reverb and the room what the
    drive wrote"""
    a, b = _handles()
    eq, dy, dr, ch, dl, rv, rm = EqModel(), DynModel(), DriveModel(), ChorusModel(), DelayModel(), Model(), RoomModel()
    c = _coeffs(2, 1)
    a.set_bus_eq(1, c); eq.set(1, c)
    curve = s2.dynamics_curve(-30.0, 4.0, 6.0, 3.0)
    a.set_bus_dynamics(1, 0, curve, 0.9, 0.999); dy.set(1, 0, curve, 0.9, 0.999)
    _set(a, dr, 1, _curve("tanh"), 1.0, 0.25, 1.0)
    _set(a, dr, 0, random_table(), 1.0, 0.0, 1.0)
    args = (2,) + SHAPES[3] + (1 << 22, 5, 0.75, 0.5)
    a.set_bus_chorus(1, *args); ch.set(1, *args)
    a.set_bus_delay(1, 200, 0.5, -0.5, 0.5, 1.0); dl.set(1, 200, 0.5, -0.5, 0.5, 1.0)
    ir = _ir(40, 77, True)
    a.set_bus_reverb(1, ir, 0.25, 1.0); rv.set(1, ir, 0.25, 1.0)
    a.set_bus_room(1, *SMALL, *ROOM_LEVELS["hall"]); rm.set(1, SMALL, ROOM_LEVELS["hall"])
    for fill, n in enumerate([300, 1, T + 1, 1024]):
        _events((a, b), V, fill)
        what = "the whole chain on one bus, fill %d" % fill
        y = dy.expect(eq.expect(b.sample_buses(n, SR, 3)))
        dr.tune(a, y, what)
        z = dr.expect(y)
        assert not np.array_equal(ubits(z[1]), ubits(y[1])) and np.array_equal(ubits(z[2]), ubits(y[2]))
        assert_bits_equal_finite(a.sample_buses(n, SR, 3), rm.expect(rv.expect(dl.expect(ch.expect(z)))), what)
    _histories(a, dr, "in the whole chain")


def test_every_route_with_the_eq_the_dynamics_the_drive_and_the_room_on():
    """Handle `a` walks all 24 rows of s2r_post_route's table with EQs, dynamics, drives and rooms on, 32 frames a call — a bus fill, a
    master fill and a master fill under the limiter, each with every subset of chorus, delay and reverb, master fills with and without
    stems —; its twin `b` makes a plain bus fill of the same frames every time.  Every step's expectation is the chain of the models:
    EQ, dynamics, drive, chorus, delay, reverb, room, master section, limiter.  Everything the device returns is collected first, then
    compared."""
    a, b = _handles()
    eq, dy, dr, ch, dl, rv, rm, mm = EqModel(), DynModel(), DriveModel(), ChorusModel(), DelayModel(), Model(), RoomModel(), Master()
    for bus, nb in enumerate((2, 4, 1)):
        c = _coeffs(nb, bus + 1)
        a.set_bus_eq(bus, c)
        eq.set(bus, c)
    curve = s2.dynamics_curve(-30.0, 4.0, 6.0, 3.0)
    for bus, key in enumerate((0, 0, 2)):
        a.set_bus_dynamics(bus, key, curve, 0.9, 0.999)
        dy.set(bus, key, curve, 0.9, 0.999)
    _set(a, dr, 0, _curve("hard"), 1.0, 0.0, 1.0)
    _set(a, dr, 2, random_table(), 1.0, 0.5, 0.75)                # (bus 1 carries none: the drive's launch copies it)
    for bus, (d, lv) in ((0, (FLAT, "hall")), (1, (SMALL, "dark"))):
        a.set_bus_room(bus, *d, *ROOM_LEVELS[lv])
        rm.set(bus, d, ROOM_LEVELS[lv])
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

    def chain(n, what, nb=3):
        y = dy.expect(eq.expect(b.sample_buses(n, SR, nb)))
        dr.tune(a, y, what)
        z = dr.expect(y)
        assert all(not np.array_equal(ubits(z[q]), ubits(y[q])) for q in (0, 2)) and np.array_equal(ubits(z[1]), ubits(y[1]))
        return rm.expect(rv.expect(dl.expect(ch.expect(z))))

    def bus_fill(what, n):
        y = chain(n, what)
        steps.append((what, {"buses": (a.sample_buses(n, SR, 3), y)}))

    def master_fill(what, n, stems):
        y = chain(n, what)
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
            what = "%d: %s, EQ, dynamics, drive and room on, chorus %s, delay %s, reverb %s" % ((k + 1, kind) + tuple("on" if o else "off" for o in on))
            if kind == "bus fill":
                bus_fill(what, 32)
            else:
                master_fill(what, 32, stems=j % 2 == 0)
            k += 1
    assert k == 24 and len(lims) == 1 and lims[0].limited() > 0.0       # on the model, before anything is compared: the walk limits
    for what, cmp in steps:
        for name, (got, want) in cmp.items():
            assert_bits_equal_finite(got, want, "%s: %s" % (what, name))
    mm.check_committed(a)
    _histories(a, dr, "after the walk")


def test_a_master_fill_applies_the_drive():
    """stems and master of s2r_fill_master against the models: the drive, then the master section, and then the limiter"""
    a, b = _handles()
    model, mm = DriveModel(), Master()
    _set(a, model, 0, _curve("tanh"), 1.0, 0.0, 1.0)
    _set(a, model, 2, random_table(), 1.0, 0.5, 0.5)
    lim = None
    for fill, n in enumerate([T + 1, 1, 300, 64, 33]):
        _events((a, b), V, fill)
        x = b.sample_buses(n, SR, 3)
        model.tune(a, x, "master fill %d" % fill)
        y = model.expect(x)
        m = mm.expect(y)
        if fill == 3:
            ceiling = float(np.abs(m).max()) / 2.0               # half this master's peak: the limiter works
            lim = Lim(48, 0, ceiling)
            lim.set((a,), ceiling)
        got, st = a.sample_master(n, SR, 3, stems=True)
        assert_bits_equal_finite(st, y, "the stems of a master fill, fill %d" % fill)
        assert_bits_equal_finite(got, lim.expect(m)[0] if lim else m, "the master, fill %d" % fill)
        _histories(a, model, "master fill %d" % fill)


def test_a_drive_past_the_calls_buses_is_idle():
    """a drive on bus 5: in calls of three buses its crafted history stays; bus 0 beside it runs; a call of eight buses goes on from it"""
    a, b = _handles()
    model = DriveModel()
    _set(a, model, 0, _curve("cubic"), 1.0, 0.0, 1.0)
    _set(a, model, 5, random_table(), 1.0, 0.5, 0.5)
    hist = (np.random.default_rng(4).standard_normal((H, 2)) * 0.25).astype(F)
    a.set_bus_drive_history(5, hist)
    model.d[5]["hist"] = hist.copy()
    for fill, n in enumerate([300, 2, T + 1]):
        _events((a, b), V, fill)
        _fill(a, b, model, n, 3, "a drive past the call's buses, fill %d" % fill)
    assert_bits_equal_finite(a.bus_drive_history(5), hist, "the idle drive's history")
    _events((a, b), V, 3)
    _fill(a, b, model, 100, 8, "eight buses: the idle drive wakes from its crafted history")
    _histories(a, model, "after the call of eight buses")
    assert not np.array_equal(bits(a.bus_drive_history(5)), bits(hist))


def test_new_parameters_in_mid_stream_keep_the_history_and_a_set_zeroes_it():
    a, b = _handles()
    model = DriveModel()
    _set(a, model, 1, _curve("tanh"), 1.0, 0.0, 1.0)
    _events((a, b), V, 0)
    _fill(a, b, model, 300, 2, "before the parameters move")
    hist = a.bus_drive_history(1)
    assert hist.any()
    a.set_bus_drive_params(1, None, 2.0, 0.5, 0.25)              # the levels alone: the table stays
    model.d[1].update(pre=F(2.0), dry=F(0.5), wet=F(0.25))
    got = a.get_bus_drive(1)
    assert np.array_equal(bits(got[0]), bits(_curve("tanh"))) and got[1:] == (2.0, 0.5, 0.25)
    assert_bits_equal_finite(a.bus_drive_history(1), hist, "the history under new levels")
    _events((a, b), V, 1)
    _fill(a, b, model, 300, 2, "after s2r_set_bus_drive_params without a table")
    new = random_table(9)
    a.set_bus_drive_params(1, new, 2.0, 0.5, 0.25)               # and with one
    model.d[1]["curve"] = new.copy()
    assert np.array_equal(bits(a.get_bus_drive(1)[0]), bits(new))
    _events((a, b), V, 2)
    _fill(a, b, model, 33, 2, "after s2r_set_bus_drive_params with a table")
    _histories(a, model, "after the parameters moved")
    _set(a, model, 1, new, 1.0, 0.0, 1.0)                        # setting it again zeroes the history
    _events((a, b), V, 3)
    _fill(a, b, model, 64, 2, "after s2r_set_bus_drive")
    _histories(a, model, "from silence")
    with pytest.raises(s2.S2rError) as err:
        a.set_bus_drive_params(0, None, 1.0, 0.0, 1.0)
    assert err.value.status == s2s.S2R_ERR_INVALID


def test_checkpoint_onto_a_fresh_handle():
    """state, pans, mix, sends, the drive's table, levels and history go into a fresh handle: the next fills are equal"""
    a, b = _handles(max_frames=512)
    model = DriveModel()
    _set(a, model, 0, _curve("fold"), 1.0, 0.25, 1.0)
    _set(a, model, 1, random_table(), 1.0, 0.0, 1.0)
    for fill, n in enumerate([400, 200]):
        _events((a, b), V, fill)
        _fill(a, b, model, n, 2, "before the checkpoint, fill %d" % fill)
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    c = s2.Synth(V, max_frames=512, block_voices=64)
    c.set_patch_bank(_bank())
    c.import_state(state)
    c.set_voice_pans(pans)
    c.set_voice_mix(gains, buses)
    c.set_voice_sends(sends, sbuses)
    for bus in (0, 1):
        c.set_bus_drive(bus, *a.get_bus_drive(bus))
        c.set_bus_drive_history(bus, a.bus_drive_history(bus))
    for k, n in enumerate([100, 400]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        _, got = _fill(a, b, model, n, 2, "the checkpointed handle, fill %d" % k, tune=False)
        assert_bits_equal_finite(c.sample_buses(n, SR, 2), got, "the resumed handle, fill %d" % k)
    for bus in (0, 1):
        assert_bits_equal_finite(c.bus_drive_history(bus), a.bus_drive_history(bus), "history of bus %d" % bus)
    # the drive is the bus's: a new bank, a program change and an imported state leave it and its history alone
    keep = a.bus_drive_history(1)
    a.set_patch_bank(_bank())
    a.program_change(3)
    a.import_state(state)
    assert a.get_bus_drive(1) is not None and np.array_equal(bits(a.bus_drive_history(1)), bits(keep))


def test_subnormal_samples_through_the_table():
    """pre = 2^-130: t is subnormal on every frame that sounds, the linear table hands it through, and with dry 0 and wet 1 the output is
    subnormal: a device that flushed them would write zeros"""
    a, b = _handles()
    model = DriveModel()
    pre = F(2.0) ** F(-130)
    assert 0.0 < float(pre) < np.finfo(F).tiny
    _set(a, model, 0, _curve("linear"), pre, 0.0, 1.0)
    for fill, n in enumerate([300, 17]):
        _events((a, b), V, fill)
        x = b.sample_buses(n, SR, 1)
        t = pre * oversampled(x[0], model.d[0]["hist"])
        assert ((t != 0.0) & (np.abs(t) < np.finfo(F).tiny)).mean() > 0.5
        want = model.expect(x)
        assert ((want != 0.0) & (np.abs(want) < np.finfo(F).tiny)).mean() > 0.5
        assert_bits_equal_finite(a.sample_buses(n, SR, 1), want, "subnormal t, fill %d" % fill)


def test_refusals_removal_and_the_other_fills():
    """a fill refused before any launch leaves the history untouched, in a bus fill and in a master fill; the panned, mono and stereo
    fills ignore the drive; the history pair's count, capacity and finiteness checks; after a removal the bus is the twin's on bits
    again; a device-list handle refuses every entry and renders on"""
    a, b = _handles(max_frames=256)
    model = DriveModel()
    _set(a, model, 0, _curve("tanh"), 1.0, 0.0, 1.0)
    _events((a, b), V, 0)
    _fill(a, b, model, 100, 2, "before the refusals")
    before = a.bus_drive_history(0)
    L, h = a.L, a.h
    out, lr = np.empty(2 * 2 * 300, dtype=F), np.empty(2 * 300, dtype=F)
    p, q = out.ctypes.data_as(s2s._f32p), lr.ctypes.data_as(s2s._f32p)
    assert L.s2r_fill_buses(h, p, 2 * 2 * 100 - 1, 2, 100, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_buses(h, p, out.size, 9, 16, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_buses(h, p, out.size, 2, 257, SR) == s2s.S2R_ERR_TOO_MANY_FRAMES
    assert L.s2r_fill_master(h, q, p, 2 * 2 * 100 - 1, 2, 100, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_master(h, q, p, out.size, 2, 257, SR) == s2s.S2R_ERR_TOO_MANY_FRAMES
    assert_bits_equal_finite(a.bus_drive_history(0), before, "the history after refused fills")
    # the history pair
    n = 2 * H
    buf = np.zeros(n + 1, dtype=F)
    bp = buf.ctypes.data_as(s2s._f32p)
    assert L.s2r_get_bus_drive_history(h, 0, bp, n - 1) == s2s.S2R_ERR_INVALID and L.s2r_get_bus_drive_history(h, 0, None, n) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_drive_history(h, 0, bp, n + 1) == s2s.S2R_OK and np.array_equal(bits(buf[:n]), bits(before.ravel())) and buf[n] == 0.0
    assert L.s2r_set_bus_drive_history(h, 0, bp, n - 1) == s2s.S2R_ERR_INVALID and L.s2r_set_bus_drive_history(h, 0, bp, n + 1) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_drive_history(h, 0, None, n) == s2s.S2R_ERR_INVALID and L.s2r_get_bus_drive_history(h, 1, bp, n) == s2s.S2R_ERR_INVALID
    for v in (np.nan, np.inf, -np.inf):
        bad = before.copy().ravel()
        bad[n // 2] = v
        assert L.s2r_set_bus_drive_history(h, 0, bad.ctypes.data_as(s2s._f32p), n) == s2s.S2R_ERR_PATCH_RANGE
    small = np.zeros(8, dtype=F)
    assert L.s2r_get_bus_drive(h, 0, None, small.ctypes.data_as(s2s._f32p), 8, None, None, None) == s2s.S2R_ERR_INVALID and not small.any()
    assert_bits_equal_finite(a.bus_drive_history(0), before, "the history after refused restores")
    # the other fills
    assert_bits_equal_finite(a.sample_panned(100, SR), b.sample_panned(100, SR), "panned fill beside a drive")
    assert_bits_equal_finite(a.sample(np.empty(64, dtype=F), SR), b.sample(np.empty(64, dtype=F), SR), "mono fill beside a drive")
    assert_bits_equal_finite(a.sample_stereo(33, SR), b.sample_stereo(33, SR), "stereo copy beside a drive")
    assert_bits_equal_finite(a.bus_drive_history(0), before, "the history after the other fills")
    _events((a, b), V, 1)
    _fill(a, b, model, 64, 2, "after the refusals and the other fills")
    # removal
    a.clear_bus_drive(0)
    del model.d[0]
    assert a.get_bus_drive(0) is None
    _events((a, b), V, 2)
    x = b.sample_buses(64, SR, 2)
    assert_bits_equal_finite(a.sample_buses(64, SR, 2), x, "no drive left: the twin's")
    # a device list
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    one = s2.Synth(512, max_frames=64, mix_groups=2)
    for syn in (multi, one):
        for v in range(512):
            syn.note_on(36 + v % 61)
    lin = s2.drive_curve(s2.DRIVE_LINEAR)
    lp, k = lin.ctypes.data_as(s2s._f32p), C.c_uint32()
    lv = (1.0, 0.5, 0.5)
    assert multi.L.s2r_set_bus_drive(multi.h, 0, lp, *lv) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_clear_bus_drive(multi.h, 0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_drive_params(multi.h, 0, None, *lv) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_drive(multi.h, 0, C.byref(k), None, 0, None, None, None) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_drive_history(multi.h, 0, bp, n) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_drive_history(multi.h, 0, bp, n) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        multi.set_bus_drive(0, lin, *lv)
    assert err.value.status == s2s.S2R_ERR_INVALID
    x, y = multi.sample(np.empty(64, dtype=F), SR), one.sample(np.empty(64, dtype=F), SR)
    assert np.abs(y).max() > 0.0
    assert_bits_equal_finite(x, y, "the device-list handle after the refused drive calls")


def test_range_checks_on_a_handle():
    check_ranges(s2.Synth(8, max_frames=64))


def test_a_handle_that_never_had_a_drive_and_the_timing_entry():
    """s2r_debug_bus_drive_ms: -1 without s2r_set_timing; under it 0 after a bus fill and a master fill of a handle that never had a
    drive, whose outputs are the twin's and which holds nothing for one; and the kernel's time once a drive is set"""
    a, b = _handles()
    ms, alloc = a.L.s2r_debug_bus_drive_ms, a.L.s2r_debug_drive_allocated
    ms.restype, ms.argtypes = C.c_float, [C.c_void_p]
    alloc.restype, alloc.argtypes = C.c_int, [C.c_void_p]
    _events((a, b), V, 0)
    assert_bits_equal_finite(a.sample_buses(300, SR, 3), b.sample_buses(300, SR, 3), "no drive, timing off")
    assert ms(a.h) == -1.0
    a.set_timing(True)
    _events((a, b), V, 1)
    assert_bits_equal_finite(a.sample_buses(300, SR, 3), b.sample_buses(300, SR, 3), "no drive, bus fill under timing")
    assert ms(a.h) == 0.0
    _events((a, b), V, 2)
    (ma, sa), (mb, sb) = a.sample_master(300, SR, 3), b.sample_master(300, SR, 3)
    assert_bits_equal_finite(ma, mb, "no drive, master fill under timing")
    assert_bits_equal_finite(sa, sb, "no drive, the stems of a master fill")
    assert ms(a.h) == 0.0 and alloc(a.h) == 0
    a.set_bus_drive(4, _curve("tanh"), 4.0, 0.0, 1.0)
    assert alloc(a.h) == 1
    a.sample_buses(300, SR, 5)
    assert 0.0 < ms(a.h) < 100.0
    a.sample_buses(300, SR, 3)                                   # the drive is past the call's buses: idle, no kernel
    assert ms(a.h) == 0.0
