"""The per-bus flanger on the device.  Twin handles on pools of 32 voices are fed the same events, one with flangers and
one without; the twin's bus output is what enters the chain, and the expectation is the rule on the host (s2.flanger_reference, which
tests/test_flanger_host.py holds to a numpy float32 model on bits) with line and phase carried from call to call (FlangerModel), behind
the models of the stages in front of it.

The kernel walks a call in tiles of T = 32 frames (s2r_debug_flanger_tile), which is also the youngest frame a tap may read: the shapes
are H = 33 with no depth — every tap exactly one tile old, the smallest shape at which a tile that reads too early shows —, 34, 64, 65,
145, 1024 and 4096, the window the kernel keeps in LDS; the call lengths are 1, 2, 31, 32, 33, 63, 64, 65, 2 * 32 + 5 and 1024 =
max_frames, most of them shorter than H.  Before the device runs, the model must show that the recursion is not idle: over a bus's whole
call sequence its output differs on bits from the same model at feedback = cross = 0 in at least a tenth of the frames (FlangerModel.busy).
Handles, events and the one-pole bank are tests/test_gpu_reverb.py's.  Every comparison is on bits with no NaN allowance
(helpers.assert_bits_equal_finite) but the two that say why they are not."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_flanger_host import MIXES, bits, check_ranges, history_frames
from test_drive_host import random_table
from test_room_host import FLAT, SMALL
from test_gpu_buses import ubits
from test_gpu_chorus import SHAPES as CHORUS_SHAPES, ChorusModel
from test_gpu_delay import DelayModel
from test_gpu_drive import DriveModel
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
T = 32                                                           # S2R_FLANGER_TILE (csrc/s2r_device.h); test_the_tile_is_the_kernels holds it to the library
# (base, depth) by H = floor(fl(base + depth)) + 1
SHAPE = {33: (32.0, 0.0), 34: (32.75, 1.0), 64: (40.0, 23.5), 65: (40.0, 24.5), 145: (48.0, 96.5), 1024: (100.0, 923.5), 4096: (32.0, 4063.0)}
FRAMES = [1024, 1, 2, 31, 32, 33, 63, 64, 65, 2 * T + 5, 1024]
LONG = FRAMES + [1024] * 6                                       # for the rows with H >= 1024: the line turns over, and the recursion shows
INC, SPREAD = 89478 * 4, 0x40000000                              # 4 Hz at 48 kHz: a sweep of 12 000 frames; the right channel a quarter turn ahead
NONE, FB, NEG, CROSS, FULL = MIXES                               # (0, 0), (0.7, 0), (-0.7, 0.3), (0, 1), (1, 0)
# (n_buses, {bus: (H, (feedback, cross), (dry, wet))}): flangers around a bus without one, and one past the call's buses, which is idle
MATRIX = [(1, {0: (33, FB, (0.0, 1.0))}),
          (2, {0: (34, NEG, (0.5, 0.75)), 5: (145, FULL, (0.0, 1.0))}),
          (3, {0: (64, CROSS, (0.0, 1.0)), 2: (65, FULL, (0.5, 0.5))}),
          (8, {0: (145, FB, (0.5, 0.75)), 1: (1024, NEG, (0.0, 1.0)), 3: (4096, CROSS, (0.25, 1.0)), 4: (33, NONE, (0.5, 0.5)), 6: (65, FULL, (0.0, 1.0)),
               7: (4096, NEG, (0.5, 0.75))})]
for _h, _s in SHAPE.items():
    assert history_frames(*_s) == _h


def _handles(max_frames=1024):
    return _reverb_handles(voices=V, max_frames=max_frames)


def _tile():
    L = s2.load_library()
    L.s2r_debug_flanger_tile.restype, L.s2r_debug_flanger_tile.argtypes = C.c_uint32, []
    return int(L.s2r_debug_flanger_tile())


class FlangerModel:
    """the flangers of a handle on the host: per bus the parameters and the carried line and phase — and beside each the same flanger
    at feedback = cross = 0, fed the same input, which says how much of the output the recursion makes"""

    def __init__(self):
        self.f = {}

    def set(self, bus, base, depth, inc, spread, fb, cross, dry, wet):
        H = history_frames(base, depth)
        self.f[bus] = dict(shape=(base, depth), inc=inc, spread=spread, mix=(fb, cross, dry, wet), hist=np.zeros((H, 2), dtype=F), phase=0,
                           open_hist=np.zeros((H, 2), dtype=F), differs=0, frames=0)

    def expect(self, x):
        """what the stage makes of a call whose buses enter it as x [n_buses, N, 2]; lines and phases of its buses move on"""
        want = x.copy()
        for b, f in self.f.items():
            if b >= x.shape[0]:
                continue                                         # idle in this call
            ph = f["phase"]
            want[b], f["hist"], f["phase"] = s2.flanger_reference(*f["shape"], f["inc"], f["spread"], *f["mix"], x[b], f["hist"], ph)
            opened, f["open_hist"], _ = s2.flanger_reference(*f["shape"], f["inc"], f["spread"], 0.0, 0.0, *f["mix"][2:], x[b], f["open_hist"], ph)
            f["differs"] += int((ubits(want[b]) != ubits(opened)).any(axis=-1).sum())
            f["frames"] += x.shape[1]
        return want

    def busy(self, what):
        """the condition on the inputs: the recursion made at least a tenth of every bus's frames"""
        for b, f in self.f.items():
            if f["frames"] and f["mix"][:2] != (0.0, 0.0):
                assert f["differs"] >= f["frames"] / 10.0, "%s: bus %d: the recursion shows in %d of %d frames" % (what, b, f["differs"], f["frames"])


def _set(a, model, bus, H, mix, level, inc=INC, spread=SPREAD):
    args = SHAPE[H] + (inc, spread) + tuple(mix) + tuple(level)
    a.set_bus_flanger(bus, *args)
    assert a.get_bus_flanger(bus) == tuple(F(v) if isinstance(v, float) else v for v in args)
    model.set(bus, *args)
    hist, phase = a.bus_flanger_state(bus)
    assert hist.shape == (H, 2) and not bits(hist).any() and phase == 0


def _check(x, want, got, model, what):
    assert np.isfinite(x).all()
    assert_bits_equal_finite(got, want, what)
    for bus in range(x.shape[0]):
        if bus not in model.f:
            assert_bits_equal_finite(got[bus], x[bus], "%s: bus %d, which carries no flanger" % (what, bus))


def _fill(a, b, model, n, nb, what):
    """one call on both handles: the buses with a flanger against the model over the twin's, the others against the twin's"""
    x = b.sample_buses(n, SR, nb)
    want = model.expect(x)
    got = a.sample_buses(n, SR, nb)
    _check(x, want, got, model, what)
    return x, got


def _states(a, model, what):
    for bus, f in model.f.items():
        hist, phase = a.bus_flanger_state(bus)
        assert_bits_equal_finite(hist, f["hist"], "%s: line of bus %d" % (what, bus))
        assert phase == f["phase"], "%s: phase of bus %d" % (what, bus)


def test_the_tile_is_the_kernels():
    assert _tile() == T == int(s2.FLANGER_MIN_DELAY)


@pytest.mark.parametrize("n_buses,flangers", MATRIX)
def test_flangers_are_the_rule_over_the_twins_buses(n_buses, flangers):
    """the parity matrix: every H and every (feedback, cross) of the host test among the rows, calls of max_frames, then 1, 2, 31, 32,
    33, 63, 64, 65, 69 frames and max_frames again on one pair of handles (and six more of max_frames where a line is 1024 frames or
    longer); line and phase are read back at the end and once in the middle.  The twin's buses and the model come first, then the
    condition on them, then the device; everything it returns is collected first, then compared."""
    a, b = _handles()
    model = FlangerModel()
    for bus, (H, mix, level) in flangers.items():
        _set(a, model, bus, H, mix, level)
    frames = LONG if any(H >= 1024 for H, _, _ in flangers.values()) else FRAMES
    assert any(n < H for H, _, _ in flangers.values() for n in frames)       # calls shorter than a line
    steps = []
    for fill, n in enumerate(frames):
        _events((a, b), V, fill)
        what = "%d buses, fill %d of %d frames" % (n_buses, fill, n)
        x = b.sample_buses(n, SR, n_buses)
        want = model.expect(x)
        got = a.sample_buses(n, SR, n_buses)
        st = {bus: (a.bus_flanger_state(bus), (f["hist"].copy(), f["phase"])) for bus, f in model.f.items()} if fill in (4, len(frames) - 1) else {}
        steps.append((what, x, want, got, st))
    model.busy("%d buses" % n_buses)
    for what, x, want, got, st in steps:
        _check(x, want, got, model, what)
        for bus, (g, w) in st.items():
            assert_bits_equal_finite(g[0], w[0], "%s: line of bus %d" % (what, bus))
            assert g[1] == w[1], "%s: phase of bus %d" % (what, bus)
    for bus, f in model.f.items():
        if bus >= n_buses:                                       # the idle one: state untouched
            assert not f["frames"] and not bits(f["hist"]).any()


GROUP = 8 * T                                                    # kFlAhead tiles: the frames whose input the wave loads ahead, a group at a time
EDGES = [2048, GROUP - 1, GROUP, GROUP + 1, GROUP + T - 1, GROUP + T, GROUP + T + 1, 2 * GROUP - 1, 2 * GROUP, 2 * GROUP + 1, 1025, 2047, 2048]
EDGE_FLANGERS = {0: (33, FB, (0.0, 1.0)), 1: (145, NEG, (0.5, 0.75)), 2: (4096, CROSS, (0.25, 1.0))}


@pytest.mark.parametrize("n_buses", [4, 3])
def test_the_group_edges_and_calls_past_1024_frames(n_buses):
    """The wave walks groups of eight whole tiles, 256 frames, loading the next group's input first, clamped to the call's last frame,
    then a tail of fewer than eight whole tiles and a partial one: calls of 255, 256, 257, 287, 288, 289, 511, 512 and 513 frames are a
    group that ends the call (every load of the next group clamped), one frame less and more, a group and one whole tile, and the
    same around two groups.  Calls of 1025, 2047 and 2048 frames on handles of max_frames = 2048 are past the staging buffer's first
    1024 frames of a bus, and N + H walks the ring of 4096 once and a half at H = 4096.  With four buses the fourth carries no
    flanger and is copied by workgroups (1 + g, 3) of 1024 frames each, two of them; with three every bus of the call carries one,
    the grid is (1, 3) and no copy workgroup exists.  Line and phase are read back after the call of 256 frames and at the end.  The
    twin's buses and the model come first, then the condition on them, then the device; everything it returns is collected first,
    then compared."""
    assert EDGES == [2048, 255, 256, 257, 287, 288, 289, 511, 512, 513, 1025, 2047, 2048]
    a, b = _handles(max_frames=2048)
    model = FlangerModel()
    for bus, (H, mix, level) in EDGE_FLANGERS.items():
        _set(a, model, bus, H, mix, level)
    assert (n_buses - len(model.f)) == (1 if n_buses == 4 else 0)
    steps = []
    for fill, n in enumerate(EDGES):
        _events((a, b), V, fill)
        what = "%d buses, fill %d of %d frames" % (n_buses, fill, n)
        x = b.sample_buses(n, SR, n_buses)
        want = model.expect(x)
        got = a.sample_buses(n, SR, n_buses)
        st = {bus: (a.bus_flanger_state(bus), (f["hist"].copy(), f["phase"])) for bus, f in model.f.items()} if fill in (2, len(EDGES) - 1) else {}
        steps.append((what, x, want, got, st))
    model.busy("%d buses, the group edges" % n_buses)
    assert sum(1 for _, _, _, _, st in steps if st) == 2 and steps[2][1].shape[1] == GROUP
    for what, x, want, got, st in steps:
        _check(x, want, got, model, what)
        for bus, (g, w) in st.items():
            assert_bits_equal_finite(g[0], w[0], "%s: line of bus %d" % (what, bus))
            assert g[1] == w[1], "%s: phase of bus %d" % (what, bus)


def test_a_crafted_history_at_the_shortest_delay():
    """base 32, depth 0, feedback 1, wet alone: tap[n] = w[n - 32], every tap exactly one tile old.  The line goes in as a ramp of
    distinct values, comes back, and the first tile returns 32 of its 33 frames in order; a tile that read its own frames, or the
    wrong end of the line, would show"""
    a, b = _handles()
    model = FlangerModel()
    _set(a, model, 1, 33, FULL, (0.0, 1.0))
    hist = (np.arange(66, dtype=F).reshape(33, 2) + F(1.0)) * F(2.0 ** -8)
    a.set_bus_flanger_state(1, hist, 0x12345678)
    model.f[1].update(hist=hist.copy(), open_hist=hist.copy(), phase=0x12345678)
    got, phase = a.bus_flanger_state(1)
    assert np.array_equal(bits(got), bits(hist)) and phase == 0x12345678
    for fill, n in enumerate([1, 2, 31, 32, 33, 2 * T + 5]):
        _events((a, b), V, fill)
        x, y = _fill(a, b, model, n, 2, "from a crafted line, fill %d" % fill)
        if fill == 0:
            assert np.array_equal(y[1, 0], hist[1])              # w[-32], the second oldest frame of the line
        _states(a, model, "from a crafted line, fill %d" % fill)
    model.busy("from a crafted line")


@pytest.mark.parametrize("frames", [250, 64])
def test_events_inside_a_fill_and_sliced_rows(frames, monkeypatch):
    """note_ons at frames 16 and 48 split the call into segments and a rows buffer of 48 frames slices them further: the stage sees the
    call as one stream"""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    a, b = _handles(max_frames=256)
    model = FlangerModel()
    _set(a, model, 0, 34, NEG, (0.5, 0.75))
    _set(a, model, 3, 145, FB, (0.0, 1.0))
    for fill in range(4):
        _events((a, b), V, fill)
        _timed((a, b), fill)
        _fill(a, b, model, frames, 4, "events at 16 and 48, slices of 48, %d frames, fill %d" % (frames, fill))
    _states(a, model, "events and slices")
    model.busy("events and slices")
    a.L.s2r_debug_pan_slice.restype = C.c_uint32
    a.L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    assert a.L.s2r_debug_pan_slice(a.h) == 48


def test_a_send_only_bus_with_a_flanger_while_a_fader_ramps():
    """bus 6 of eight sounds through program 0's send alone and carries a flanger; program 0's fader moves across the second and third
    call — on both handles, so the twin's bus 6 enters the stage under the same sends and ramps"""
    a, b = _handles()
    model = FlangerModel()
    _set(a, model, 6, 65, NEG, (0.25, 1.0))
    walk = [(1.0, 0.0), (0.25, 1.0), (0.7, -0.5), (0.7, -0.5)]
    for fill, n in enumerate([300, 1000, 17, 64]):
        _events((a, b), V, fill)
        for syn in (a, b):
            syn.set_program_fader(0, *walk[fill])
        x, _ = _fill(a, b, model, n, 8, "send-only bus under a fader ramp, fill %d" % fill)
        assert ubits(x[6]).any()
        f = a.get_program_fader(0)
        assert f == b.get_program_fader(0) and f[:2] == f[2:]    # committed on both
    _states(a, model, "under the ramps")
    model.busy("under the ramps")


def test_every_route_with_the_eq_the_dynamics_the_drive_the_flanger_and_the_room_on():
    """Handle `a` walks all 24 rows of s2r_post_route's table with EQs, dynamics, drives, flangers and rooms on, 32 frames a call — a bus
    fill, a master fill and a master fill under the limiter, each with every subset of chorus, delay and reverb, master fills with and
    without stems —; its twin `b` makes a plain bus fill of the same frames every time.  Every step's expectation is the chain of the
    models: EQ, dynamics, drive, flanger, chorus, delay, reverb, room, master section, limiter.  Everything the device returns is
    collected first, then compared."""
    a, b = _handles()
    eq, dy, dr, fl, ch, dl, rv, rm, mm = EqModel(), DynModel(), DriveModel(), FlangerModel(), ChorusModel(), DelayModel(), Model(), RoomModel(), Master()
    for bus, nb in enumerate((2, 4, 1)):
        c = _coeffs(nb, bus + 1)
        a.set_bus_eq(bus, c)
        eq.set(bus, c)
    curve = s2.dynamics_curve(-30.0, 4.0, 6.0, 3.0)
    for bus, key in enumerate((0, 0, 2)):
        a.set_bus_dynamics(bus, key, curve, 0.9, 0.999)
        dy.set(bus, key, curve, 0.9, 0.999)
    for bus, (table, lv) in ((0, (s2.drive_curve(s2.DRIVE_HARD, 2.0), (0.0, 1.0))), (2, (random_table(), (0.5, 0.75)))):
        a.set_bus_drive(bus, table, 4.0, *lv)
        dr.set(bus, table, 4.0, *lv)
    _set(a, fl, 1, 33, FULL, (0.25, 1.0))                        # (bus 0 carries none: the flanger's launch copies it)
    _set(a, fl, 2, 65, NEG, (0.5, 0.75))
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
                for bus, args in ((2, (3,) + CHORUS_SHAPES[145] + (89478 * 20, 0x40000000, 0.5, 0.25)), (1, (2,) + CHORUS_SHAPES[3] + (1 << 22, 5, 0.75, 0.5))):
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
        y = dr.expect(dy.expect(eq.expect(b.sample_buses(n, SR, nb))))
        z = fl.expect(y)
        assert np.array_equal(ubits(z[0]), ubits(y[0]))
        return rm.expect(rv.expect(dl.expect(ch.expect(z))))

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
            what = "%d: %s, EQ, dynamics, drive, flanger and room on, chorus %s, delay %s, reverb %s" % ((k + 1, kind) + tuple("on" if o else "off" for o in on))
            if kind == "bus fill":
                bus_fill(what, 32)
            else:
                master_fill(what, 32, stems=j % 2 == 0)
            k += 1
    assert k == 24 and len(lims) == 1 and lims[0].limited() > 0.0       # on the model, before anything is compared: the walk limits
    fl.busy("the walk")
    for what, cmp in steps:
        for name, (got, want) in cmp.items():
            assert_bits_equal_finite(got, want, "%s: %s" % (what, name))
    mm.check_committed(a)
    _states(a, fl, "after the walk")


def test_without_feedback_it_is_the_twins_one_voice_chorus():
    """no model in the loop: feedback = cross = 0 on one handle, a chorus of one voice at the same parameters on its twin.  As VALUES,
    not on bits: the flanger's line is x + (+0.0), which turns a -0.0 of the bus over, and the chorus keeps the bus's own zero"""
    a, b = _handles()
    for k, H in enumerate((34, 145, 4096)):
        a.set_bus_flanger(k, *SHAPE[H], INC * 8, SPREAD, 0.0, 0.0, 0.5, 0.75)
        b.set_bus_chorus(k, 1, *SHAPE[H], INC * 8, SPREAD, 0.5, 0.75)
    for fill, n in enumerate([1024, 33, 1, 1024, 700]):
        _events((a, b), V, fill)
        ya, yb = a.sample_buses(n, SR, 4), b.sample_buses(n, SR, 4)
        assert np.isfinite(ya).all() and np.array_equal(ya, yb), "fill %d" % fill
        assert ubits(ya[:3]).any() and np.array_equal(ubits(ya[3]), ubits(yb[3]))
    for k in range(3):
        (ha, pa), (hb, pb) = a.bus_flanger_state(k), b.bus_chorus_state(k)
        assert np.array_equal(ha, hb) and pa == pb and ha.any()


def test_half_the_wet_is_half():
    """no model in the loop: the line does not know the wet level, so with no dry part a twin at wet 0.5 returns half of what wet 1
    returns — the product by 0.5 is exact or rounds as numpy's.  As values: a zero may come out with either sign"""
    a, b = _handles()
    for k, (H, mix) in enumerate(((33, FULL), (65, NEG), (1024, CROSS))):
        a.set_bus_flanger(k, *SHAPE[H], INC, SPREAD, *mix, 0.0, 1.0)
        b.set_bus_flanger(k, *SHAPE[H], INC, SPREAD, *mix, 0.0, 0.5)
    for fill, n in enumerate([1024, 69, 1024]):
        _events((a, b), V, fill)
        ya, yb = a.sample_buses(n, SR, 3), b.sample_buses(n, SR, 3)
        assert np.isfinite(ya).all() and ubits(ya).any()
        with np.errstate(under="ignore"):
            assert np.array_equal(yb, F(0.5) * ya), "fill %d" % fill
    for k in range(3):
        (ha, pa), (hb, pb) = a.bus_flanger_state(k), b.bus_flanger_state(k)
        assert_bits_equal_finite(ha, hb, "the line of bus %d knows nothing of the wet level" % k)
        assert pa == pb


def test_a_master_fill_applies_the_flanger():
    """stems and master of s2r_fill_master against the models: the flanger, then the master section, and then the limiter"""
    a, b = _handles()
    model, mm = FlangerModel(), Master()
    _set(a, model, 0, 34, FB, (0.0, 1.0))
    _set(a, model, 2, 145, NEG, (0.5, 0.5))
    lim = None
    for fill, n in enumerate([300, 1, 300, 64, 33]):
        _events((a, b), V, fill)
        y = model.expect(b.sample_buses(n, SR, 3))
        m = mm.expect(y)
        if fill == 3:
            ceiling = float(np.abs(m).max()) / 2.0               # half this master's peak: the limiter works
            lim = Lim(48, 0, ceiling)
            lim.set((a,), ceiling)
        got, st = a.sample_master(n, SR, 3, stems=True)
        assert_bits_equal_finite(st, y, "the stems of a master fill, fill %d" % fill)
        assert_bits_equal_finite(got, lim.expect(m)[0] if lim else m, "the master, fill %d" % fill)
        _states(a, model, "master fill %d" % fill)
    model.busy("master fills")


def test_new_parameters_in_mid_stream_keep_line_and_phase_and_a_set_zeroes_them():
    a, b = _handles()
    model = FlangerModel()
    _set(a, model, 1, 65, FB, (0.0, 1.0))
    _events((a, b), V, 0)
    _fill(a, b, model, 300, 2, "before the parameters move")
    hist, phase = a.bus_flanger_state(1)
    assert hist.any() and phase == (INC * 300) & 0xFFFFFFFF
    a.set_bus_flanger_params(1, INC * 3, 7, -0.5, 0.5, 0.5, 0.25)
    model.f[1].update(inc=INC * 3, spread=7, mix=(-0.5, 0.5, 0.5, 0.25))
    assert a.get_bus_flanger(1) == SHAPE[65] + (INC * 3, 7, -0.5, 0.5, 0.5, 0.25)
    got, ph = a.bus_flanger_state(1)
    assert_bits_equal_finite(got, hist, "the line under new parameters")
    assert ph == phase
    for fill, n in enumerate([300, 33], start=1):
        _events((a, b), V, fill)
        _fill(a, b, model, n, 2, "after s2r_set_bus_flanger_params, fill %d" % fill)
    _states(a, model, "after the parameters moved")
    _set(a, model, 1, 65, FB, (0.0, 1.0))                        # setting it again zeroes line and phase
    _events((a, b), V, 3)
    _fill(a, b, model, 64, 2, "after s2r_set_bus_flanger")
    _states(a, model, "from silence")
    with pytest.raises(s2.S2rError) as err:
        a.set_bus_flanger_params(0, 1, 2, 0.0, 0.0, 1.0, 1.0)
    assert err.value.status == s2s.S2R_ERR_INVALID


def test_checkpoint_state_out_and_in():
    """line and phase out, more calls, line and phase back in, the same calls: the same bits"""
    a, b = _handles(max_frames=512)
    model = FlangerModel()
    _set(a, model, 0, 145, NEG, (0.25, 1.0))
    _set(a, model, 1, 4096, FB, (0.0, 1.0))
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
        c.set_bus_flanger(bus, *a.get_bus_flanger(bus))
        c.set_bus_flanger_state(bus, *a.bus_flanger_state(bus))
    for k, n in enumerate([100, 400, 33]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        _, got = _fill(a, b, model, n, 2, "the checkpointed handle, fill %d" % k)
        assert_bits_equal_finite(c.sample_buses(n, SR, 2), got, "the resumed handle, fill %d" % k)
    for bus in (0, 1):
        (ha, pa), (hc, pc) = a.bus_flanger_state(bus), c.bus_flanger_state(bus)
        assert_bits_equal_finite(hc, ha, "line of bus %d" % bus)
        assert pa == pc
    # the flanger is the bus's: a new bank, a program change and an imported state leave it and its state alone
    keep, kp = a.bus_flanger_state(1)
    a.set_patch_bank(_bank())
    a.program_change(3)
    a.import_state(state)
    got, gp = a.bus_flanger_state(1)
    assert a.get_bus_flanger(1)[0] == 32.0 and np.array_equal(bits(got), bits(keep)) and gp == kp


def test_refusals_removal_and_the_other_fills():
    """a fill refused before any launch leaves line and phase untouched, in a bus fill and in a master fill; the panned, mono and stereo
    fills ignore the flanger; after a removal the bus is the twin's on bits again; a device-list handle refuses every entry and renders
    on"""
    a, b = _handles(max_frames=256)
    model = FlangerModel()
    _set(a, model, 0, 34, FB, (0.0, 1.0))
    _events((a, b), V, 0)
    _fill(a, b, model, 100, 2, "before the refusals")
    before, phase = a.bus_flanger_state(0)
    L, h = a.L, a.h
    out, lr = np.empty(2 * 2 * 300, dtype=F), np.empty(2 * 300, dtype=F)
    p, q = out.ctypes.data_as(s2s._f32p), lr.ctypes.data_as(s2s._f32p)
    assert L.s2r_fill_buses(h, p, 2 * 2 * 100 - 1, 2, 100, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_buses(h, p, out.size, 9, 16, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_buses(h, p, out.size, 2, 257, SR) == s2s.S2R_ERR_TOO_MANY_FRAMES
    assert L.s2r_fill_master(h, q, p, 2 * 2 * 100 - 1, 2, 100, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_master(h, q, p, out.size, 2, 257, SR) == s2s.S2R_ERR_TOO_MANY_FRAMES
    got, ph = a.bus_flanger_state(0)
    assert_bits_equal_finite(got, before, "the line after refused fills")
    assert ph == phase
    # the other fills
    assert_bits_equal_finite(a.sample_panned(100, SR), b.sample_panned(100, SR), "panned fill beside a flanger")
    assert_bits_equal_finite(a.sample(np.empty(64, dtype=F), SR), b.sample(np.empty(64, dtype=F), SR), "mono fill beside a flanger")
    assert_bits_equal_finite(a.sample_stereo(33, SR), b.sample_stereo(33, SR), "stereo copy beside a flanger")
    got, ph = a.bus_flanger_state(0)
    assert_bits_equal_finite(got, before, "the line after the other fills")
    assert ph == phase
    _events((a, b), V, 1)
    _fill(a, b, model, 64, 2, "after the refusals and the other fills")
    # removal
    a.clear_bus_flanger(0)
    del model.f[0]
    assert a.get_bus_flanger(0)[0] == 0.0
    _events((a, b), V, 2)
    x = b.sample_buses(64, SR, 2)
    assert_bits_equal_finite(a.sample_buses(64, SR, 2), x, "no flanger left: the twin's")
    # a device list
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    one = s2.Synth(512, max_frames=64, mix_groups=2)
    for syn in (multi, one):
        for v in range(512):
            syn.note_on(36 + v % 61)
    buf, k = np.zeros(80, dtype=F), C.c_uint32()
    bp = buf.ctypes.data_as(s2s._f32p)
    assert multi.L.s2r_set_bus_flanger(multi.h, 0, 32.0, 0.0, 1, 2, 0.5, 0.5, 0.5, 0.5) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_clear_bus_flanger(multi.h, 0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_flanger_params(multi.h, 0, 1, 2, 0.5, 0.5, 0.5, 0.5) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_flanger(multi.h, 0, None, None, C.byref(k), None, None, None, None, None) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_flanger_state(multi.h, 0, bp, 66, None) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_flanger_state(multi.h, 0, bp, 66, 0) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        multi.set_bus_flanger(0, 32.0, 0.0, 1, 2, 0.5, 0.5, 0.5, 0.5)
    assert err.value.status == s2s.S2R_ERR_INVALID
    x, y = multi.sample(np.empty(64, dtype=F), SR), one.sample(np.empty(64, dtype=F), SR)
    assert np.abs(y).max() > 0.0
    assert_bits_equal_finite(x, y, "the device-list handle after the refused flanger calls")


def test_range_checks_on_a_handle():
    check_ranges(s2.Synth(8, max_frames=64))


def test_a_handle_that_never_had_a_flanger_and_the_timing_entry():
    """s2r_debug_bus_flanger_ms: -1 without s2r_set_timing; under it 0 after a bus fill and a master fill of a handle that never had a
    flanger, whose outputs are the twin's and which holds nothing for one; and the kernel's time once a flanger is set"""
    a, b = _handles()
    ms, alloc = a.L.s2r_debug_bus_flanger_ms, a.L.s2r_debug_flanger_allocated
    ms.restype, ms.argtypes = C.c_float, [C.c_void_p]
    alloc.restype, alloc.argtypes = C.c_int, [C.c_void_p]
    _events((a, b), V, 0)
    assert_bits_equal_finite(a.sample_buses(300, SR, 3), b.sample_buses(300, SR, 3), "no flanger, timing off")
    assert ms(a.h) == -1.0
    a.set_timing(True)
    _events((a, b), V, 1)
    assert_bits_equal_finite(a.sample_buses(300, SR, 3), b.sample_buses(300, SR, 3), "no flanger, bus fill under timing")
    assert ms(a.h) == 0.0
    _events((a, b), V, 2)
    (ma, sa), (mb, sb) = a.sample_master(300, SR, 3), b.sample_master(300, SR, 3)
    assert_bits_equal_finite(ma, mb, "no flanger, master fill under timing")
    assert_bits_equal_finite(sa, sb, "no flanger, the stems of a master fill")
    assert ms(a.h) == 0.0 and alloc(a.h) == 0
    a.set_bus_flanger(4, *SHAPE[145], INC, SPREAD, 0.5, 0.25, 0.5, 0.5)
    assert alloc(a.h) == 1
    a.sample_buses(300, SR, 5)
    assert 0.0 < ms(a.h) < 100.0
    a.sample_buses(300, SR, 3)                                   # the flanger is past the call's buses: idle, no kernel
    assert ms(a.h) == 0.0
