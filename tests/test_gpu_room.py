"""The per-bus room reverb on the device.  Twin handles on pools of 32 voices are fed the same events, one with rooms and
one without; the twin's bus output is what enters the chain, and the expectation is the rule on the host (s2.room_reference, which
tests/test_room_host.py holds to a numpy float32 model on bits) with the state carried from call to call (RoomModel), behind the models
of the stages in front of it.

The kernel works in tiles of T frames (s2r_debug_room_tile), loads a tile ahead and writes the combs' lines a phase behind — a pipeline
two tiles deep —, so the call lengths are 1, 2, T - 1, T, T + 1, 2T + 1, 2T, 300 (a line of 64 frames turns over more than four times
inside the call) and 1024 = max_frames.  Handles, events and the one-pole bank are tests/test_gpu_reverb.py's.  Every comparison is on
bits with no NaN allowance (helpers.assert_bits_equal_finite)."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_room_host import FLAT, SMALL, bits, check_ranges
from test_gpu_buses import ubits
from test_gpu_chorus import SHAPES, ChorusModel
from test_gpu_delay import DelayModel
from test_gpu_dyn import DynModel
from test_gpu_eq import EqModel, _coeffs
from test_gpu_limiter import Lim
from test_gpu_master import Master
from test_gpu_reverb import SR, Model, _bank, _events, _handles as _reverb_handles, _ir, _timed
from test_master_host import np_meters

pytestmark = pytest.mark.gpu
F = np.float32

V = 32                                                           # voices of a pool
T = 32                                                           # S2R_ROOM_TILE (csrc/s2r_device.h); test_the_tile_is_the_kernels holds it to the library
DEPTH = 2                                                        # tiles between a line's load and the write that follows it
FRAMES = [1024, 1, 2, T - 1, T, T + 1, 2 * T + 1, DEPTH * T, 300, 1, 1024]
LONG = ([8192] * 8, [8192] * 4, 0)
# seven levels by name: (feedback, damp, g, gain, dry, wet, cross)
LEVELS = {"hall": (0.84, 0.2, 0.5, 0.25, 0.75, 0.5, 0.25), "dark": (0.7, 0.9, -0.6, 0.5, 0.0, 1.0, 0.0), "wide": (0.95, 0.0, 0.7, 0.125, 1.0, 0.25, 1.0)}
# (n_buses, what each bus carries: a (delays, levels) pair by name, or None); in the last row buses 6 and 7 sound through sends alone
MATRIX = [(1, ("small:hall",)), (2, (None, "flat:dark")), (3, ("flat:hall", None, "small:wide")),
          (8, ("small:hall", "flat:wide", None, "design:hall", "small:dark", None, "flat:hall", "design:wide"))]


def _delays(name):
    return {"flat": FLAT, "small": SMALL, "long": LONG}[name] if name != "design" else tuple(s2.room_design(48000.0))


def _handles(max_frames=1024):
    return _reverb_handles(voices=V, max_frames=max_frames)


def _tile():
    L = s2.load_library()
    L.s2r_debug_room_tile.restype, L.s2r_debug_room_tile.argtypes = C.c_uint32, []
    return int(L.s2r_debug_room_tile())


class RoomModel:
    """the rooms of a handle on the host: per bus the delays, the levels and the carried state"""

    def __init__(self):
        self.r = {}

    def set(self, bus, delays, levels):
        cd, ad, sp = delays
        self.r[bus] = dict(delays=(np.array(cd, dtype=np.uint32), np.array(ad, dtype=np.uint32), int(sp)), lv=tuple(levels),
                           st=np.zeros(s2.room_state_floats(cd, ad, sp), dtype=F))

    def expect(self, x):
        """what the stage makes of a call whose buses enter it as x [n_buses, N, 2]; the states of its buses move on"""
        want = x.copy()
        for b, f in self.r.items():
            if b >= x.shape[0]:
                continue                                         # idle in this call
            cd, ad, sp = f["delays"]
            want[b], f["st"] = s2.room_reference(cd, ad, sp, *f["lv"], x[b], f["st"])
        return want


def _set(a, model, bus, delays, levels):
    cd, ad, sp = delays
    a.set_bus_room(bus, cd, ad, sp, *levels)
    got = a.get_bus_room(bus)
    assert list(got[0]) == list(cd) and list(got[1]) == list(ad) and got[2] == sp
    assert np.array_equal(bits(np.array(got[3:], dtype=F)), bits(np.array(levels, dtype=F)))
    model.set(bus, delays, levels)
    assert not a.bus_room_state(bus).any() and a.bus_room_state(bus).size == model.r[bus]["st"].size


def _set_named(a, model, bus, name):
    d, lv = name.split(":")
    _set(a, model, bus, _delays(d), LEVELS[lv])


def _fill(a, b, model, n, nb, what, differs=True):
    """one call on both handles: the buses with a room against the model over the twin's, the others against the twin's"""
    x = b.sample_buses(n, SR, nb)
    assert np.isfinite(x).all()
    want = model.expect(x)
    got = a.sample_buses(n, SR, nb)
    assert_bits_equal_finite(got, want, what)
    for bus in range(nb):
        if bus in model.r:
            assert ubits(x[bus]).any(), "%s: bus %d is silent" % (what, bus)
            if differs:
                assert not np.array_equal(ubits(got[bus]), ubits(x[bus])), "%s: the room on bus %d changes no bit" % (what, bus)
        else:
            assert_bits_equal_finite(got[bus], x[bus], "%s: bus %d, which carries no room" % (what, bus))
    return x, got


def _states(a, model, what):
    for bus, f in model.r.items():
        assert_bits_equal_finite(a.bus_room_state(bus), f["st"], "%s: state of bus %d" % (what, bus))


def test_the_tile_is_the_kernels():
    assert _tile() == T and 2 * T <= s2.ROOM_MIN_DELAY


@pytest.mark.parametrize("n_buses,rooms", MATRIX)
def test_rooms_are_the_rule_over_the_twins_buses(n_buses, rooms):
    """the parity matrix: calls of max_frames, then 1, 2, T - 1, T, T + 1, 2T + 1, 2T, 300, 1 frames and max_frames again on one pair
    of handles; the state is read back at the end and once in the middle.  Everything the device returns is collected first, then
    compared."""
    a, b = _handles()
    model = RoomModel()
    for bus, name in enumerate(rooms):
        if name is not None:
            _set_named(a, model, bus, name)
    steps = []
    for fill, n in enumerate(FRAMES):
        _events((a, b), V, fill)
        what = "%d buses, %s, fill %d of %d frames" % (n_buses, rooms, fill, n)
        x = b.sample_buses(n, SR, n_buses)
        want = model.expect(x)
        got = a.sample_buses(n, SR, n_buses)
        st = {bus: (a.bus_room_state(bus), f["st"].copy()) for bus, f in model.r.items()} if fill in (4, len(FRAMES) - 1) else {}
        steps.append((what, x, want, got, st))
    for k, (what, x, want, got, st) in enumerate(steps):
        assert np.isfinite(x).all()
        assert_bits_equal_finite(got, want, what)
        for bus in range(n_buses):
            if bus in model.r:
                assert ubits(x[bus]).any(), "%s: bus %d is silent" % (what, bus)
                # (the design's shortest comb is 1215 frames: with dry = 1 its room changes no bit before the second call ends; by the
                # last call every line has turned over)
                if k == len(steps) - 1:
                    assert not np.array_equal(ubits(got[bus]), ubits(x[bus])), "%s: the room on bus %d changes no bit" % (what, bus)
            else:
                assert_bits_equal_finite(got[bus], x[bus], "%s: bus %d, which carries no room" % (what, bus))
        for bus, (g, w) in st.items():
            assert_bits_equal_finite(g, w, "%s: state of bus %d" % (what, bus))


def test_every_delay_at_its_largest():
    """one bus with all 24 lines of 8192 frames: nine calls until the lines have turned over, then the tail"""
    a, b = _handles()
    model = RoomModel()
    _set(a, model, 0, LONG, LEVELS["hall"])
    for fill, n in enumerate([1024] * 8 + [1, 1024, T + 1, 300]):
        _events((a, b), V, fill)
        _fill(a, b, model, n, 1, "delays of 8192, fill %d" % fill, differs=fill >= 8)
    _states(a, model, "delays of 8192")


def test_a_crafted_state_is_read_from_the_first_frame():
    """no twin history needed: a state with nothing regular about it goes in, comes back, and the first call of one frame reads every
    line's oldest frame and every f"""
    a, b = _handles()
    model = RoomModel()
    _set(a, model, 1, SMALL, LEVELS["hall"])
    _events((a, b), V, 0)
    _fill(a, b, model, 300, 2, "before the state is crafted")   # (a voice's first frame is +0.0: the calls of one frame come later)
    st = (np.random.default_rng(3).standard_normal(model.r[1]["st"].size) * 0.25).astype(F)
    a.set_bus_room_state(1, st)
    model.r[1]["st"] = st.copy()
    assert_bits_equal_finite(a.bus_room_state(1), st, "the state set and read back")
    for fill, n in enumerate([1, 2, T + 1, 300], start=1):
        _events((a, b), V, fill)
        _fill(a, b, model, n, 2, "from a crafted state, fill %d" % fill)
        _states(a, model, "from a crafted state, fill %d" % fill)


def test_gain_zero_and_dry_one_pass_the_twin():
    """no model in the loop: from silence with gain 0 nothing enters a line, so the bus is the twin's up to the sign of zero"""
    a, b = _handles()
    a.set_bus_room(0, *SMALL, 0.84, 0.2, 0.5, 0.0, 1.0, 1.0, 1.0)
    for fill, n in enumerate([300, 1, 2 * T + 1]):
        _events((a, b), V, fill)
        x = b.sample_buses(n, SR, 2)
        got = a.sample_buses(n, SR, 2)
        assert ubits(x).any()
        assert_bits_equal_finite(got[0], x[0] + F(0.0), "gain 0, dry 1, fill %d" % fill)
        assert_bits_equal_finite(got[1], x[1], "the bus beside it")
    assert not a.bus_room_state(0).any()


def test_a_run_of_short_calls_is_one_long_call():
    """no model in the loop: four handles, two with the same rooms; one of each kind renders the same frames in a run of calls, the
    other in one call.  The mixdown itself is one stream only where calls are cut at multiples of 16 — asserted on the handles
    without rooms —, and the cuts here are such.  On bits, the two handles with the rooms agree, outputs and states"""
    a, b, c, d = _handles() + _handles()
    for syn in (a, c):
        syn.set_bus_room(0, *SMALL, *LEVELS["hall"])
        syn.set_bus_room(2, *FLAT, *LEVELS["wide"])
    cuts = [16, 48, 16, T, T + 16, 16, 64, 2 * T + 16, 304, 96]
    total = sum(cuts)
    assert total <= 1024 and all(n % 16 == 0 for n in cuts)
    _events((a, b, c, d), V, 0)
    short_room = np.concatenate([a.sample_buses(n, SR, 3) for n in cuts], axis=1)
    short_dry = np.concatenate([b.sample_buses(n, SR, 3) for n in cuts], axis=1)
    long_room, long_dry = c.sample_buses(total, SR, 3), d.sample_buses(total, SR, 3)
    assert_bits_equal_finite(short_dry, long_dry, "without rooms: the mixdown in short calls and in one")
    assert_bits_equal_finite(short_room, long_room, "with the rooms: short calls and one long call")
    assert_bits_equal_finite(short_room[1], long_dry[1], "the bus without a room")
    for bus in (0, 2):
        assert not np.array_equal(ubits(long_room[bus]), ubits(long_dry[bus]))
        assert_bits_equal_finite(a.bus_room_state(bus), c.bus_room_state(bus), "the state of bus %d after both" % bus)


@pytest.mark.parametrize("frames", [250, 64])
def test_events_inside_a_fill_and_sliced_rows(frames, monkeypatch):
    """note_ons at frames 16 and 48 split the call into segments and a rows buffer of 48 frames slices them further: the stage sees the
    call as one stream"""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    a, b = _handles(max_frames=256)
    model = RoomModel()
    _set(a, model, 0, SMALL, LEVELS["hall"])
    _set(a, model, 3, FLAT, LEVELS["dark"])
    for fill in range(3):
        _events((a, b), V, fill)
        _timed((a, b), fill)
        _fill(a, b, model, frames, 4, "events at 16 and 48, slices of 48, %d frames, fill %d" % (frames, fill))
    _states(a, model, "events and slices")
    a.L.s2r_debug_pan_slice.restype = C.c_uint32
    a.L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    assert a.L.s2r_debug_pan_slice(a.h) == 48


def test_a_send_only_bus_with_a_room_while_a_fader_ramps():
    """bus 6 of eight sounds through program 0's send alone and carries a room; program 0's fader moves across the second and third
    call — on both handles, so the twin's bus 6 enters the stage under the same sends and ramps"""
    a, b = _handles()
    model = RoomModel()
    _set(a, model, 6, SMALL, LEVELS["hall"])
    walk = [(1.0, 0.0), (0.25, 1.0), (0.7, -0.5), (0.7, -0.5)]
    for fill, n in enumerate([300, 1000, 17, 64]):
        _events((a, b), V, fill)
        for syn in (a, b):
            syn.set_program_fader(0, *walk[fill])
        _fill(a, b, model, n, 8, "send-only bus under a fader ramp, fill %d" % fill)
        f = a.get_program_fader(0)
        assert f == b.get_program_fader(0) and f[:2] == f[2:]    # committed on both
    _states(a, model, "under the ramps")


def test_the_room_behind_a_convolution_reverb_on_the_same_bus():
    """a short measured response for the early reflections, the room for the tail: the room reads what the reverb wrote"""
    a, b = _handles()
    rv, model = Model(), RoomModel()
    ir = _ir(40, 77, True)
    a.set_bus_reverb(1, ir, 0.25, 1.0)
    rv.set(1, ir, 0.25, 1.0)
    _set(a, model, 1, SMALL, LEVELS["hall"])
    _set(a, model, 0, FLAT, LEVELS["wide"])
    for fill, n in enumerate([300, 1, T + 1, 1024]):
        _events((a, b), V, fill)
        x = b.sample_buses(n, SR, 3)
        y = rv.expect(x)
        assert not np.array_equal(ubits(y[1]), ubits(x[1]))
        assert_bits_equal_finite(a.sample_buses(n, SR, 3), model.expect(y), "reverb, then room, fill %d" % fill)
    _states(a, model, "behind the reverb")


def test_every_route_with_the_eq_the_dynamics_and_the_room_on():
    """Handle `a` walks all 24 rows of s2r_post_route's table with EQs, dynamics and rooms on, T frames a call — a bus fill, a master
    fill and a master fill under the limiter, each with every subset of chorus, delay and reverb, master fills with and without
    stems —; its twin `b` makes a plain bus fill of the same frames every time.  Every step's expectation is the chain of the models:
    EQ, dynamics, chorus, delay, reverb, room, master section, limiter.  Everything the device returns is collected first, then compared."""
    a, b = _handles()
    eq, dy, ch, dl, rv, rm, mm = EqModel(), DynModel(), ChorusModel(), DelayModel(), Model(), RoomModel(), Master()
    for bus, nb in enumerate((2, 4, 1)):
        c = _coeffs(nb, bus + 1)
        a.set_bus_eq(bus, c)
        eq.set(bus, c)
    curve = s2.dynamics_curve(-30.0, 4.0, 6.0, 3.0)
    for bus, key in enumerate((0, 0, 2)):
        a.set_bus_dynamics(bus, key, curve, 0.9, 0.999)
        dy.set(bus, key, curve, 0.9, 0.999)
    _set(a, rm, 0, FLAT, LEVELS["hall"])
    _set(a, rm, 1, SMALL, LEVELS["dark"])                        # (bus 2 carries none: the room's launch copies it)
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
        y = rv.expect(dl.expect(ch.expect(dy.expect(eq.expect(x)))))
        z = rm.expect(y)
        assert all(not np.array_equal(ubits(z[q]), ubits(y[q])) for q in (0, 1)) and np.array_equal(ubits(z[2]), ubits(y[2]))
        return z

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
            what = "%d: %s, EQ, dynamics and room on, chorus %s, delay %s, reverb %s" % ((k + 1, kind) + tuple("on" if o else "off" for o in on))
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
    _states(a, rm, "after the walk")


def test_a_room_past_the_calls_buses_is_idle():
    """a room on bus 5: in calls of three buses its crafted state stays; bus 0 beside it runs; a call of eight buses goes on from it"""
    a, b = _handles()
    model = RoomModel()
    _set(a, model, 0, SMALL, LEVELS["hall"])
    _set(a, model, 5, FLAT, LEVELS["wide"])
    st = (np.random.default_rng(4).standard_normal(model.r[5]["st"].size) * 0.25).astype(F)
    a.set_bus_room_state(5, st)
    model.r[5]["st"] = st.copy()
    for fill, n in enumerate([300, 2, T + 1]):
        _events((a, b), V, fill)
        _fill(a, b, model, n, 3, "a room past the call's buses, fill %d" % fill)
    assert_bits_equal_finite(a.bus_room_state(5), st, "the idle room's state")
    _events((a, b), V, 3)
    _fill(a, b, model, 100, 8, "eight buses: the idle room wakes from its crafted state")
    _states(a, model, "after the call of eight buses")
    assert not np.array_equal(bits(a.bus_room_state(5)), bits(st))


def test_new_levels_in_mid_tail_keep_the_state_and_a_set_zeroes_it():
    a, b = _handles()
    model = RoomModel()
    _set(a, model, 1, SMALL, LEVELS["hall"])
    _events((a, b), V, 0)
    _fill(a, b, model, 300, 2, "before the levels move")
    st = a.bus_room_state(1)
    assert st.any()
    a.set_bus_room_params(1, *LEVELS["dark"])
    model.r[1]["lv"] = LEVELS["dark"]
    assert_bits_equal_finite(a.bus_room_state(1), st, "the state under new levels")
    got = a.get_bus_room(1)
    assert list(got[0]) == SMALL[0] and got[2] == 3 and np.array_equal(bits(np.array(got[3:], dtype=F)), bits(np.array(LEVELS["dark"], dtype=F)))
    _events((a, b), V, 1)
    _fill(a, b, model, 300, 2, "after s2r_set_bus_room_params")
    _states(a, model, "after the levels moved")
    _set(a, model, 1, SMALL, LEVELS["dark"])                     # setting it again zeroes the state
    _events((a, b), V, 2)
    _fill(a, b, model, 64, 2, "after s2r_set_bus_room")
    _states(a, model, "from silence")
    with pytest.raises(s2.S2rError) as err:
        a.set_bus_room_params(0, *LEVELS["dark"])
    assert err.value.status == s2s.S2R_ERR_INVALID


def test_checkpoint_in_mid_tail():
    """the notes are released and the room rings on; state, pans, mix, sends, the room's parameters and state go into a fresh handle:
    the next fills are equal"""
    a, b = _handles(max_frames=512)
    model = RoomModel()
    _set(a, model, 0, SMALL, LEVELS["hall"])
    _set(a, model, 1, _delays("design"), LEVELS["hall"])
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
        c.set_bus_room(bus, *a.get_bus_room(bus))
        c.set_bus_room_state(bus, a.bus_room_state(bus))
    for k, n in enumerate([100, 400]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        _, got = _fill(a, b, model, n, 2, "the checkpointed handle, fill %d" % k)
        assert_bits_equal_finite(c.sample_buses(n, SR, 2), got, "the resumed handle, fill %d" % k)
    for bus in (0, 1):
        assert_bits_equal_finite(c.bus_room_state(bus), a.bus_room_state(bus), "state of bus %d" % bus)
    # the room is the bus's: a new bank, a program change and an imported state leave it and its state alone
    keep = a.bus_room_state(1)
    a.set_patch_bank(_bank())
    a.program_change(3)
    a.import_state(state)
    assert a.get_bus_room(1)[2] == 25 and np.array_equal(bits(a.bus_room_state(1)), bits(keep))


def test_refusals_removal_and_the_other_fills():
    """a fill refused before any launch leaves the state untouched, in a bus fill and in a master fill; the panned, mono and stereo
    fills ignore the room; the state pair's count and capacity checks; after a removal the bus is the twin's on bits again; a
    device-list handle refuses every entry and renders on"""
    a, b = _handles(max_frames=256)
    model = RoomModel()
    _set(a, model, 0, SMALL, LEVELS["hall"])
    _events((a, b), V, 0)
    _fill(a, b, model, 100, 2, "before the refusals")
    before = a.bus_room_state(0)
    L, h = a.L, a.h
    out, lr = np.empty(2 * 2 * 300, dtype=F), np.empty(2 * 300, dtype=F)
    p, q = out.ctypes.data_as(s2s._f32p), lr.ctypes.data_as(s2s._f32p)
    assert L.s2r_fill_buses(h, p, 2 * 2 * 100 - 1, 2, 100, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_buses(h, p, out.size, 9, 16, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_buses(h, p, out.size, 2, 257, SR) == s2s.S2R_ERR_TOO_MANY_FRAMES
    assert L.s2r_fill_master(h, q, p, 2 * 2 * 100 - 1, 2, 100, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_master(h, q, p, out.size, 2, 257, SR) == s2s.S2R_ERR_TOO_MANY_FRAMES
    assert_bits_equal_finite(a.bus_room_state(0), before, "the state after refused fills")
    # the state pair
    n = before.size
    buf = np.zeros(n + 1, dtype=F)
    bp = buf.ctypes.data_as(s2s._f32p)
    assert L.s2r_get_bus_room_state(h, 0, bp, n - 1) == s2s.S2R_ERR_INVALID and L.s2r_get_bus_room_state(h, 0, None, n) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_room_state(h, 0, bp, n + 1) == s2s.S2R_OK and np.array_equal(bits(buf[:n]), bits(before)) and buf[n] == 0.0
    assert L.s2r_set_bus_room_state(h, 0, bp, n - 1) == s2s.S2R_ERR_INVALID and L.s2r_set_bus_room_state(h, 0, bp, n + 1) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_room_state(h, 0, None, n) == s2s.S2R_ERR_INVALID and L.s2r_get_bus_room_state(h, 1, bp, n) == s2s.S2R_ERR_INVALID
    for v in (np.nan, np.inf, -np.inf):
        bad = before.copy()
        bad[n // 2] = v
        assert L.s2r_set_bus_room_state(h, 0, bad.ctypes.data_as(s2s._f32p), n) == s2s.S2R_ERR_PATCH_RANGE
    assert_bits_equal_finite(a.bus_room_state(0), before, "the state after refused restores")
    # the other fills
    assert_bits_equal_finite(a.sample_panned(100, SR), b.sample_panned(100, SR), "panned fill beside a room")
    assert_bits_equal_finite(a.sample(np.empty(64, dtype=F), SR), b.sample(np.empty(64, dtype=F), SR), "mono fill beside a room")
    assert_bits_equal_finite(a.sample_stereo(33, SR), b.sample_stereo(33, SR), "stereo copy beside a room")
    assert_bits_equal_finite(a.bus_room_state(0), before, "the state after the other fills")
    _events((a, b), V, 1)
    _fill(a, b, model, 64, 2, "after the refusals and the other fills")
    # removal
    a.clear_bus_room(0)
    del model.r[0]
    assert a.get_bus_room(0) is None
    _events((a, b), V, 2)
    x = b.sample_buses(64, SR, 2)
    assert_bits_equal_finite(a.sample_buses(64, SR, 2), x, "no room left: the twin's")
    # a device list
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    one = s2.Synth(512, max_frames=64, mix_groups=2)
    for syn in (multi, one):
        for v in range(512):
            syn.note_on(36 + v % 61)
    cd, ad = np.full(8, 100, dtype=np.uint32), np.full(4, 100, dtype=np.uint32)
    cp, ap, k = cd.ctypes.data_as(s2s._u32p), ad.ctypes.data_as(s2s._u32p), C.c_uint32()
    lv = (0.5,) * 7
    assert multi.L.s2r_set_bus_room(multi.h, 0, cp, ap, 0, *lv) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_clear_bus_room(multi.h, 0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_room_params(multi.h, 0, *lv) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_room(multi.h, 0, C.byref(k), None, None, None, None) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_room_state(multi.h, 0, bp, n) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_room_state(multi.h, 0, bp, n) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        multi.set_bus_room(0, cd, ad, 0, *lv)
    assert err.value.status == s2s.S2R_ERR_INVALID
    x, y = multi.sample(np.empty(64, dtype=F), SR), one.sample(np.empty(64, dtype=F), SR)
    assert np.abs(y).max() > 0.0
    assert_bits_equal_finite(x, y, "the device-list handle after the refused room calls")


def test_a_master_fill_applies_the_room():
    """stems and master of s2r_fill_master against the models: the room, then the master section"""
    a, b = _handles()
    model, mm = RoomModel(), Master()
    _set(a, model, 0, SMALL, LEVELS["hall"])
    _set(a, model, 2, FLAT, LEVELS["wide"])
    for fill, n in enumerate([T + 1, 1, 300]):
        _events((a, b), V, fill)
        y = model.expect(b.sample_buses(n, SR, 3))
        got, st = a.sample_master(n, SR, 3, stems=True)
        assert_bits_equal_finite(st, y, "the stems of a master fill, fill %d" % fill)
        assert_bits_equal_finite(got, mm.expect(y), "the master, fill %d" % fill)
        _states(a, model, "master fill %d" % fill)


def test_range_checks_on_a_handle():
    check_ranges(s2.Synth(8, max_frames=64))


def test_a_handle_that_never_had_a_room_and_the_timing_entry():
    """s2r_debug_bus_room_ms: -1 without s2r_set_timing; under it 0 after a bus fill and a master fill of a handle that never had a
    room, whose outputs are the twin's and which holds nothing for one; and the kernel's time once a room is set"""
    a, b = _handles()
    ms, alloc = a.L.s2r_debug_bus_room_ms, a.L.s2r_debug_room_allocated
    ms.restype, ms.argtypes = C.c_float, [C.c_void_p]
    alloc.restype, alloc.argtypes = C.c_int, [C.c_void_p]
    _events((a, b), V, 0)
    assert_bits_equal_finite(a.sample_buses(300, SR, 3), b.sample_buses(300, SR, 3), "no room, timing off")
    assert ms(a.h) == -1.0
    a.set_timing(True)
    _events((a, b), V, 1)
    assert_bits_equal_finite(a.sample_buses(300, SR, 3), b.sample_buses(300, SR, 3), "no room, bus fill under timing")
    assert ms(a.h) == 0.0
    _events((a, b), V, 2)
    (ma, sa), (mb, sb) = a.sample_master(300, SR, 3), b.sample_master(300, SR, 3)
    assert_bits_equal_finite(ma, mb, "no room, master fill under timing")
    assert_bits_equal_finite(sa, sb, "no room, the stems of a master fill")
    assert ms(a.h) == 0.0 and alloc(a.h) == 0
    a.set_bus_room(4, *SMALL, *LEVELS["hall"])
    assert alloc(a.h) == 1
    a.sample_buses(300, SR, 5)
    assert 0.0 < ms(a.h) < 100.0
    a.sample_buses(300, SR, 3)                                   # the room is past the call's buses: idle, no kernel
    assert ms(a.h) == 0.0
