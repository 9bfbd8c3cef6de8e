"""The per-bus chorus on the device.  Twin handles are fed the same events, one with choruses and one without; the
twin's bus output is x, what the bus combine writes, and the expectation is the numpy float32 model of the rule
(test_chorus_host.np_chorus) over x with history and phase carried from call to call (ChorusModel); behind it come the models of the
stages that follow: the delay's (test_gpu_delay.DelayModel), the reverb's (test_gpu_reverb.Model), the master section's
(test_gpu_master.Master), the limiter's (test_gpu_limiter.Lim).

Handles, events and the one-pole bank are tests/test_gpu_reverb.py's.  Every comparison is on bits with no NaN allowance
(helpers.assert_bits_equal_finite) unless a test says why it compares values."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_chorus_host import M32, check_ranges, history_frames, np_chorus
from test_gpu_buses import ubits
from test_gpu_delay import DelayModel
from test_gpu_limiter import Lim
from test_gpu_master import Master
from test_gpu_reverb import CALLS, SR, V, Model, _bank, _events, _handles, _ir, _timed
from test_master_host import np_meters

pytestmark = pytest.mark.gpu
F = np.float32
# H -> (base, depth), the base fractional: below, at and past a tile of 256 frames, and the history limit
SHAPES = {2: (1.5, 0.25), 3: (1.5, 1.0), 64: (40.5, 23.0), 65: (40.5, 24.0), 145: (96.5, 48.0), 256: (200.5, 55.25), 257: (200.5, 56.0),
          1024: (512.5, 511.0), 4096: (2000.5, 2094.5)}
VOICES = [1, 2, 3, 8]
BUSES = [1, 2, 3, 8]
INCS = [0, 89478, 1 << 31, M32]
MATRIX = [(H, VOICES[i % 4], BUSES[(i + 1) % 4]) for i, H in enumerate(sorted(SHAPES))] + [(145, 8, 8), (4096, 8, 1)]


def test_the_shapes_reach_their_histories():
    assert all(history_frames(*bd) == H == s2.chorus_history_frames(*bd) for H, bd in SHAPES.items())


class ChorusModel:
    """the choruses of a handle in numpy: per bus the parameters and the carried history [H, 2] and phase"""

    def __init__(self):
        self.c = {}
        self.changed = set()                                     # the buses whose signal the rule has changed in some call so far

    def set(self, bus, voices, base, depth, inc, spread, dry, wet):
        self.c[bus] = dict(V=voices, base=base, depth=depth, inc=inc, spread=spread, dry=dry, wet=wet,
                           hist=np.zeros((history_frames(base, depth), 2), dtype=F), phase=0)

    def expect(self, x):
        """what the chorus stage makes of a call whose combined buses are x [n_buses, N, 2]; the states of its buses move on"""
        want = x.copy()
        for b, f in self.c.items():
            if b >= x.shape[0]:
                continue                                         # idle in this call
            want[b], f["hist"], f["phase"] = np_chorus(f["V"], f["base"], f["depth"], f["inc"], f["spread"], f["dry"], f["wet"], x[b], f["hist"], f["phase"])
        return want


def _set(a, model, bus, voices, base, depth, inc, spread, dry, wet):
    a.set_bus_chorus(bus, voices, base, depth, inc, spread, dry, wet)
    assert a.get_bus_chorus(bus) == (voices, float(F(base)), float(F(depth)), inc, spread, float(F(dry)), float(F(wet)))
    model.set(bus, voices, base, depth, inc, spread, dry, wet)


def _fill(a, b, model, n, nb, what):
    """one call on both handles: the buses with a chorus against the model over the twin's, the others against the twin's.  A chorus
    must change its bus wherever the rule does: in a call in which the model's output differs from x, so does the device's (a call
    whose taps all land in a history of zeros under a dry of 1 changes nothing, by the rule); model.changed collects those buses."""
    x = b.sample_buses(n, SR, nb)
    assert np.isfinite(x).all()
    want = model.expect(x)
    got = a.sample_buses(n, SR, nb)
    assert_bits_equal_finite(got, want, what)
    for bus in range(nb):
        if bus in model.c:
            assert ubits(x[bus]).any(), "%s: bus %d is silent" % (what, bus)
            if not np.array_equal(ubits(want[bus]), ubits(x[bus])):
                assert not np.array_equal(ubits(got[bus]), ubits(x[bus])), "%s: the chorus on bus %d changes no bit" % (what, bus)
                model.changed.add(bus)
        else:
            assert_bits_equal_finite(got[bus], x[bus], "%s: bus %d, which carries no chorus" % (what, bus))
    return x, got


def _states(a, model, what):
    for bus, f in model.c.items():
        hist, phase = a.bus_chorus_state(bus)
        assert_bits_equal_finite(hist, f["hist"], "%s: history of bus %d" % (what, bus))
        assert phase == f["phase"], "%s: phase of bus %d" % (what, bus)


@pytest.mark.parametrize("H,voices,n_buses", MATRIX)
def test_chorus_is_the_rule_over_the_dry_bus(H, voices, n_buses):
    """the parity matrix: every LFO step — the later ones through the rate entry, so that phase and history go on — in calls of 1000,
    1, 16, 17 and 300 frames with the state carried: shorter than, as long as and longer than H.  The choruses sit on bus 0, on the
    call's last bus — where the voices booked past it arrive folded — and, with eight buses, on bus 6, which sounds through sends
    only; the buses between them must equal the twin's on bits."""
    a, b = _handles()
    model = ChorusModel()
    base, depth = SHAPES[H]
    buses = sorted({0, n_buses - 1} | ({6} if n_buses == 8 else set()))
    fill = 0
    for j, inc in enumerate(INCS):
        spread = (0x40000000, 0, 0x80000001, M32)[j]
        for bus in buses:
            if j == 0:
                _set(a, model, bus, voices, base, depth, inc, spread, (1.0, 0.0, 0.25)[bus % 3], 1.0 / voices)
            else:
                a.set_bus_chorus_rate(bus, inc, spread)
                model.c[bus]["inc"], model.c[bus]["spread"] = inc, spread
        for n in CALLS:
            _events((a, b), V, fill)
            _fill(a, b, model, n, n_buses, "H %d, %d voices, %d buses, phase_inc %d, fill %d of %d frames" % (H, voices, n_buses, inc, fill, n))
            fill += 1
        _states(a, model, "H %d, phase_inc %d" % (H, inc))
    # (at H = 4096 the first 1334 frames, at a standing LFO 2000.5 frames deep, read zeros alone: under a dry of 1 nothing changes yet)
    assert model.changed == set(buses), "over the twenty fills the rule has changed buses %s of %s" % (sorted(model.changed), buses)


@pytest.mark.parametrize("H", [2, 4096])
def test_a_call_of_max_frames(H):
    """calls of 8192 and 8191 frames at eight voices: thirty-two tiles per bus, the last one short"""
    a, b = _handles(max_frames=8192)
    model = ChorusModel()
    base, depth = SHAPES[H]
    _set(a, model, 0, 8, base, depth, 89478 * 3, 0x40000000, 0.5, 0.125)
    _set(a, model, 1, 8, base, depth, M32, 0x12345678, 1.0, 0.25)
    for fill, n in enumerate([8192, 8191]):
        _events((a, b), V, fill)
        _fill(a, b, model, n, 2, "H %d, fill of %d frames" % (H, n))
    _states(a, model, "H %d" % H)


def test_several_choruses_in_one_call_and_an_idle_one():
    """H = 1024 on bus 0 and H = 3 on bus 2 of three buses: bus 1 between them is the twin's; a chorus on bus 5 is idle in these
    calls, and its crafted state, read back, is unchanged"""
    a, b = _handles()
    model = ChorusModel()
    _set(a, model, 0, 3, *SHAPES[1024], 89478, 0x40000000, 1.0, 0.5)
    _set(a, model, 2, 8, *SHAPES[3], 1 << 20, 0, 0.25, 0.125)
    a.set_bus_chorus(5, 2, *SHAPES[145], 89478, 7, 1.0, 1.0)
    idle = np.random.default_rng(5).standard_normal((145, 2)).astype(F)
    a.set_bus_chorus_state(5, idle, 0xCAFEF00D)
    for fill, n in enumerate(CALLS):
        _events((a, b), V, fill)
        x, got = _fill(a, b, model, n, 3, "H 1024 and 3 on buses 0 and 2, fill %d" % fill)
        assert_bits_equal_finite(got[1], x[1], "the bus between them, fill %d" % fill)
    _states(a, model, "two choruses")
    hist, phase = a.bus_chorus_state(5)
    assert_bits_equal_finite(hist, idle, "the idle chorus's history")
    assert phase == 0xCAFEF00D and a.get_bus_chorus(5) == (2,) + SHAPES[145] + (89478, 7, 1.0, 1.0)


def test_the_top_of_the_triangle_reads_the_oldest_frame():
    """phase 2^31 and phase_inc 0: m == 1 at every frame and i = H - 1.  At H = 4096 (d = 4095, f = 0) frame 0 is the history's
    second frame, and the oldest is read and weighs nothing; at H = 4095 (d = 4094.75) a history that is zero but for its oldest
    frame gives 0.75 of it at frame 0 and nothing after — values: sums with zeros give up the sign of a zero.  Both against the model
    on bits from a crafted history."""
    for (base, depth), f in ((SHAPES[4096], 0.0), ((2000.25, 2094.5), 0.75)):
        H = history_frames(base, depth)
        a, b = _handles()
        model = ChorusModel()
        _set(a, model, 1, 1, base, depth, 0, 0, 0.0, 1.0)
        hist = np.zeros((H, 2), dtype=F)
        hist[0] = (3.0, -5.0)
        hist[1] = (0.0, 0.0) if f else (7.0, 11.0)
        a.set_bus_chorus_state(1, hist, 1 << 31)
        _events((a, b), V, 0)
        b.sample_buses(16, SR, 2)
        got = a.sample_buses(16, SR, 2)
        want0 = np.array([0.75 * 3.0, 0.75 * -5.0] if f else [7.0, 11.0], dtype=F)
        assert np.array_equal(got[1, 0], want0), (H, got[1, :2])
        assert not got[1, 1:].any()                              # (frames 1 .. 15 read history frames 1 .. 16 alone: zeros)
        crafted = (np.random.default_rng(H).standard_normal((H, 2)) * 0.25).astype(F)
        a.set_bus_chorus_state(1, crafted, 1 << 31)
        model.c[1]["hist"], model.c[1]["phase"] = crafted.copy(), 1 << 31
        for fill in range(2):
            _events((a, b), V, 1 + fill)
            _fill(a, b, model, 300, 2, "H %d from a crafted history, fill %d" % (H, fill))
        _states(a, model, "H %d, crafted" % H)
        got, phase = a.bus_chorus_state(1)
        assert phase == 1 << 31
        assert_bits_equal_finite(got[:H - 600], crafted[600:], "the untouched part of the history, moved 600 frames to the front")


def test_a_call_shorter_than_the_history():
    """H = 1024 and 4096 under calls of 1, 16 and 300 frames: after every call the state read back is the model's — old history moved
    to the front, the call's input behind it"""
    a, b = _handles()
    model = ChorusModel()
    _set(a, model, 0, 2, *SHAPES[1024], 89478 * 7, 0x40000000, 0.5, 0.5)
    _set(a, model, 1, 3, *SHAPES[4096], 89478, 0, 1.0, 0.25)
    for fill, n in enumerate([300, 1, 16, 300, 17]):
        _events((a, b), V, fill)
        x, _ = _fill(a, b, model, n, 2, "shorter than H, fill %d" % fill)
        _states(a, model, "after fill %d of %d frames" % (fill, n))
        for bus in (0, 1):
            assert_bits_equal_finite(a.bus_chorus_state(bus)[0][-n:], x[bus], "the tail of the history is the call's input")


@pytest.mark.parametrize("frames", [250, 64])
def test_events_inside_a_fill_and_sliced_rows(frames, monkeypatch):
    """note_ons at frames 16 and 48 split the call into segments and a rows buffer of 48 frames slices them further: the chorus sees
    the call as one stream"""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    a, b = _handles(max_frames=256)
    model = ChorusModel()
    _set(a, model, 0, 3, *SHAPES[145], 89478 * 50, 0x40000000, 0.25, 0.5)
    _set(a, model, 3, 8, *SHAPES[3], 1 << 24, 0, 0.0, 0.125)
    for fill in range(3):
        _events((a, b), V, fill)
        _timed((a, b), fill)
        _fill(a, b, model, frames, 4, "events at 16 and 48, slices of 48, %d frames, fill %d" % (frames, fill))
    a.L.s2r_debug_pan_slice.restype = C.c_uint32
    a.L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    assert a.L.s2r_debug_pan_slice(a.h) == 48


def test_a_send_only_bus_with_a_chorus_while_a_fader_ramps():
    """bus 6 of eight sounds through program 0's send alone and carries the chorus; program 0's fader moves across the second and
    third call — on both handles, so the twin's bus 6 is x under the same sends and ramps"""
    a, b = _handles()
    model = ChorusModel()
    _set(a, model, 6, 3, *SHAPES[257], 89478 * 2, 0x40000000, 0.25, 0.5)
    walk = [(1.0, 0.0), (0.25, 1.0), (0.7, -0.5), (0.7, -0.5)]
    for fill, n in enumerate([300, 1000, 17, 64]):
        _events((a, b), V, fill)
        for syn in (a, b):
            syn.set_program_fader(0, *walk[fill])
        _fill(a, b, model, n, 8, "send-only bus under a fader ramp, fill %d" % fill)
        f = a.get_program_fader(0)
        assert f == b.get_program_fader(0) and f[:2] == f[2:]    # committed on both


def test_every_route_on_one_handle():
    """Handle `a` walks all 24 rows of s2r_post_route's table, one call each — a bus fill, a master fill and a master fill under the
    limiter, each with every subset of chorus, delay and reverb —; its twin `b` makes a plain bus fill of the same frames every time,
    so its stems are x.  The chorus and the delay share bus 2 and the reverb sits on bus 1 of three, with a second chorus in front
    of it.  Every step's expectation is the chain of the models: chorus, delay, reverb, master section, limiter; the meters after a
    master fill are np_meters over the model's stems and master.  Everything the device returns is collected first, then compared."""
    a, b = _handles()
    ch, dl, rv, mm = ChorusModel(), DelayModel(), Model(), Master()
    ir = _ir(40, 77, True)
    steps, lims = [], []
    state = {"lim": None, "c": None, "on": (False, False, False)}

    def stages(chorus, delay, reverb):
        was = state["on"]
        if chorus != was[0]:
            if chorus:
                _set(a, ch, 2, 3, *SHAPES[145], 89478 * 20, 0x40000000, 0.5, 0.25)
                _set(a, ch, 1, 2, *SHAPES[3], 1 << 22, 5, 0.75, 0.5)
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
        y = ch.expect(x)
        if state["on"][0] and n > 1:                             # (both choruses have a dry other than 1: they change what sounds)
            assert not np.array_equal(ubits(y[2]), ubits(x[2])) and not np.array_equal(ubits(y[1]), ubits(x[1]))
        return rv.expect(dl.expect(y))

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
    frames = [257, 16, 300, 100, 1, 256, 300, 17]
    k = 0
    for kind in ("bus fill", "master fill", "master fill under the limiter"):
        if kind == "master fill under the limiter":
            state["lim"] = Lim(48, 0, state["c"])
            state["lim"].set((a,), state["c"])
            lims.append(state["lim"])
        for j, on in enumerate(combos if kind != "master fill" else combos[::-1]):
            _events((a, b), V, k)
            stages(*on)
            what = "%d: %s, chorus %s, delay %s, reverb %s" % ((k + 1, kind) + tuple("on" if o else "off" for o in on))
            n = frames[(j + k) % len(frames)]
            if kind == "bus fill":
                bus_fill(what, n)
            else:
                master_fill(what, n, stems=j % 2 == 0)
            k += 1
    assert k == 24 and len(lims) == 1 and lims[0].limited() > 0.0       # on the model, before anything is compared: the walk limits
    for what, cmp in steps:
        for name, (got, want) in cmp.items():
            assert_bits_equal_finite(got, want, "%s: %s" % (what, name))
    mm.check_committed(a)
    _states(a, ch, "after the walk")
    for bus, f in dl.d.items():
        assert_bits_equal_finite(a.bus_delay_history(bus), f["hist"], "the delay's history after the walk")


@pytest.mark.parametrize("B", [1, 255, 1000, 4095])
def test_a_plain_delay_is_the_twin_late(B):
    """no model in the loop: one voice, depth 0, a whole base B, dry 0, wet 1 is the twin's bus B frames late, across the calls'
    boundaries, whatever the LFO does.  Values, not bits: a + 0 * (bb - a) and 0 * x + t give up the sign of a zero."""
    a, b = _handles()
    a.set_bus_chorus(1, 1, float(B), 0.0, 89478 * 100, 0x40000000, 0.0, 1.0)
    stream = [np.zeros((B, 2), dtype=F)]
    at = 0
    for fill, n in enumerate(CALLS):
        _events((a, b), V, fill)
        x = b.sample_buses(n, SR, 3)
        got = a.sample_buses(n, SR, 3)
        stream.append(x[1])
        late = np.concatenate(stream, axis=0)[at:at + n]
        at += n
        assert np.isfinite(got).all() and np.abs(x[1]).max() > 0.0
        assert np.array_equal(got[1], late), "a delay of %d frames, fill %d" % (B, fill)
        assert_bits_equal_finite(got[[0, 2]], x[[0, 2]], "the buses beside it")


def test_a_base_of_one_and_a_half_is_the_mean_of_two_neighbours():
    """no model in the loop: one voice, base 1.5, depth 0, dry 0, wet 1: i = 1, f = 0.5 and y[n] = a + 0.5 * (bb - a) with a = x[n - 1]
    and bb = x[n - 2]: their mean.  As values within the rule's own rounding: fl(bb - a) is off by at most 2^-24 |bb - a|, halving is
    exact above the denormals, and the last sum is off by at most 2^-24 of its result: together at most 2^-24 (|a| + |bb|) (1 + 2^-20),
    plus 2^-149 where a denormal is halved; the mean itself is exact in double."""
    a, b = _handles()
    a.set_bus_chorus(0, 1, 1.5, 0.0, 12345, 999, 0.0, 1.0)
    stream = np.zeros((2, 2), dtype=F)
    for fill, n in enumerate([300, 17, 1000]):
        _events((a, b), V, fill)
        x = b.sample_buses(n, SR, 2)
        got = a.sample_buses(n, SR, 2)
        s = np.concatenate([stream, x[0]], axis=0).astype(np.float64)
        pa, pb = s[1:1 + n], s[0:n]
        bound = 2.0 ** -24 * (np.abs(pa) + np.abs(pb)) * (1.0 + 2.0 ** -20) + 2.0 ** -149
        err = np.abs(got[0].astype(np.float64) - (pa + pb) / 2.0)
        assert np.abs(pa).max() > 0.0 and (err <= bound).all(), "fill %d: off by %g where %g is allowed" % (fill, err.max(), bound[err.argmax()])
        stream = s[-2:].astype(F)
        assert_bits_equal_finite(got[1], x[1], "the bus beside it")


def test_half_the_wet_halves_every_sample():
    """no model in the loop: dry 0 on two handles, wet 1 and wet 0.5, everything else alike: every sample of the second is half of the
    first's, on bits — a power of two, exact while no sample is close to the denormal range, which is asserted"""
    a, b, c = _handles(n=3)
    a.set_bus_chorus(0, 3, 96.5, 48.0, 89478 * 10, 0x40000000, 0.0, 1.0)
    c.set_bus_chorus(0, 3, 96.5, 48.0, 89478 * 10, 0x40000000, 0.0, 0.5)
    for fill, n in enumerate([300, 17, 1000]):
        _events((a, b, c), V, fill)
        x, y = a.sample_buses(n, SR, 2), c.sample_buses(n, SR, 2)
        mag = np.abs(x[0].astype(np.float64))
        assert mag.max() > 0.0 and not ((mag > 0.0) & (mag < 2.0 ** -100)).any()
        assert_bits_equal_finite(y[0], x[0] * F(0.5), "wet 0.5, fill %d" % fill)
        assert_bits_equal_finite(y[1], x[1], "the bus beside it")


def test_the_rate_entry_keeps_phase_and_history():
    a, b = _handles()
    model = ChorusModel()
    _set(a, model, 1, 2, *SHAPES[145], 89478 * 30, 0x40000000, 0.5, 0.5)
    _events((a, b), V, 0)
    _fill(a, b, model, 300, 2, "before the rate changes")
    hist, phase = a.bus_chorus_state(1)
    assert ubits(hist).any() and phase == (89478 * 30 * 300) & M32
    a.set_bus_chorus_rate(1, 89478 * 3, 0x80000000)
    model.c[1]["inc"], model.c[1]["spread"] = 89478 * 3, 0x80000000
    again, phase2 = a.bus_chorus_state(1)
    assert_bits_equal_finite(again, hist, "the history under a new rate")
    assert phase2 == phase and a.get_bus_chorus(1)[3:5] == (89478 * 3, 0x80000000)
    _events((a, b), V, 1)
    _fill(a, b, model, 300, 2, "after s2r_set_bus_chorus_rate")
    _states(a, model, "after the rate changed")
    a.set_bus_chorus_mix(1, 1.0, 0.25)
    model.c[1]["dry"], model.c[1]["wet"] = 1.0, 0.25
    _states(a, model, "under a new mix")
    _fill(a, b, model, 64, 2, "after s2r_set_bus_chorus_mix")


def test_checkpoint_carries_the_state():
    """state, pans, mix, sends and the chorus's history and phase into a fresh handle with the same chorus: the next fills are equal"""
    a, b = _handles(max_frames=512)
    model = ChorusModel()
    _set(a, model, 1, 3, *SHAPES[257], 89478 * 9, 0x40000000, 0.25, 0.5)
    _events((a, b), V, 0)
    _fill(a, b, model, 200, 2, "before the checkpoint")
    hist, phase = a.bus_chorus_state(1)
    assert hist.shape == (257, 2) and ubits(hist).any() and phase == (89478 * 9 * 200) & M32
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    c = s2.Synth(V, max_frames=512, block_voices=64)
    c.set_patch_bank(_bank())
    c.import_state(state)
    c.set_voice_pans(pans)
    c.set_voice_mix(gains, buses)
    c.set_voice_sends(sends, sbuses)
    c.set_bus_chorus(1, *a.get_bus_chorus(1))
    c.set_bus_chorus_state(1, hist, phase)
    for k, n in enumerate([100, 400]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        _, got = _fill(a, b, model, n, 2, "the checkpointed handle, fill %d" % k)
        assert_bits_equal_finite(c.sample_buses(n, SR, 2), got, "the resumed handle, fill %d" % k)
    (ha, pa), (hc, pc) = a.bus_chorus_state(1), c.bus_chorus_state(1)
    assert_bits_equal_finite(hc, ha, "both histories after them")
    assert pa == pc
    _set(a, model, 1, 3, *SHAPES[257], 89478 * 9, 0x40000000, 0.25, 0.5)     # setting the chorus again zeroes its state
    hist, phase = a.bus_chorus_state(1)
    assert not ubits(hist).any() and phase == 0
    _fill(a, b, model, 64, 2, "after s2r_set_bus_chorus")


def test_refusals_removal_and_the_other_fills():
    """a fill refused before any launch — a capacity too small, too many buses, too many frames — leaves history and phase untouched, in
    a bus fill and in a master fill; a wrong history size is refused; the panned, mono and stereo fills ignore choruses; after a
    removal the bus is the twin's on bits again; a device-list handle refuses all six entries and renders on"""
    a, b = _handles(max_frames=256)
    model = ChorusModel()
    _set(a, model, 0, 3, *SHAPES[145], 89478 * 11, 0x40000000, 0.25, 0.5)
    _events((a, b), V, 0)
    _fill(a, b, model, 100, 2, "before the refusals")
    before, phase = a.bus_chorus_state(0)
    assert ubits(before).any() and phase == (89478 * 11 * 100) & M32
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

    def untouched(what):
        hist, ph = a.bus_chorus_state(0)
        assert_bits_equal_finite(hist, before, "the history " + what)
        assert ph == phase, what

    untouched("after the refused fills")
    buf = np.zeros(2 * 145 + 2, dtype=F)
    bp = buf.ctypes.data_as(s2s._f32p)
    for count in (0, 2 * 145 - 1, 2 * 145 + 1, 2 * 144):
        assert L.s2r_set_bus_chorus_state(h, 0, bp, count, 1) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_chorus_state(h, 0, bp, 2 * 145 - 1, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_chorus_state(h, 1, bp, buf.size, None) == s2s.S2R_ERR_INVALID       # no chorus there
    assert L.s2r_set_bus_chorus_state(h, 1, bp, 290, 0) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_chorus_mix(h, 1, 1.0, 1.0) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_chorus_rate(h, 1, 1, 1) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        a.set_bus_chorus_state(0, np.zeros((146, 2), dtype=F), 0)
    assert err.value.status == s2s.S2R_ERR_INVALID
    untouched("after the refused setters")
    # the other fills
    assert_bits_equal_finite(a.sample_panned(100, SR), b.sample_panned(100, SR), "panned fill beside a chorus")
    assert_bits_equal_finite(a.sample(np.empty(64, dtype=F), SR), b.sample(np.empty(64, dtype=F), SR), "mono fill beside a chorus")
    assert_bits_equal_finite(a.sample_stereo(33, SR), b.sample_stereo(33, SR), "stereo copy beside a chorus")
    untouched("after the other fills")
    _events((a, b), V, 1)
    _fill(a, b, model, 64, 2, "after the refusals and the other fills")
    # removal
    a.clear_bus_chorus(0)
    del model.c[0]
    _events((a, b), V, 2)
    x = b.sample_buses(64, SR, 2)
    assert_bits_equal_finite(a.sample_buses(64, SR, 2), x, "no chorus left: the twin's")
    # a device list
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    one = s2.Synth(512, max_frames=64, mix_groups=2)
    for syn in (multi, one):
        for v in range(512):
            syn.note_on(36 + v % 61)
    n = C.c_uint32()
    assert multi.L.s2r_set_bus_chorus(multi.h, 0, 2, 1.5, 0.25, 1, 1, 1.0, 1.0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_chorus(multi.h, 0, 0, 0.0, 0.0, 0, 0, 0.0, 0.0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_chorus_mix(multi.h, 0, 1.0, 1.0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_chorus_rate(multi.h, 0, 1, 1) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_chorus(multi.h, 0, C.byref(n), None, None, None, None, None, None) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_chorus_state(multi.h, 0, bp, buf.size, C.byref(n)) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_chorus_state(multi.h, 0, bp, 4, 0) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        multi.set_bus_chorus(0, 2, 1.5, 0.25, 1)
    assert err.value.status == s2s.S2R_ERR_INVALID
    x, y = multi.sample(np.empty(64, dtype=F), SR), one.sample(np.empty(64, dtype=F), SR)
    assert np.abs(y).max() > 0.0
    assert_bits_equal_finite(x, y, "the device-list handle after the refused chorus calls")


def test_range_checks_on_a_handle():
    check_ranges(s2.Synth(8, max_frames=64))


def test_a_handle_that_never_had_a_chorus_and_the_timing_entry():
    """s2r_debug_bus_chorus_ms: -1 without s2r_set_timing; under it 0 after a bus fill and a master fill of a handle that never had a
    chorus, whose outputs are the twin's; and the chorus kernel's time once a chorus is set"""
    a, b = _handles()
    ms = a.L.s2r_debug_bus_chorus_ms
    ms.restype, ms.argtypes = C.c_float, [C.c_void_p]
    _events((a, b), V, 0)
    assert_bits_equal_finite(a.sample_buses(300, SR, 3), b.sample_buses(300, SR, 3), "no chorus, timing off")
    assert ms(a.h) == -1.0
    a.set_timing(True)
    _events((a, b), V, 1)
    assert_bits_equal_finite(a.sample_buses(300, SR, 3), b.sample_buses(300, SR, 3), "no chorus, bus fill under timing")
    assert ms(a.h) == 0.0
    _events((a, b), V, 2)
    (ma, sa), (mb, sb) = a.sample_master(300, SR, 3), b.sample_master(300, SR, 3)
    assert_bits_equal_finite(ma, mb, "no chorus, master fill under timing")
    assert_bits_equal_finite(sa, sb, "no chorus, the stems of a master fill")
    assert ms(a.h) == 0.0
    a.set_bus_chorus(1, 3, 96.5, 48.0, 89478, 0x40000000, 1.0, 0.5)
    a.sample_buses(300, SR, 3)
    assert 0.0 < ms(a.h) < 100.0
    a.sample_buses(300, SR, 1)                                   # the chorus idle: no kernel
    assert ms(a.h) == 0.0
