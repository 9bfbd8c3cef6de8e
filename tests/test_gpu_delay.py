"""The per-bus feedback delay on the device.  Twin handles are fed the same events, one with delays and one without;
the twin's bus output is x, what the bus combine writes, and the expectation is the numpy float32 model of the rule
(test_delay_host.np_delay) over x with the history carried from call to call (DelayModel); behind it come the models of the stages
that follow: the reverb's (test_gpu_reverb.Model), the master section's (test_gpu_master.Master), the limiter's (test_gpu_limiter.Lim).

Handles, events and the one-pole bank are tests/test_gpu_reverb.py's.  Every comparison is on bits with no NaN allowance
(helpers.assert_bits_equal_finite) unless a test says why it compares values."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_delay_host import FEEDS, check_ranges, np_delay
from test_gpu_buses import ubits
from test_gpu_limiter import Lim
from test_gpu_master import Master
from test_gpu_reverb import CALLS, SR, V, Model, _bank, _events, _handles, _ir, _timed
from test_master_host import np_meters

pytestmark = pytest.mark.gpu
F = np.float32
DELAYS = [1, 2, 63, 64, 65, 255, 256, 257, 999, 1000, 1001, 1024, 1025, 4096]
BUSES = [1, 2, 3, 8]
# every D with one bus count in turn, and D = 65 and 1000 — a call shorter, one longer than the delay — with all four
MATRIX = sorted({(D, BUSES[i % 4]) for i, D in enumerate(DELAYS)} | {(D, nb) for D in (65, 1000) for nb in BUSES})


class DelayModel:
    """the delays of a handle in numpy: per bus the time, the four levels and the carried history [D, 2]"""

    def __init__(self):
        self.d = {}

    def set(self, bus, D, feedback, cross, dry, wet):
        self.d[bus] = dict(D=D, mix=(feedback, cross, dry, wet), hist=np.zeros((D, 2), dtype=F))

    def expect(self, x):
        """what the delay stage makes of a call whose combined buses are x [n_buses, N, 2]; the histories of its buses move on"""
        want = x.copy()
        for b, f in self.d.items():
            if b >= x.shape[0]:
                continue                                         # idle in this call
            want[b], f["hist"] = np_delay(f["D"], *f["mix"], x[b], f["hist"])
        return want


def _set(a, model, bus, D, feedback, cross, dry, wet):
    a.set_bus_delay(bus, D, feedback, cross, dry, wet)
    assert a.get_bus_delay(bus) == (D,) + tuple(float(F(v)) for v in (feedback, cross, dry, wet))
    model.set(bus, D, feedback, cross, dry, wet)


def _fill(a, b, model, n, nb, what, changed=None):
    """one call on both handles: the buses with a delay against the model over the twin's, the others against the twin's.  A delay
    must change its bus wherever the rule makes it: with a dry other than 1, or where the call reads a frame of the line that is
    not zero."""
    x = b.sample_buses(n, SR, nb)
    assert np.isfinite(x).all()
    if changed is None:
        changed = [q for q, f in model.d.items() if q < nb and (f["mix"][2] != 1.0 or ubits(f["hist"][:min(n, f["D"])]).any())]
    want = model.expect(x)
    got = a.sample_buses(n, SR, nb)
    assert_bits_equal_finite(got, want, what)
    for bus in changed:
        assert ubits(x[bus]).any(), "%s: bus %d is silent" % (what, bus)
        assert not np.array_equal(ubits(got[bus]), ubits(x[bus])), "%s: the delay on bus %d changes no bit" % (what, bus)
    return x, got


def _histories(a, model, what):
    for bus, f in model.d.items():
        assert_bits_equal_finite(a.bus_delay_history(bus), f["hist"], "%s: history of bus %d" % (what, bus))


@pytest.mark.parametrize("D,n_buses", MATRIX)
def test_delay_is_the_rule_over_the_dry_bus(D, n_buses):
    """the parity matrix: every (feedback, cross) pair of the host test, calls of 1000, 1, 16, 17 and 300 frames with the history
    carried — shorter than, as long as and longer than D, and no multiple of it.  The delays sit on bus 0, on the call's last bus —
    where the voices booked past it arrive folded — and, with eight buses, on bus 6, which sounds through sends only; the buses
    between them must equal the twin's on bits."""
    a, b = _handles()
    model = DelayModel()
    buses = sorted({0, n_buses - 1} | ({6} if n_buses == 8 else set()))
    fill = 0
    for j, (fb, cr) in enumerate(FEEDS):
        dry, wet = ((1.0, 0.5), (0.0, 1.0), (0.25, 1.0))[j % 3]
        for bus in buses:                                        # (the later pairs through the mix entry: the line goes on, past the longest D)
            if j == 0:
                _set(a, model, bus, D, fb, cr, dry, wet)
            else:
                a.set_bus_delay_mix(bus, fb, cr, dry, wet)
                model.d[bus]["mix"] = (fb, cr, dry, wet)
        for n in CALLS:
            _events((a, b), V, fill)
            _fill(a, b, model, n, n_buses, "D %d, %d buses, feedback %g cross %g dry %g wet %g, fill %d of %d frames" % (D, n_buses, fb, cr, dry, wet, fill, n))
            fill += 1
        _histories(a, model, "D %d, feedback %g cross %g" % (D, fb, cr))


@pytest.mark.parametrize("D", [1, 3, 64, 100])
def test_a_call_many_times_the_delay(D):
    """calls of 8192 and 8191 frames: a thread walks up to 8192 steps, through whole groups of loads issued ahead and the rest behind
    them"""
    a, b = _handles(max_frames=8192)
    model = DelayModel()
    _set(a, model, 0, D, 0.6, -float(F(1.0) - F(0.6)), 0.5, 1.0)
    _set(a, model, 1, D, 0.9, 0.0, 1.0, 0.25)
    for fill, n in enumerate([8192, 8191]):
        _events((a, b), V, fill)
        _fill(a, b, model, n, 2, "D %d, fill of %d frames" % (D, n))
    _histories(a, model, "D %d" % D)


def test_several_delays_in_one_call_and_an_idle_one():
    """D = 1000 on bus 0 and D = 37 on bus 2 of three buses: bus 1 between them is the twin's; a delay on bus 5 is idle in these
    calls, and its crafted history, read back, is unchanged"""
    a, b = _handles()
    model = DelayModel()
    _set(a, model, 0, 1000, 0.5, 0.5, 1.0, 1.0)
    _set(a, model, 2, 37, -0.75, 0.25, 0.25, 1.0)
    a.set_bus_delay(5, 300, 0.5, 0.0, 1.0, 1.0)
    idle = np.random.default_rng(5).standard_normal((300, 2)).astype(F)
    a.set_bus_delay_history(5, idle)
    for fill, n in enumerate(CALLS):
        _events((a, b), V, fill)
        x, got = _fill(a, b, model, n, 3, "D 1000 and 37 on buses 0 and 2, fill %d" % fill)
        assert_bits_equal_finite(got[1], x[1], "the bus between them, fill %d" % fill)
    _histories(a, model, "two delays")
    assert_bits_equal_finite(a.bus_delay_history(5), idle, "the idle delay's history")
    assert a.get_bus_delay(5) == (300, 0.5, 0.0, 1.0, 1.0)


def test_the_longest_delay():
    """D = S2R_MAX_DELAY_FRAMES from a crafted history, two calls of 1024 frames: the outputs are the model's and so is the whole
    history read back — 262 144 - 1024 frames of it moved to the front untouched by each call"""
    D = s2.MAX_DELAY_FRAMES
    a, b = _handles()
    model = DelayModel()
    _set(a, model, 1, D, 0.5, -0.5, 0.5, 1.0)
    hist = (np.random.default_rng(6).standard_normal((D, 2)) * 0.25).astype(F)
    a.set_bus_delay_history(1, hist)
    model.d[1]["hist"] = hist.copy()
    for fill in range(2):
        _events((a, b), V, fill)
        _fill(a, b, model, 1024, 2, "D %d, fill %d" % (D, fill))
    got = a.bus_delay_history(1)
    assert_bits_equal_finite(got, model.d[1]["hist"], "the whole history")
    assert_bits_equal_finite(got[:D - 2048], hist[2048:], "the untouched part of the history, moved 2048 frames to the front")


@pytest.mark.parametrize("frames", [250, 64])
def test_events_inside_a_fill_and_sliced_rows(frames, monkeypatch):
    """note_ons at frames 16 and 48 split the call into segments and a rows buffer of 48 frames slices them further: the delay sees the
    call as one stream"""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    a, b = _handles(max_frames=256)
    model = DelayModel()
    _set(a, model, 0, 100, 0.6, -float(F(1.0) - F(0.6)), 0.25, 1.0)
    _set(a, model, 3, 7, 0.0, 1.0, 0.0, 1.0)
    for fill in range(3):
        _events((a, b), V, fill)
        _timed((a, b), fill)
        _fill(a, b, model, frames, 4, "events at 16 and 48, slices of 48, %d frames, fill %d" % (frames, fill))
    a.L.s2r_debug_pan_slice.restype = C.c_uint32
    a.L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    assert a.L.s2r_debug_pan_slice(a.h) == 48


def test_a_send_only_bus_with_a_delay_while_a_fader_ramps():
    """bus 6 of eight sounds through program 0's send alone and carries the delay; program 0's fader moves across the second and third
    call — on both handles, so the twin's bus 6 is x under the same sends and ramps"""
    a, b = _handles()
    model = DelayModel()
    _set(a, model, 6, 480, 0.5, 0.5, 0.25, 1.0)
    walk = [(1.0, 0.0), (0.25, 1.0), (0.7, -0.5), (0.7, -0.5)]
    for fill, n in enumerate([300, 1000, 17, 64]):
        _events((a, b), V, fill)
        for syn in (a, b):
            syn.set_program_fader(0, *walk[fill])
        _fill(a, b, model, n, 8, "send-only bus under a fader ramp, fill %d" % fill)
        f = a.get_program_fader(0)
        assert f == b.get_program_fader(0) and f[:2] == f[2:]    # committed on both


def test_delay_and_reverb():
    """a delay and a reverb on bus 1: the reverb's dry signal is the delay's output; bus 6 carries a delay alone and bus 7 a reverb
    alone in the same calls"""
    a, b = _handles()
    dl, rv = DelayModel(), Model()
    _set(a, dl, 1, 300, 0.5, -0.25, 0.5, 1.0)
    _set(a, dl, 6, 64, 0.0, 1.0, 1.0, 1.0)
    for bus, ir in ((1, _ir(257, 21, True)), (7, _ir(40, 22))):
        a.set_bus_reverb(bus, ir, 0.25, 1.0)
        rv.set(bus, ir, 0.25, 1.0)
    for fill, n in enumerate(CALLS):
        _events((a, b), V, fill)
        x = b.sample_buses(n, SR, 8)
        y = dl.expect(x)
        want = rv.expect(y)
        assert not np.array_equal(ubits(y[1]), ubits(x[1])) and not np.array_equal(ubits(want[1]), ubits(y[1]))
        assert_bits_equal_finite(a.sample_buses(n, SR, 8), want, "delay in front of a reverb, fill %d" % fill)
    _histories(a, dl, "in front of a reverb")
    for bus in (1, 7):
        assert_bits_equal_finite(a.bus_reverb_history(bus), rv.fx[bus]["hist"], "the reverb's history on bus %d" % bus)


def test_every_route_on_one_handle():
    """Handle `a` walks fifteen configurations, one call each; its twin `b` makes a plain bus fill of the same frames every time, so
    its stems are x.  The delay sits on bus 2 and the reverb on bus 1 of three: a call of two buses leaves the delay idle with its
    history kept (steps 4 and 9: a route without the delay between two with it), removing and setting it starts it afresh.  Every
    step's expectation is the chain of the models: delay, reverb, master section, limiter; the meters after a master fill are
    np_meters over the model's stems and master.  Everything the device returns is collected first, then compared on bits."""
    a, b = _handles()
    dl, rv, mm = DelayModel(), Model(), Master()
    ir = _ir(40, 77, True)
    steps, lims = [], []
    state = {"lim": None, "c": None}

    def delay(on):
        if on:
            _set(a, dl, 2, 200, 0.5, -0.5, 0.5, 1.0)
        else:
            a.clear_bus_delay(2)
            del dl.d[2]

    def reverb(on):
        if on:
            a.set_bus_reverb(1, ir, 0.25, 1.0)
            rv.set(1, ir, 0.25, 1.0)
        else:
            a.clear_bus_reverb(1)
            del rv.fx[1]

    def limiter(on):
        if on:
            state["lim"] = Lim(48, 0, state["c"])
            state["lim"].set((a,), state["c"])
            lims.append(state["lim"])
        else:
            a.clear_master_limiter()
            state["lim"] = None

    def bus_fill(what, n, nb=3):
        y = rv.expect(dl.expect(b.sample_buses(n, SR, nb)))
        steps.append((what, {"buses": (a.sample_buses(n, SR, nb), y)}))

    def master_fill(what, n, stems, nb=3):
        y = rv.expect(dl.expect(b.sample_buses(n, SR, nb)))
        m = mm.expect(y)
        if state["c"] is None:
            state["c"] = float(np.abs(m).max()) / 2.0            # the ceiling of every limiter below: half the first master's peak
        want = state["lim"].expect(m)[0] if state["lim"] else m
        got, st = a.sample_master(n, SR, nb, stems=stems)
        peak, energy = a.meters()
        wp, we = np_meters(y, m)
        cmp = {"master": (got, want), "peaks": (peak, wp), "energies": (energy, we)}
        if stems:
            cmp["stems"] = (st, y)
        steps.append((what, cmp))

    frames = [257, 16, 300, 257, 1, 256, 300, 17, 257, 300, 64, 257, 300, 100, 257]
    for k, n in enumerate(frames):
        _events((a, b), V, k)
        if k == 0:
            bus_fill("1: bus fill, plain", n)
        elif k == 1:
            delay(True)
            bus_fill("2: bus fill, delay", n)
        elif k == 2:
            reverb(True)
            bus_fill("3: bus fill, delay and reverb", n)
        elif k == 3:
            bus_fill("4: bus fill of two buses: reverb, the delay idle", n, nb=2)
        elif k == 4:
            master_fill("5: master fill with stems, delay and reverb, from the history of step 3", n, True)
        elif k == 5:
            limiter(True)
            master_fill("6: master fill with stems, delay, reverb and limiter", n, True)
        elif k == 6:
            reverb(False)
            master_fill("7: master fill without stems, delay and limiter", n, False)
        elif k == 7:
            bus_fill("8: bus fill, delay; the limiter set but idle", n)
        elif k == 8:
            master_fill("9: master fill of two buses with stems, limiter; the delay idle", n, True, nb=2)
        elif k == 9:
            mm.ret((a,), 2, 0.5)
            mm.fader((a,), 0.7)
            master_fill("10: master fill with stems, delay and limiter, a return and the master fader on their way", n, True)
        elif k == 10:
            delay(False)
            reverb(True)
            master_fill("11: master fill with stems, reverb and limiter, the delay removed", n, True)
        elif k == 11:
            limiter(False)
            master_fill("12: master fill without stems, reverb", n, False)
        elif k == 12:
            reverb(False)
            master_fill("13: master fill with stems, plain", n, True)
        elif k == 13:
            delay(True)
            master_fill("14: master fill with stems, the delay afresh", n, True)
        else:
            reverb(True)
            bus_fill("15: bus fill, delay and reverb", n)
    assert len(lims) == 1 and lims[0].limited() > 0.0            # on the model, before anything is compared: the walk limits
    for what, cmp in steps:
        for name, (got, want) in cmp.items():
            assert_bits_equal_finite(got, want, "%s: %s" % (what, name))
    mm.check_committed(a)
    _histories(a, dl, "after the walk")


@pytest.mark.parametrize("D", [1, 255, 1000, 1025])
def test_a_plain_delay_is_the_twin_late(D):
    """no model in the loop: feedback 0, cross 0, dry 0, wet 1 is the twin's bus D frames late, across the calls' boundaries.
    Values, not bits: 0 * x + t gives up the sign of a zero."""
    a, b = _handles()
    a.set_bus_delay(1, D, 0.0, 0.0, 0.0, 1.0)
    stream = [np.zeros((D, 2), dtype=F)]
    at = 0
    for fill, n in enumerate(CALLS):
        _events((a, b), V, fill)
        x = b.sample_buses(n, SR, 3)
        got = a.sample_buses(n, SR, 3)
        stream.append(x[1])
        late = np.concatenate(stream, axis=0)[at:at + n]
        at += n
        assert np.isfinite(got).all() and np.abs(x[1]).max() > 0.0
        assert np.array_equal(got[1], late), "a delay of %d frames, fill %d" % (D, fill)
        assert_bits_equal_finite(got[[0, 2]], x[[0, 2]], "the buses beside it")


def test_half_the_wet_halves_every_sample():
    """no model in the loop: dry 0 on two handles, wet 1 and wet 0.5, feedback and cross alike: every sample of the second is half of
    the first's, on bits — a power of two, exact while no sample is close to the denormal range, which is asserted"""
    a, b, c = _handles(n=3)
    a.set_bus_delay(0, 100, 0.5, -0.5, 0.0, 1.0)
    c.set_bus_delay(0, 100, 0.5, -0.5, 0.0, 0.5)
    for fill, n in enumerate([300, 17, 1000]):
        _events((a, b, c), V, fill)
        x, y = a.sample_buses(n, SR, 2), c.sample_buses(n, SR, 2)
        mag = np.abs(x[0].astype(np.float64))
        assert mag.max() > 0.0 and not ((mag > 0.0) & (mag < 2.0 ** -100)).any()
        assert_bits_equal_finite(y[0], x[0] * F(0.5), "wet 0.5, fill %d" % fill)
        assert_bits_equal_finite(y[1], x[1], "the bus beside it")


def test_cross_feed_swaps_the_channels_per_repeat():
    """no model in the loop: program 0, alone on bus 0, panned hard left; cross 1, feedback 0, dry 0, wet 1 and D = 400 over one call
    of 1000 frames: the first repeat is the left input 400 frames late on the LEFT, the second the same 800 frames late on the
    RIGHT, and before them there is nothing.  Values: x + 0.0 keeps every value and gives up the sign of a zero."""
    D, n = 400, 1000
    a, b = _handles()
    for syn in (a, b):
        syn.set_program_pan(0, -1.0, 0.0)
    a.set_bus_delay(0, D, 0.0, 1.0, 0.0, 1.0)
    _events((a, b), V, 0)
    x = b.sample_buses(n, SR, 2)[0]
    got = a.sample_buses(n, SR, 2)[0]
    assert np.abs(x[:, 0]).max() > 0.0 and not x[:, 1].any()     # hard left: nothing on the right
    assert not got[:D, 0].any() and np.array_equal(got[D:, 0], x[:n - D, 0])
    assert not got[:2 * D, 1].any() and np.array_equal(got[2 * D:, 1], x[:n - 2 * D, 0])
    assert np.abs(got[2 * D:, 1]).max() > 0.0


def test_checkpoint_carries_the_history():
    """state, pans, mix, sends and the delay's history into a fresh handle with the same delay: the next fills are equal"""
    a, b = _handles(max_frames=512)
    model = DelayModel()
    _set(a, model, 1, 300, 0.6, -float(F(1.0) - F(0.6)), 0.25, 1.0)
    _events((a, b), V, 0)
    _fill(a, b, model, 200, 2, "before the checkpoint")
    hist = a.bus_delay_history(1)
    assert hist.shape == (300, 2) and ubits(hist).any()
    assert_bits_equal_finite(hist, model.d[1]["hist"], "the history read back")
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    c = s2.Synth(V, max_frames=512, block_voices=64)
    c.set_patch_bank(_bank())
    c.import_state(state)
    c.set_voice_pans(pans)
    c.set_voice_mix(gains, buses)
    c.set_voice_sends(sends, sbuses)
    c.set_bus_delay(1, *a.get_bus_delay(1))
    c.set_bus_delay_history(1, hist)
    for k, n in enumerate([100, 400]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        _, got = _fill(a, b, model, n, 2, "the checkpointed handle, fill %d" % k)
        assert_bits_equal_finite(c.sample_buses(n, SR, 2), got, "the resumed handle, fill %d" % k)
    assert_bits_equal_finite(c.bus_delay_history(1), a.bus_delay_history(1), "both histories after them")
    # the mix keeps the history ...
    a.set_bus_delay_mix(1, -0.5, 0.5, 1.0, 0.5)
    model.d[1]["mix"] = (-0.5, 0.5, 1.0, 0.5)
    assert_bits_equal_finite(a.bus_delay_history(1), model.d[1]["hist"], "the history under a new mix")
    _fill(a, b, model, 64, 2, "after s2r_set_bus_delay_mix")
    # ... and setting the delay again zeroes it
    _set(a, model, 1, 300, -0.5, 0.5, 1.0, 0.5)
    assert not ubits(a.bus_delay_history(1)).any()
    _fill(a, b, model, 64, 2, "after s2r_set_bus_delay")


def test_refusals_removal_and_the_other_fills():
    """a fill refused before any launch — a capacity too small, too many buses, too many frames — leaves every history untouched, in a
    bus fill and in a master fill; a wrong history size is refused; the panned, mono and stereo fills ignore delays; after a removal
    the bus is the twin's on bits again; a device-list handle refuses all five entries and renders on"""
    a, b = _handles(max_frames=256)
    model = DelayModel()
    _set(a, model, 0, 300, 0.5, 0.5, 0.25, 1.0)
    _events((a, b), V, 0)
    _fill(a, b, model, 100, 2, "before the refusals")
    before = a.bus_delay_history(0)
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
    assert_bits_equal_finite(a.bus_delay_history(0), before, "the history after the refused fills")
    buf = np.zeros(2 * 300 + 2, dtype=F)
    bp = buf.ctypes.data_as(s2s._f32p)
    for count in (0, 2 * 300 - 1, 2 * 300 + 1, 2 * 299):
        assert L.s2r_set_bus_delay_history(h, 0, bp, count) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_delay_history(h, 0, bp, 2 * 300 - 1) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_delay_history(h, 1, bp, buf.size) == s2s.S2R_ERR_INVALID       # no delay there
    assert L.s2r_set_bus_delay_history(h, 1, bp, 600) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_delay_mix(h, 1, 0.5, 0.5, 1.0, 1.0) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        a.set_bus_delay_history(0, np.zeros((301, 2), dtype=F))
    assert err.value.status == s2s.S2R_ERR_INVALID
    assert_bits_equal_finite(a.bus_delay_history(0), before, "the history after the refused setters")
    # the other fills
    assert_bits_equal_finite(a.sample_panned(100, SR), b.sample_panned(100, SR), "panned fill beside a delay")
    assert_bits_equal_finite(a.sample(np.empty(64, dtype=F), SR), b.sample(np.empty(64, dtype=F), SR), "mono fill beside a delay")
    assert_bits_equal_finite(a.sample_stereo(33, SR), b.sample_stereo(33, SR), "stereo copy beside a delay")
    assert_bits_equal_finite(a.bus_delay_history(0), before, "the other fills leave the history alone")
    _events((a, b), V, 1)
    _fill(a, b, model, 64, 2, "after the refusals and the other fills")
    # removal
    a.clear_bus_delay(0)
    del model.d[0]
    _events((a, b), V, 2)
    x = b.sample_buses(64, SR, 2)
    assert_bits_equal_finite(a.sample_buses(64, SR, 2), x, "no delay left: the twin's")
    # a device list
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    one = s2.Synth(512, max_frames=64, mix_groups=2)
    for syn in (multi, one):
        for v in range(512):
            syn.note_on(36 + v % 61)
    n = C.c_uint32()
    assert multi.L.s2r_set_bus_delay(multi.h, 0, 5, 0.5, 0.5, 1.0, 1.0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_delay(multi.h, 0, 0, 0.0, 0.0, 0.0, 0.0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_delay_mix(multi.h, 0, 0.5, 0.5, 1.0, 1.0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_delay(multi.h, 0, C.byref(n), None, None, None, None) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_delay_history(multi.h, 0, bp, buf.size) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_delay_history(multi.h, 0, bp, 10) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        multi.set_bus_delay(0, 5)
    assert err.value.status == s2s.S2R_ERR_INVALID
    x, y = multi.sample(np.empty(64, dtype=F), SR), one.sample(np.empty(64, dtype=F), SR)
    assert np.abs(y).max() > 0.0
    assert_bits_equal_finite(x, y, "the device-list handle after the refused delay calls")


def test_range_checks_on_a_handle():
    check_ranges(s2.Synth(8, max_frames=64))


def test_a_handle_that_never_had_a_delay_and_the_timing_entry():
    """s2r_debug_bus_delay_ms: -1 without s2r_set_timing; under it 0 after a bus fill and a master fill of a handle that never had a
    delay, whose outputs are the twin's; and the delay kernel's time once a delay is set"""
    a, b = _handles()
    ms = a.L.s2r_debug_bus_delay_ms
    ms.restype, ms.argtypes = C.c_float, [C.c_void_p]
    _events((a, b), V, 0)
    assert_bits_equal_finite(a.sample_buses(300, SR, 3), b.sample_buses(300, SR, 3), "no delay, timing off")
    assert ms(a.h) == -1.0
    a.set_timing(True)
    _events((a, b), V, 1)
    assert_bits_equal_finite(a.sample_buses(300, SR, 3), b.sample_buses(300, SR, 3), "no delay, bus fill under timing")
    assert ms(a.h) == 0.0
    _events((a, b), V, 2)
    (ma, sa), (mb, sb) = a.sample_master(300, SR, 3), b.sample_master(300, SR, 3)
    assert_bits_equal_finite(ma, mb, "no delay, master fill under timing")
    assert_bits_equal_finite(sa, sb, "no delay, the stems of a master fill")
    assert ms(a.h) == 0.0
    a.set_bus_delay(1, 100, 0.5, 0.5, 1.0, 1.0)
    a.sample_buses(300, SR, 3)
    assert 0.0 < ms(a.h) < 100.0
    a.sample_buses(300, SR, 1)                                   # the delay idle: no kernel
    assert ms(a.h) == 0.0
