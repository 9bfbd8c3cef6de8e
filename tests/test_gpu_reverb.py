"""The per-bus convolution reverb on the device.  Twin handles are fed the same events, one with reverbs and one
without; the twin's bus output is the dry signal x, and the expectation is the numpy float32 model of the rule
(test_reverb_host.np_reverb) over x with the history carried from call to call.  No oracle is in the loop.

Every mix is non-degenerate: seeds[v] = v, noise > 0, notes 36 + v % 61.  Every comparison is on bits with no NaN allowance
(helpers.assert_bits_equal_finite) unless a test says why it compares values."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite, make_patch
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_gpu_buses import VELS, _pair, ubits
from test_gpu_panned import _onepole, ON
from test_reverb_host import check_ranges, np_reverb

pytestmark = pytest.mark.gpu
SR = 48000
F = np.float32
CALLS = [1000, 1, 16, 17, 300]                                   # histories shorter and longer than a call both occur
MIXES = [(0.0, 1.0), (1.0, 0.5), (0.25, 1.0)]
V = 272
PROGRAMS = 8
MAINS = 6                                                        # programs that note_ons use


def _bank():
    """eight programs of two patches, both with the one-pole filter: a test here runs up to thirty fills on voices that are never
    all restarted, and the dry buses must stay finite that long (the LP2 patch of test_gpu_panned._bank2 grows without bound over
    some thousand frames)"""
    return [_onepole(), make_patch(osc_kind=s2.OSC_SINE, lpf_freq=900.0, noise=0.2)] * (PROGRAMS // 2)


def _ir(K, seed, stereo=False):
    rng = np.random.default_rng(seed)
    ir = (rng.standard_normal((K, 2)) * np.exp(-np.arange(K) / max(K / 3.0, 1.0))[:, None]).astype(F)
    if not stereo:
        return np.ascontiguousarray(ir[:, 0])
    assert K == 1 or not np.array_equal(ir[:, 0], ir[:, 1])
    return ir


class Model:
    """the reverbs of a handle in numpy: per bus the response, dry, wet and the carried history [K - 1, 2]"""

    def __init__(self):
        self.fx = {}

    def set(self, bus, ir, dry, wet):
        ir = np.asarray(ir, dtype=F)
        ir2 = np.stack([ir, ir], axis=1) if ir.ndim == 1 else ir
        self.fx[bus] = dict(ir=ir2, dry=dry, wet=wet, hist=np.zeros((ir2.shape[0] - 1, 2), dtype=F))

    def expect(self, x):
        """what a call returns whose dry buses are x [n_buses, N, 2]; the histories of its buses move on"""
        want = x.copy()
        n = x.shape[1]
        for b, f in self.fx.items():
            if b >= x.shape[0]:
                continue                                         # idle in this call
            line = np.concatenate([f["hist"], x[b]], axis=0)
            for c in range(2):
                want[b, :, c] = np_reverb(f["ir"][:, c], line[:, c], n, f["dry"], f["wet"])
            f["hist"] = line[line.shape[0] - (f["ir"].shape[0] - 1):].copy()
        return want


def _handles(voices=V, max_frames=1024, n=2, block=64):
    """handles with eight programs, program p booked on bus p with a pan of its own; programs 0 and 1 also send to buses 6 and 7"""
    hs = _pair(voices, block, bank=_bank(), max_frames=max_frames)
    if n == 3:
        hs.append(_pair(voices, block, bank=_bank(), max_frames=max_frames)[0])
    for syn in hs:
        for p in range(PROGRAMS):
            syn.set_program_pan(p, -0.7 + 0.2 * p, 0.5)
            syn.set_program_mix(p, 1.0 - p / 16.0, p / 8.0, p)
        syn.set_program_send(0, 0.5, 6)
        syn.set_program_send(1, 1.0 / 3.0, 7)
    return hs


def _events(handles, voices, fill):
    """the same events on every handle: fill 0 starts every voice, programs 0 .. 5 in turn (nobody is booked on buses 6 and 7: they
    sound through sends alone); later fills release two notes and restart one voice per program, so that every bus keeps sounding
    however many fills a test makes"""
    for syn in handles:
        if fill == 0:
            step = max(1, voices // 12)
            for v in range(voices):
                if v % step == 0:
                    syn.program_change((v // step) % MAINS)
                syn.note_on(36 + v % 61, VELS[(v + v // 4) % 4])
        else:
            for note in (36 + (7 * fill) % 61, 36 + (11 * fill + 3) % 61):
                syn.note_off(note)
            for p in range(MAINS):
                syn.program_change(p)
                syn.note_on(40 + (5 * p + fill) % 50, VELS[1 + (p + fill) % 3])


def _set(a, model, bus, ir, dry, wet):
    a.set_bus_reverb(bus, ir, dry, wet)
    model.set(bus, ir, dry, wet)


def _fill(a, b, model, n, nb, what, fx_buses=None):
    """one call on both handles: the buses with a reverb against the model over the twin's, the others against the twin's"""
    x = b.sample_buses(n, SR, nb)
    assert np.isfinite(x).all()
    want = model.expect(x)
    got = a.sample_buses(n, SR, nb)
    assert_bits_equal_finite(got, want, what)
    for bus in (fx_buses if fx_buses is not None else [q for q in model.fx if q < nb]):
        f = model.fx[bus]
        assert ubits(x[bus]).any(), "%s: bus %d is silent" % (what, bus)
        if f["ir"].shape[0] > 1 or (f["dry"], f["wet"]) != (0.0, 1.0):
            assert not np.array_equal(ubits(got[bus]), ubits(x[bus])), "%s: the reverb on bus %d changes no bit" % (what, bus)
    return x, got


@pytest.mark.parametrize("n_buses", [1, 2, 3, 8])
@pytest.mark.parametrize("K", [1, 255, 256, 257, 600])
def test_reverb_is_the_rule_over_the_dry_bus(K, n_buses):
    """the parity matrix: every K, a mono and a stereo response, three (dry, wet) pairs, calls of 1000, 1, 16, 17 and 300 frames.
    The reverbs sit on bus 0, on the call's last bus — where the voices booked past it arrive folded — and, with eight buses, on
    bus 6, which sounds through sends only; the buses between them must equal the twin's on bits."""
    a, b = _handles()
    model = Model()
    buses = sorted({0, n_buses - 1} | ({6} if n_buses == 8 else set()))
    fill = 0
    for stereo in (False, True):
        for dry, wet in MIXES:
            for j, bus in enumerate(buses):                      # (setting it again zeroes the history, on the device and in the model)
                _set(a, model, bus, _ir(K, 100 * K + 10 * j + stereo, stereo), dry, wet)
            for n in CALLS:
                _events((a, b), V, fill)
                _fill(a, b, model, n, n_buses, "K %d, %d buses, stereo %d, dry %g wet %g, fill %d of %d frames" % (K, n_buses, stereo, dry, wet, fill, n))
                fill += 1
    for bus in buses:                                            # the device's history is the model's
        assert_bits_equal_finite(a.bus_reverb_history(bus), model.fx[bus]["hist"], "history of bus %d" % bus)


def test_two_reverbs_of_different_lengths_in_one_call():
    a, b = _handles()
    model = Model()
    _set(a, model, 0, _ir(600, 1, True), 0.25, 1.0)
    _set(a, model, 1, _ir(255, 2), 1.0, 0.5)
    _set(a, model, 2, _ir(1, 3), 0.0, 0.5)
    for fill, n in enumerate(CALLS):
        _events((a, b), V, fill)
        _fill(a, b, model, n, 3, "K 600, 255 and 1 on three buses, fill %d" % fill)


def test_a_reverb_past_the_calls_buses_is_idle():
    """a reverb on bus 2: a call of two buses returns the twin's bits and leaves its history alone, and a later call of three buses
    goes on from that history"""
    a, b = _handles()
    model = Model()
    _set(a, model, 2, _ir(300, 4, True), 0.25, 1.0)
    _events((a, b), V, 0)
    _fill(a, b, model, 100, 3, "three buses")
    before = a.bus_reverb_history(2)
    assert ubits(before).any()
    _events((a, b), V, 1)
    x, got = _fill(a, b, model, 200, 2, "two buses: the reverb is idle", fx_buses=[])
    assert_bits_equal_finite(got, x, "two buses: the twin's")
    assert_bits_equal_finite(a.bus_reverb_history(2), before, "the idle reverb's history")
    _events((a, b), V, 2)
    _fill(a, b, model, 100, 3, "three buses again")
    assert_bits_equal_finite(a.bus_reverb_history(2), model.fx[2]["hist"], "the history after the wider call")


def test_the_longest_response():
    """K = S2R_MAX_IR_TAPS on a small pool and 64 frames: 256 segments"""
    voices = 16
    a, b = _handles(voices, max_frames=64)
    model = Model()
    _set(a, model, 0, _ir(s2.MAX_IR_TAPS, 5), 0.25, 1.0)
    for fill, n in enumerate([64, 17]):
        _events((a, b), voices, fill)
        _fill(a, b, model, n, 2, "K 65536, fill %d" % fill)


def _timed(handles, fill):
    ev = [(ON, 50 + fill, 16, 0.6), (ON, 77, 16, 1.0), (ON, 60 + fill, 48, 0.25), (ON, 90, 48, 1.0)]
    for syn in handles:
        syn.note_events(np.array(ev, dtype=s2.NOTE_EVENT_DTYPE))


@pytest.mark.parametrize("frames", [250, 64])
def test_events_inside_a_fill_and_sliced_rows(frames, monkeypatch):
    """note_ons at frames 16 and 48 split the call into segments and a rows buffer of 48 frames slices them further: the reverb sees
    the call as one stream"""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    a, b = _handles(max_frames=256)
    model = Model()
    _set(a, model, 0, _ir(300, 6, True), 0.25, 1.0)
    _set(a, model, 3, _ir(40, 7), 0.0, 1.0)
    for fill in range(3):
        _events((a, b), V, fill)
        _timed((a, b), fill)
        _fill(a, b, model, frames, 4, "events at 16 and 48, slices of 48, %d frames, fill %d" % (frames, fill))
    a.L.s2r_debug_pan_slice.restype = C.c_uint32
    a.L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    assert a.L.s2r_debug_pan_slice(a.h) == 48


def test_events_inside_a_fill():
    a, b = _handles(max_frames=256)
    model = Model()
    _set(a, model, 1, _ir(257, 8), 1.0, 0.5)
    for fill in range(2):
        _events((a, b), V, fill)
        _timed((a, b), fill)
        _fill(a, b, model, 256, 2, "events at 16 and 48, fill %d" % fill)


def test_a_send_only_bus_with_a_reverb_while_a_fader_ramps():
    """the whole chain: bus 6 of eight sounds through program 0's send alone and carries the reverb; program 0's fader moves across
    the second and third call — on both handles, so the twin's bus 6 is the dry signal under the same sends and ramps"""
    a, b = _handles()
    model = Model()
    _set(a, model, 6, _ir(600, 9, True), 0.25, 1.0)
    walk = [(1.0, 0.0), (0.25, 1.0), (0.7, -0.5), (0.7, -0.5)]
    for fill, n in enumerate([300, 1000, 17, 64]):
        _events((a, b), V, fill)
        for syn in (a, b):
            syn.set_program_fader(0, *walk[fill])
        _fill(a, b, model, n, 8, "send-only bus under a fader ramp, fill %d" % fill)
        f = a.get_program_fader(0)
        assert f == b.get_program_fader(0) and f[:2] == f[2:]    # committed on both


@pytest.mark.parametrize("D", [0, 255, 256, 300])
def test_a_unit_tap_is_a_delay(D):
    """no model in the loop: a response of D zeros and a one, dry 0, wet 1, is the twin's bus D frames late, across the calls'
    boundaries.  Values, not bits: 0 * x + r gives up the sign of a zero."""
    a, b = _handles()
    ir = np.zeros(D + 1, dtype=F)
    ir[D] = 1.0
    a.set_bus_reverb(1, ir, 0.0, 1.0)
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
    """no model in the loop: dry 0 on two handles, wet 1 and wet 0.5: every sample of the second is half of the first's — exact
    while no sample is close to the denormal range, which is asserted.  Values, not bits."""
    a, b, c = _handles(n=3)
    ir = _ir(600, 10, True)
    a.set_bus_reverb(0, ir, 0.0, 1.0)
    c.set_bus_reverb(0, ir, 0.0, 0.5)
    for fill, n in enumerate([300, 17]):
        _events((a, b, c), V, fill)
        x, y = a.sample_buses(n, SR, 2), c.sample_buses(n, SR, 2)
        mag = np.abs(x[0].astype(np.float64))
        assert mag.max() > 0.0 and not ((mag > 0.0) & (mag < 2.0 ** -100)).any()
        assert np.array_equal(y[0], x[0] * F(0.5)), "wet 0.5, fill %d" % fill
        assert_bits_equal_finite(y[1], x[1], "the bus beside it")


def test_removing_a_reverb_and_the_other_fills():
    """after n_taps = 0 the bus is the twin's on bits again; the panned, mono, stereo and oversampled fills of a handle with reverbs
    are the twin's throughout"""
    a, b = _handles()
    model = Model()
    _set(a, model, 0, _ir(257, 11), 0.25, 1.0)
    _set(a, model, 1, _ir(40, 12, True), 1.0, 0.5)
    _events((a, b), V, 0)
    _fill(a, b, model, 100, 2, "with reverbs")
    assert_bits_equal_finite(a.sample_panned(100, SR), b.sample_panned(100, SR), "panned fill beside reverbs")
    assert_bits_equal_finite(a.sample(np.empty(64, dtype=F), SR), b.sample(np.empty(64, dtype=F), SR), "mono fill beside reverbs")
    assert_bits_equal_finite(a.sample_stereo(33, SR), b.sample_stereo(33, SR), "stereo copy beside reverbs")
    assert_bits_equal_finite(a.sample_oversampled(48, SR), b.sample_oversampled(48, SR), "oversampled fill beside reverbs")
    assert_bits_equal_finite(a.bus_reverb_history(0), model.fx[0]["hist"], "the other fills leave the history alone")
    _events((a, b), V, 1)
    _fill(a, b, model, 64, 2, "with reverbs, after the other fills")
    a.clear_bus_reverb(0)
    del model.fx[0]
    _events((a, b), V, 2)
    x, got = _fill(a, b, model, 64, 2, "bus 0 without its reverb")
    assert_bits_equal_finite(got[0], x[0], "bus 0 is the twin's again")
    a.clear_bus_reverb(1)
    _events((a, b), V, 3)
    x = b.sample_buses(64, SR, 2)
    assert_bits_equal_finite(a.sample_buses(64, SR, 2), x, "no reverb left")


def test_checkpoint_carries_the_history():
    """state, pans, mix, sends and the reverb's history into a fresh handle: the next fills are equal.  s2r_set_bus_reverb_mix keeps the
    history, s2r_set_bus_reverb zeroes it."""
    a, b = _handles(max_frames=512)
    model = Model()
    ir = _ir(300, 13, True)
    _set(a, model, 1, ir, 0.25, 1.0)
    _events((a, b), V, 0)
    _fill(a, b, model, 200, 2, "before the checkpoint")
    hist = a.bus_reverb_history(1)
    assert hist.shape == (299, 2) and ubits(hist).any()
    assert_bits_equal_finite(hist, model.fx[1]["hist"], "the history read back")
    state, pans, (gains, buses), (sends, sbuses) = a.export_state(), a.voice_pans(), a.voice_mix(), a.voice_sends()
    c = s2.Synth(V, max_frames=512, block_voices=64)
    c.set_patch_bank(_bank())
    c.import_state(state)
    c.set_voice_pans(pans)
    c.set_voice_mix(gains, buses)
    c.set_voice_sends(sends, sbuses)
    c.set_bus_reverb(1, ir, *a.get_bus_reverb(1)[1:])
    c.set_bus_reverb_history(1, hist)
    for k, n in enumerate([100, 400]):
        for syn in (a, b, c):
            syn.note_off(40 + k)
        _, got = _fill(a, b, model, n, 2, "the checkpointed handle, fill %d" % k)
        assert_bits_equal_finite(c.sample_buses(n, SR, 2), got, "the resumed handle, fill %d" % k)
    # the mix keeps the history ...
    a.set_bus_reverb_mix(1, 1.0, 0.5)
    model.fx[1]["dry"], model.fx[1]["wet"] = 1.0, 0.5
    assert_bits_equal_finite(a.bus_reverb_history(1), model.fx[1]["hist"], "the history under a new mix")
    _fill(a, b, model, 64, 2, "after s2r_set_bus_reverb_mix")
    # ... and setting the reverb again zeroes it
    _set(a, model, 1, ir, 1.0, 0.5)
    assert not ubits(a.bus_reverb_history(1)).any()
    _fill(a, b, model, 64, 2, "after s2r_set_bus_reverb")


def test_refusals_leave_the_histories_alone():
    """a bus fill refused before any launch — a capacity too small, too many buses, too many frames — leaves every history untouched, a
    wrong history size is refused, and a device-list handle refuses all five entries and renders on"""
    a, b = _handles(max_frames=256)
    model = Model()
    _set(a, model, 0, _ir(300, 14), 0.25, 1.0)
    _events((a, b), V, 0)
    _fill(a, b, model, 100, 2, "before the refusals")
    before = a.bus_reverb_history(0)
    L, h = a.L, a.h
    out = np.empty(2 * 2 * 300, dtype=F)
    p = out.ctypes.data_as(s2s._f32p)
    assert L.s2r_fill_buses(h, p, 2 * 2 * 100 - 1, 2, 100, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_buses(h, p, out.size, 9, 16, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_buses(h, p, out.size, 0, 16, SR) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_buses(h, p, out.size, 2, 257, SR) == s2s.S2R_ERR_TOO_MANY_FRAMES
    assert_bits_equal_finite(a.bus_reverb_history(0), before, "the history after the refused fills")
    buf = np.zeros(2 * 299 + 2, dtype=F)
    bp = buf.ctypes.data_as(s2s._f32p)
    for count in (0, 2 * 299 - 1, 2 * 299 + 1, 2 * 300):
        assert L.s2r_set_bus_reverb_history(h, 0, bp, count) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_reverb_history(h, 0, bp, 2 * 299 - 1) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_reverb_history(h, 1, bp, buf.size) == s2s.S2R_ERR_INVALID      # no reverb there
    with pytest.raises(s2.S2rError) as err:
        a.set_bus_reverb_history(0, np.zeros((300, 2), dtype=F))
    assert err.value.status == s2s.S2R_ERR_INVALID
    assert_bits_equal_finite(a.bus_reverb_history(0), before, "the history after the refused setters")
    _events((a, b), V, 1)
    _fill(a, b, model, 64, 2, "after the refusals")
    multi = s2.Synth(512, max_frames=64, devices=[0, 0])
    one = s2.Synth(512, max_frames=64, mix_groups=2)
    for syn in (multi, one):
        for v in range(512):
            syn.note_on(36 + v % 61)
    ir = _ir(5, 15)
    irp = ir.ctypes.data_as(s2s._f32p)
    k, d, w = C.c_uint32(), C.c_float(), C.c_float()
    assert multi.L.s2r_set_bus_reverb(multi.h, 0, irp, None, 5, 0.0, 1.0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_reverb(multi.h, 0, None, None, 0, 0.0, 1.0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_reverb_mix(multi.h, 0, 0.0, 1.0) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_reverb(multi.h, 0, C.byref(k), C.byref(d), C.byref(w)) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_get_bus_reverb_history(multi.h, 0, bp, buf.size) == s2s.S2R_ERR_INVALID
    assert multi.L.s2r_set_bus_reverb_history(multi.h, 0, bp, 8) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        multi.set_bus_reverb(0, ir)
    assert err.value.status == s2s.S2R_ERR_INVALID
    x, y = multi.sample(np.empty(64, dtype=F), SR), one.sample(np.empty(64, dtype=F), SR)
    assert np.abs(y).max() > 0.0
    assert_bits_equal_finite(x, y, "the device-list handle after the refused reverb calls")


def test_range_checks_on_a_handle():
    check_ranges(s2.Synth(8, max_frames=64))
