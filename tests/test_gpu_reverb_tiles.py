"""The bus reverb where tests/test_gpu_reverb.py never takes it: calls longer than the convolve kernel's tile of
1024 frames, max_frames that the partials' and the lines' strides have to round up, responses shorter than one window load,
a response replaced by one of another length, histories that no synth voice produces, and — with no float32 model taking part —
the device against a plain float64 convolution.

The handles, the events, the model and the bank are test_gpu_reverb's (one-pole patches only, for the reason its _bank gives), on
pools of 32 voices.  Every comparison is on bits with no NaN allowance unless a test says why it compares values; the guards of
test_gpu_reverb._fill hold here too: the dry bus is not silent and the reverb changes at least one bit."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_gpu_buses import ubits
from test_gpu_panned import ON
from test_gpu_reverb import MIXES, SR, Model, _events, _fill, _handles, _ir, _set
from test_reverb_host import crafted_denormal, crafted_mixed, f64_reverb_and_bound

pytestmark = pytest.mark.gpu
F = np.float32
V = 32
TILE = 1024                                                      # kFxTile of csrc/s2r_fx.hip


def _small(max_frames):
    return _handles(V, max_frames=max_frames, block=64)


@pytest.mark.parametrize("K", [1, 5, 256, 257, 600, 1300, 2049])
def test_calls_past_one_tile(K):
    """max_frames = 2501 is odd on purpose: the partials' stride becomes 2504 and the lines' stride is rounded up as well.  The
    calls: one exactly full tile; a second tile of one frame (thread 0 takes the scalar tail, every other thread stores nothing);
    a second tile of exactly one 8-frame store; two full tiles; a third tile; frames == max_frames with an odd tail in the third
    tile; a short call whose whole history comes from the long call before it; a second tile of 7 frames, scalar tail only.
    K = 1300: the history is longer than a tile — tile 0's segments 4 and 5 read history alone, tile 1's reach through tile 0 into
    it.  K = 2049: nine segments, the last of one tap and 255 pads.  Bus 0 carries a stereo response, bus 2 — the call's last,
    where the folded voices arrive — a mono one, and bus 1 none: it is the twin's on bits."""
    a, b = _small(2501)
    model = Model()
    _set(a, model, 0, _ir(K, 7 * K, True), 0.25, 1.0)
    _set(a, model, 2, _ir(K, 7 * K + 1), 1.0, 0.5)
    for fill, n in enumerate([1024, 1025, 1032, 2048, 2049, 2501, 7, 1031]):
        _events((a, b), V, fill)
        x, got = _fill(a, b, model, n, 3, "K %d, fill %d of %d frames" % (K, fill, n))
        assert ubits(x[1]).any()
        assert_bits_equal_finite(got[1], x[1], "K %d, fill %d: the bus without a reverb" % (K, fill))
    for bus in (0, 2):
        hist = a.bus_reverb_history(bus)
        assert hist.shape == (K - 1, 2)
        assert_bits_equal_finite(hist, model.fx[bus]["hist"], "K %d: history of bus %d" % (K, bus))


def test_eight_short_responses_at_once():
    """K = 2, 3, 4, 5, 8, 9, 255 and 1 on the eight buses of one call, mono and stereo in turn: sixteen bus channels in the grid, one
    segment each, and histories shorter than the four samples a window load takes.  Buses 6 and 7 sound through sends only.
    max_frames = 1032 is a tile and one 8-frame store; the last call uses all of it bar the scalar tail's seven frames."""
    a, b = _small(1032)
    model = Model()
    for bus, K in enumerate([2, 3, 4, 5, 8, 9, 255, 1]):
        _set(a, model, bus, _ir(K, 50 + bus, bool(bus & 1)), *MIXES[bus % 3])
        assert a.bus_reverb_history(bus).shape == (K - 1, 2)
    for fill, n in enumerate([1000, 1, 17, 1025]):
        _events((a, b), V, fill)
        _fill(a, b, model, n, 8, "eight short responses, fill %d of %d frames" % (fill, n))
    for bus in range(8):
        assert_bits_equal_finite(a.bus_reverb_history(bus), model.fx[bus]["hist"], "history of bus %d" % bus)


def _crafted(ir, hist, dry, wet, sounding):
    """K = 1300 on bus 1 of two, the crafted history in front of calls of 1500 and 64 frames on handles with max_frames = 1504: each
    call against the model on bits and the history read back after it; the first call, independently of the model, against
    s2r_reverb_reference over the same line.  Returns the first call's output on the bus, [1500, 2], and the twin's."""
    K = ir.shape[0]
    assert K == 1300 and hist.shape == (K - 1, 2)
    a, b = _small(1504)
    model = Model()
    _set(a, model, 1, ir, dry, wet)
    a.set_bus_reverb_history(1, hist)
    model.fx[1]["hist"] = hist.copy()
    assert_bits_equal_finite(a.bus_reverb_history(1), hist, "the crafted history read back")
    first = None
    for fill, n in enumerate([1500, 64]):
        if sounding:
            _events((a, b), V, fill)
        x, got = _fill(a, b, model, n, 2, "crafted history, fill %d of %d frames" % (fill, n), fx_buses=[1] if sounding else [])
        assert_bits_equal_finite(a.bus_reverb_history(1), model.fx[1]["hist"], "the history after fill %d" % fill)
        if not sounding:                                         # nothing was started: the twin's buses are +0.0 in every bit
            assert not ubits(x).any(), "an idle bus is not +0.0 everywhere"
            assert_bits_equal_finite(got[0], x[0], "the bus beside it")
        if fill == 0:
            assert ubits(got[1]).any() and not np.array_equal(ubits(got[1]), ubits(x[1]))
            for c in range(2):
                line = np.concatenate([hist[:, c], x[1, :, c]])
                assert_bits_equal_finite(got[1, :, c], s2.reverb_reference(ir[:, c], line, n, dry, wet), "channel %d against s2r_reverb_reference" % c)
            first = (got[1].copy(), x[1].copy())
    return first


PARTS = ["denormals, wet 1", "denormals, wet 0.5", "mixed magnitudes on an idle bus", "mixed magnitudes under a sounding bus"]


@pytest.mark.parametrize("part", PARTS)
def test_crafted_histories(part):
    """Samples that no synth voice produces, put in front of the convolve kernel through s2r_set_bus_reverb_history (_crafted).
    Denormals: a response scaled by 2^-70 over a uniform history scaled by 2^-68, at (dry 0, wet 1) and (dry 0, wet 0.5), on a bus
    that carries nothing — no voice is started, and the twin's buses are asserted to be +0.0 in every bit.  Every product and every
    sum is a denormal, which on the device rests on the build's denormal mode and on v_pk_mul_f32 / v_pk_add_f32 keeping them; at
    wet 0.5 the mix's product rounds in the denormal range as well.  The condition is stated on the model alone and before anything
    is compared, so a flushing device cannot pass by agreeing with a flushed expectation: at least 90 % of the model's first K - 1
    frames are non-zero and below 2^-126.
    Mixed magnitudes: a response scaled by 1e-8 over a history that repeats (1e30, -1e30, 2^-126, -2^-140, -0.0, +0.0, 3.0,
    2^-149), the right channel three elements on, at (dry 0.25, wet 1): terms of 1e22 that cancel beside denormals and both zeros;
    once on a bus that carries nothing and once under a sounding bus, where crafted history and real dry samples meet inside one
    segment.  The model's output is finite, about 4e23 at most, and assert_bits_equal_finite enforces it.
    Non-finite samples stay out: DESIGN.md 4.16 puts them outside the contract, and the padded taps make the device differ from
    the rule there by design."""
    K = 1300
    if part.startswith("denormals"):
        wet = 1.0 if part.endswith("wet 1") else 0.5
        pairs = [crafted_denormal(K, 41 + c) for c in range(2)]
        ir, hist = (np.stack([p[k] for p in pairs], axis=1) for k in range(2))
        alone = Model()
        alone.set(1, ir, 0.0, wet)
        alone.fx[1]["hist"] = hist.copy()
        mag = np.abs(alone.expect(np.zeros((2, 1500, 2), dtype=F))[1, :K - 1].astype(np.float64))
        assert ((mag > 0.0) & (mag < 2.0 ** -126)).mean() >= 0.9
        _crafted(ir, hist, 0.0, wet, sounding=False)
    else:
        sounding = part.endswith("sounding bus")
        pairs = [crafted_mixed(K, 43 + c, 3 * c) for c in range(2)]
        ir, hist = (np.stack([p[k] for p in pairs], axis=1) for k in range(2))
        got, x = _crafted(ir, hist, 0.25, 1.0, sounding)
        assert np.abs(got).max() > 1e20
        assert bool(ubits(x).any()) == sounding


def test_replacing_a_response_by_another_length():
    """bus 1 of two gets K = 600, then 40, then 1300 (longer than max_frames = 512): each replacement brings new strides, a new
    segment count and new partials while the staging buffer stays, zeroes the history, and the reported K and the history's shape
    follow it.  Then a reverb on bus 0 as well, set when the staging buffer already exists, and last bus 1's reverb removed while
    bus 0 keeps its own."""
    a, b = _small(512)
    model = Model()
    fill = 0
    for K in (600, 40, 1300):
        _set(a, model, 1, _ir(K, 60 + K, K == 40), 0.25, 1.0)
        assert a.get_bus_reverb(1) == (K, 0.25, 1.0)
        hist = a.bus_reverb_history(1)
        assert hist.shape == (K - 1, 2) and not ubits(hist).any()
        for n in (300, 17):
            _events((a, b), V, fill)
            _fill(a, b, model, n, 2, "K %d on bus 1, fill %d of %d frames" % (K, fill, n))
            fill += 1
        assert_bits_equal_finite(a.bus_reverb_history(1), model.fx[1]["hist"], "history under K %d" % K)
    _set(a, model, 0, _ir(257, 70, True), 1.0, 0.5)
    _events((a, b), V, fill)
    _fill(a, b, model, 300, 2, "a second reverb on bus 0")
    fill += 1
    a.clear_bus_reverb(1)
    del model.fx[1]
    assert a.get_bus_reverb(1) == (0, 0.0, 0.0) and a.get_bus_reverb(0) == (257, 1.0, 0.5)
    for n in (17, 300):
        _events((a, b), V, fill)
        x, got = _fill(a, b, model, n, 2, "bus 1 without its reverb, %d frames" % n)
        assert ubits(x[1]).any()
        assert_bits_equal_finite(got[1], x[1], "bus 1 is the twin's again")
        fill += 1
    assert_bits_equal_finite(a.bus_reverb_history(0), model.fx[0]["hist"], "history of bus 0")


def _timed(handles, fill, frames):
    ev = [(ON, 50 + fill + 7 * k, f, v) for k, (f, v) in enumerate(zip(frames, (0.6, 1.0, 0.25, 0.8)))]
    for syn in handles:
        syn.note_events(np.array(ev, dtype=s2.NOTE_EVENT_DTYPE))


def test_events_and_slices_past_the_first_tile(monkeypatch):
    """a rows buffer of 48 frames and timed note_ons on both sides of both tile boundaries: the mixer writes a call of 2501 frames
    in about fifty slices and five event segments, and the reverb must see it as one stream.  An event's frame is a multiple of 16
    (s2r.h; frames 1023 and 2047 are refused, which is asserted), so the events beside the boundaries sit at 1008 and 2032, one
    16-frame chunk in front of those at 1024 and 2048.  The call of 1025 frames takes the two events that lie inside it."""
    monkeypatch.setenv("S2R_PAN_SLICE", "48")
    a, b = _small(2501)
    model = Model()
    _set(a, model, 0, _ir(600, 80, True), 0.25, 1.0)
    _set(a, model, 3, _ir(40, 81), 0.0, 1.0)
    for frame in (TILE - 1, 2 * TILE - 1):
        with pytest.raises(s2.S2rError) as err:
            a.note_events(np.array([(ON, 60, frame, 1.0)], dtype=s2.NOTE_EVENT_DTYPE))
        assert err.value.status == s2s.S2R_ERR_INVALID
    for fill, n in enumerate([2501, 2501, 1025]):
        _events((a, b), V, fill)
        _timed((a, b), fill, [f for f in (TILE - 16, TILE, 2 * TILE - 16, 2 * TILE) if f < n])
        _fill(a, b, model, n, 4, "events beside the tile boundaries, slices of 48, fill %d of %d frames" % (fill, n))
    for bus in (0, 3):
        assert_bits_equal_finite(a.bus_reverb_history(bus), model.fx[bus]["hist"], "history of bus %d" % bus)
    a.L.s2r_debug_pan_slice.restype = C.c_uint32
    a.L.s2r_debug_pan_slice.argtypes = [C.c_void_p]
    assert a.L.s2r_debug_pan_slice(a.h) == 48


@pytest.mark.parametrize("K", [5, 600, 2049])
def test_device_is_a_float64_convolution(K):
    """No float32 model takes part: the device's output of a call of 2501 frames, after one of 1025, against
    dry * x + wet * np.convolve(line, ir)[K - 1 : K - 1 + N] in float64 over the twin's dry bus and the history it carried, at
    (dry 0.25, wet 1), inside test_reverb_host.f64_reverb_and_bound — values, not bits, because float64 is another arithmetic.
    The bound is the worst case of sequential summation: derived, not measured, and wide — at K = 2049 the numpy model uses under
    1 % of it.  It catches a reading of the rule that device, model and reference would share (the response against the samples
    the wrong way round, a history off by a frame, dry and wet swapped), not a single dropped term; the bit comparisons of this
    file and of tests/test_gpu_reverb.py remain the sharp instrument."""
    a, b = _small(2501)
    ir = _ir(K, 90 + K, True)
    a.set_bus_reverb(0, ir, 0.25, 1.0)
    stream = [np.zeros((K - 1, 2), dtype=F)]
    for fill, n in enumerate([1025, 2501]):
        _events((a, b), V, fill)
        x = b.sample_buses(n, SR, 2)
        got = a.sample_buses(n, SR, 2)
        assert np.isfinite(x).all() and np.isfinite(got).all() and ubits(x[0]).any()
        stream.append(x[0])
        past = np.concatenate(stream, axis=0)
        line = past[past.shape[0] - (K - 1 + n):]
        for c in range(2):
            y64, bound = f64_reverb_and_bound(ir[:, c], line[:, c], n, 0.25, 1.0)
            ratio = np.abs(got[0, :, c].astype(np.float64) - y64) / bound
            print("K %d, fill %d, channel %d: largest error over the bound %.4f" % (K, fill, c, ratio.max()))
            assert ratio.max() <= 1.0, (K, fill, c, int(ratio.argmax()), float(ratio.max()))
            assert np.abs(y64).max() > 1e-3 and not np.array_equal(ubits(got[0, :, c]), ubits(x[0, :, c]))
        assert_bits_equal_finite(got[1], x[1], "the bus beside it")
