"""Aux sends, the host side: the gain of a send, held against numpy float32, and the range checks of the entry
points that need no device."""
import ctypes as C

import numpy as np

import synth2_amd as s2
from synth2_amd import synth as s2s

F = np.float32
NAN = float("nan")
_u8p = C.POINTER(C.c_uint8)
GAINS = [0.0, 2.0 ** -149, 2.0 ** -126, 0.15, 0.25, 1.0 / 3.0, 0.5 ** 0.5, 0.7, 1.0 - 2.0 ** -24, 1.0]
SENDS = [0.0, 2.0 ** -149, 0.25, 1.0 / 3.0, 0.5, 0.7, 1.0 - 2.0 ** -24, 1.0]
BAD = [(1.5, 0), (-0.25, 0), (1.0000001, 0), (-1e-9, 0), (NAN, 0), (float("inf"), 0), (-float("inf"), 3), (0.5, 8), (0.5, 255), (0.0, 8),
       (1.0, 0xffffffff)]
GOOD = [(0.0, 0), (1.0, 7), (0.5, 3), (1.0 / 3.0, 1)]


def bits(x):
    return np.asarray(x, dtype=F).view(np.uint32)


def test_send_gain_is_one_rounded_multiply():
    distinct = set()
    for g in GAINS:
        for s in SENDS:
            with np.errstate(under="ignore"):
                want = F(F(g) * F(s))
            got = F(s2.send_gain(g, s))
            assert bits(got) == bits(want), (g, s, got, want)
            assert 0.0 <= got <= F(g)
            distinct.add(int(bits(got)))
    assert len(distinct) > 30
    for g in GAINS:
        assert int(bits(F(s2.send_gain(g, 0.0)))) == 0          # send 0: +0.0, whatever the gain
        assert bits(F(s2.send_gain(g, 1.0))) == bits(F(g))       # send 1: the gain itself
    assert s2.Synth.send_gain(0.7, 0.5) == s2.send_gain(0.7, 0.5)


def _new_or_skip(**kw):
    try:
        return s2.Synth(**kw)
    except s2.S2rError as e:
        if e.status == s2s.S2R_ERR_NO_DEVICE:
            return None
        raise


def test_range_errors_and_program_bounds():
    """s2r_set_program_send looks at the values before it looks at the handle, so the range check answers without a device;
    S2R_ERR_INVALID is what no handle gets for values in range.  With a device the bank-size cases run on a real handle
    (check_ranges, also called by tests/test_gpu_sends.py)."""
    L = s2.load_library()
    for send, bus in BAD:
        assert L.s2r_set_program_send(None, 0, send, bus) == s2s.S2R_ERR_PATCH_RANGE, (send, bus)
    for send, bus in GOOD:
        assert L.s2r_set_program_send(None, 0, send, bus) == s2s.S2R_ERR_INVALID, (send, bus)
    sd, bu = C.c_float(), C.c_uint32()
    assert L.s2r_get_program_send(None, 0, C.byref(sd), C.byref(bu)) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_voice_sends(None, None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_voice_sends(None, None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_abi_version() == 4
    syn = _new_or_skip(num_voices=8, max_frames=64)
    if syn is not None:
        check_ranges(syn)


def check_ranges(syn):
    L, h = syn.L, syn.h
    assert syn.get_program_send(0) == (0.0, 0)                  # a fresh handle: the defaults
    for send, bus in BAD:
        assert L.s2r_set_program_send(h, 0, send, bus) == s2s.S2R_ERR_PATCH_RANGE, (send, bus)
        assert L.s2r_set_program_send(h, 5, send, bus) == s2s.S2R_ERR_PATCH_RANGE, (send, bus)      # the values are looked at first
    assert syn.get_program_send(0) == (0.0, 0)                  # a refused call changes nothing
    assert L.s2r_set_program_send(h, 1, 0.5, 0) == s2s.S2R_ERR_INVALID       # a bank of one
    assert L.s2r_set_program_send(h, 256, 0.5, 0) == s2s.S2R_ERR_INVALID
    sd, bu = C.c_float(), C.c_uint32()
    assert L.s2r_get_program_send(h, 1, C.byref(sd), C.byref(bu)) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_program_send(h, 0, None, None) == s2s.S2R_OK            # either pointer may be null
    syn.set_program_send(0, 0.25, 7)
    assert syn.get_program_send(0) == (0.25, 7)
    for send, bus in BAD:
        assert L.s2r_set_program_send(h, 0, send, bus) == s2s.S2R_ERR_PATCH_RANGE, (send, bus)
        assert syn.get_program_send(0) == (0.25, 7)
    # the bank grows, shrinks: survivors keep their sends, the rest come back with the defaults
    syn.set_patch_bank([s2.default_patch()] * 3)
    assert syn.get_program_send(0) == (0.25, 7) and syn.get_program_send(2) == (0.0, 0)
    syn.set_program_send(2, 0.5, 3)
    syn.set_patch_bank([s2.default_patch()] * 2)
    assert L.s2r_set_program_send(h, 2, 0.5, 0) == s2s.S2R_ERR_INVALID
    syn.set_patch_bank([s2.default_patch()] * 3)
    assert syn.get_program_send(2) == (0.0, 0) and syn.get_program_send(0) == (0.25, 7)
    n = syn.shard_voices
    before = syn.voice_sends()
    assert not bits(before[0]).any() and not before[1].any()   # never started: send +0.0, bus 0
    sends, buses = np.zeros(n, dtype=F), np.zeros(n, dtype=np.uint8)
    for bad_send, bad_bus in [(1.5, 0), (-0.5, 0), (NAN, 0), (0.5, 8), (0.5, 255)]:
        sends[:] = 0.25
        buses[:] = 2
        sends[-1], buses[-1] = bad_send, bad_bus
        assert L.s2r_set_voice_sends(h, sends.ctypes.data_as(s2s._f32p), buses.ctypes.data_as(_u8p)) == s2s.S2R_ERR_PATCH_RANGE
        got = syn.voice_sends()
        assert not bits(got[0]).any() and not got[1].any()     # nothing was changed
    assert L.s2r_set_voice_sends(h, sends.ctypes.data_as(s2s._f32p), None) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_voice_sends(h, None, buses.ctypes.data_as(_u8p)) == s2s.S2R_ERR_INVALID
    sends[:] = np.linspace(0, 1, n, dtype=F)
    buses[:] = np.arange(n) % 8
    syn.set_voice_sends(sends, buses)
    got = syn.voice_sends()
    assert np.array_equal(bits(got[0]), bits(sends)) and np.array_equal(got[1], buses)
