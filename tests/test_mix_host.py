"""The voice mixer, the host side: the gain a note_on gives its voice, held against a numpy float32 restatement
of its four lines, and the range checks of the entry points that need no device."""
import ctypes as C

import numpy as np

import synth2_amd as s2
from synth2_amd import synth as s2s

F = np.float32
LEVELS = [0.0, 0.25, 1.0 / 3.0, 0.7, 1.0]
VELOCITIES = [-1.0, -0.0, 0.0, 2.0 ** -149, 0.25, 0.6, 1.0 - 2.0 ** -24, 1.0, 1.5, float("inf"), float("nan")]
_u8p = C.POINTER(C.c_uint8)


def np_voice_gain(level, sens, velocity):
    """u = velocity < 1 ? velocity : 1 (NaN -> 1); u = u > 0 ? u : 0; a = 1 - sens * (1 - u); w = level * a — binary32, every
    operation rounded on its own"""
    v = F(velocity)
    u = v if v < F(1.0) else F(1.0)
    u = u if u > F(0.0) else F(0.0)
    with np.errstate(all="ignore"):
        a = F(F(1.0) - F(F(sens) * F(F(1.0) - u)))
        return F(F(level) * a)


def bits(x):
    return np.asarray(x, dtype=F).view(np.uint32)


def test_voice_gain_is_the_formula():
    distinct = set()
    for level in LEVELS:
        for sens in LEVELS:
            for vel in VELOCITIES:
                want = np_voice_gain(level, sens, vel)
                got = F(s2.voice_gain(level, sens, vel))
                assert bits(got) == bits(want), (level, sens, vel, got, want)
                assert 0.0 <= got <= 1.0
                distinct.add(int(bits(got)))
    assert len(distinct) > 40                                   # the grid is not a table of zeros and ones


def test_defaults_give_exactly_one():
    one = int(bits(F(1.0)))
    for vel in VELOCITIES + [1e-30, 0.999, 3.0e38, -float("inf")]:
        assert int(bits(F(s2.voice_gain(1.0, 0.0, vel)))) == one, vel


def test_full_sensitivity_at_velocity_zero_is_plus_zero():
    for level in LEVELS:
        for vel in (0.0, -0.0, -1.0):
            assert int(bits(F(s2.voice_gain(level, 1.0, vel)))) == 0, (level, vel)
    # and full velocity leaves the level alone, whatever the sensitivity
    for level in LEVELS:
        for sens in LEVELS:
            assert bits(F(s2.voice_gain(level, sens, 1.0))) == bits(F(level))


def _new_or_skip(**kw):
    try:
        return s2.Synth(**kw)
    except s2.S2rError as e:
        if e.status == s2s.S2R_ERR_NO_DEVICE:
            return None
        raise


NAN = float("nan")
BAD = [(1.5, 0.0, 0), (-0.25, 0.0, 0), (1.0000001, 0.0, 0), (1.0, 1.0000001, 0), (1.0, -1e-9, 0), (NAN, 0.0, 0), (1.0, NAN, 0),
       (float("inf"), 0.0, 0), (1.0, 0.0, 8), (1.0, 0.0, 255), (0.5, 0.5, 0xffffffff)]


def test_range_errors_and_program_bounds():
    """s2r_set_program_mix looks at the values before it looks at the handle, so the range check answers without a device;
    S2R_ERR_INVALID is what no handle gets for values in range.  With a device the bank-size cases run on a real handle
    (check_ranges, also called by tests/test_gpu_buses.py)."""
    L = s2.load_library()
    for level, sens, bus in BAD:
        assert L.s2r_set_program_mix(None, 0, level, sens, bus) == s2s.S2R_ERR_PATCH_RANGE, (level, sens, bus)
    for level, sens, bus in [(1.0, 0.0, 0), (0.0, 1.0, 7), (0.5, 0.5, 3)]:
        assert L.s2r_set_program_mix(None, 0, level, sens, bus) == s2s.S2R_ERR_INVALID
    lv, se, bu = C.c_float(), C.c_float(), C.c_uint32()
    assert L.s2r_get_program_mix(None, 0, C.byref(lv), C.byref(se), C.byref(bu)) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_voice_mix(None, None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_voice_mix(None, None, None) == s2s.S2R_ERR_INVALID
    for n_buses in (0, 1, 8, 9):
        assert L.s2r_fill_buses(None, None, 0, n_buses, 16, 48000) == s2s.S2R_ERR_INVALID
    assert s2.MAX_BUSES == 8
    syn = _new_or_skip(num_voices=8, max_frames=64)
    if syn is not None:
        check_ranges(syn)


def check_ranges(syn):
    L, h = syn.L, syn.h
    for level, sens, bus in BAD:
        assert L.s2r_set_program_mix(h, 0, level, sens, bus) == s2s.S2R_ERR_PATCH_RANGE, (level, sens, bus)
    assert syn.get_program_mix(0) == (1.0, 0.0, 0)              # the defaults; a refused call changes nothing
    assert L.s2r_set_program_mix(h, 1, 1.0, 0.0, 0) == s2s.S2R_ERR_INVALID   # a bank of one
    assert L.s2r_set_program_mix(h, 256, 1.0, 0.0, 0) == s2s.S2R_ERR_INVALID
    lv, se, bu = C.c_float(), C.c_float(), C.c_uint32()
    assert L.s2r_get_program_mix(h, 1, C.byref(lv), C.byref(se), C.byref(bu)) == s2s.S2R_ERR_INVALID
    syn.set_program_mix(0, 0.25, 1.0, 7)
    assert syn.get_program_mix(0) == (0.25, 1.0, 7)
    # the bank grows, shrinks: survivors keep their mix, the rest come back with the defaults
    syn.set_patch_bank([s2.default_patch()] * 3)
    assert syn.get_program_mix(0) == (0.25, 1.0, 7) and syn.get_program_mix(2) == (1.0, 0.0, 0)
    syn.set_program_mix(2, 0.5, 0.75, 3)
    syn.set_patch_bank([s2.default_patch()] * 2)
    assert L.s2r_set_program_mix(h, 2, 1.0, 0.0, 0) == s2s.S2R_ERR_INVALID
    syn.set_patch_bank([s2.default_patch()] * 3)
    assert syn.get_program_mix(2) == (1.0, 0.0, 0) and syn.get_program_mix(0) == (0.25, 1.0, 7)
    n = syn.shard_voices
    gains, buses = np.ones(n, dtype=F), np.zeros(n, dtype=np.uint8)
    before = syn.voice_mix()
    assert np.array_equal(bits(before[0]), bits(gains)) and not before[1].any()      # never started: gain 1, bus 0
    for bad_gain, bad_bus in [(1.5, 0), (-0.5, 0), (NAN, 0), (0.5, 8), (0.5, 255)]:
        gains[:] = 0.25
        buses[:] = 2
        gains[-1], buses[-1] = bad_gain, bad_bus
        assert L.s2r_set_voice_mix(h, gains.ctypes.data_as(s2s._f32p), buses.ctypes.data_as(_u8p)) == s2s.S2R_ERR_PATCH_RANGE
        got = syn.voice_mix()
        assert np.array_equal(bits(got[0]), bits(before[0])) and not got[1].any()    # nothing was changed
    assert L.s2r_set_voice_mix(h, gains.ctypes.data_as(s2s._f32p), None) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_voice_mix(h, None, buses.ctypes.data_as(_u8p)) == s2s.S2R_ERR_INVALID
    gains[:] = np.linspace(0, 1, n, dtype=F)
    buses[:] = np.arange(n) % 8
    syn.set_voice_mix(gains, buses)
    got = syn.voice_mix()
    assert np.array_equal(bits(got[0]), bits(gains)) and np.array_equal(got[1], buses)
