"""True stereo, the host side: the pan a note_on gives its voice and the constant-power gains, held against
numpy float32 restatements of their op sequences, and the range checks of the entry points that need no device."""
import ctypes as C

import numpy as np
import pytest

import synth2_amd as s2
from synth2_amd import synth as s2s

F = np.float32
VALUES = [-1.0, -0.5, 0.0, 1.0 / 3.0, 0.7, 1.0]


def np_voice_pan(pan, spread, note):
    k = F(int(note) - 64) * F(0.015625)                        # exact
    p = F(pan) + F(F(spread) * k)                               # product rounded, then the sum
    return F(-1.0) if p < F(-1.0) else (F(1.0) if p > F(1.0) else p)


def bits(x):
    return np.asarray(x, dtype=F).view(np.uint32)


def test_voice_pan_is_the_formula_for_every_note():
    clamped = 0
    for pan in VALUES:
        for spread in VALUES:
            for note in range(128):
                want = np_voice_pan(pan, spread, note)
                got = F(s2.voice_pan(pan, spread, note))
                assert bits(got) == bits(want), (pan, spread, note, got, want)
                raw = F(pan) + F(F(spread) * (F(note - 64) * F(0.015625)))
                clamped += int(raw < -1 or raw > 1)
    assert clamped > 100                                        # the grid does reach the clamp, on both sides
    assert s2.voice_pan(1.0, 1.0, 127) == 1.0 and s2.voice_pan(-1.0, 1.0, 0) == -1.0
    assert s2.voice_pan(0.25, 1.0, 64) == 0.25                  # note 64 is the spread's centre


def test_pan_gains_are_correctly_rounded_roots():
    p = (np.arange(-4096, 4097, dtype=np.int64).astype(np.float64) / 4096.0).astype(F)       # exact in binary32
    got = np.array([s2.pan_gains(float(x)) for x in p], dtype=F)
    one, half = F(1.0), F(0.5)
    want_l = np.sqrt((one - p) * half, dtype=F)
    want_r = np.sqrt((one + p) * half, dtype=F)
    assert np.array_equal(bits(got[:, 0]), bits(want_l))
    assert np.array_equal(bits(got[:, 1]), bits(want_r))
    # mirror symmetry, bit for bit: gL(-p) is gR(p)
    assert np.array_equal(bits(got[::-1, 0]), bits(got[:, 1]))
    # constant power: each gain is within half an ulp of the true root of a value that itself carries half an ulp, and
    # g <= 1, so each square is off by at most 2^-24 + 2^-24
    power = got[:, 0].astype(np.float64) ** 2 + got[:, 1].astype(np.float64) ** 2
    assert np.max(np.abs(power - 1.0)) <= 2.0 ** -22
    assert s2.pan_gains(-1.0) == (1.0, 0.0) and s2.pan_gains(1.0) == (0.0, 1.0)
    c = float(np.sqrt(F(0.5), dtype=F))
    assert s2.pan_gains(0.0) == (c, c)


def _new_or_skip(**kw):
    try:
        return s2.Synth(**kw)
    except s2.S2rError as e:
        if e.status == s2s.S2R_ERR_NO_DEVICE:
            return None
        raise


BAD = [(1.5, 0.0), (-1.0000001, 0.0), (0.0, 1.0000001), (0.0, -2.0), (float("nan"), 0.0), (0.0, float("nan")), (float("inf"), 0.0)]


def test_range_errors_and_program_bounds():
    """s2r_set_program_pan looks at the values before it looks at the handle, so the range check answers without a device;
    S2R_ERR_INVALID is what a handle that has no such program — here: no handle — gets for values in range.  With a device
    the bank-size cases run on a real handle (check_ranges, also called by tests/test_gpu_panned.py)."""
    L = s2.load_library()
    for pan, spread in BAD:
        assert L.s2r_set_program_pan(None, 0, pan, spread) == s2s.S2R_ERR_PATCH_RANGE, (pan, spread)
    for pan, spread in [(0.0, 0.0), (-1.0, 1.0), (1.0, -1.0)]:
        assert L.s2r_set_program_pan(None, 0, pan, spread) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_panned(None, None, 16, 48000) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_voice_pans(None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_voice_pans(None, None) == s2s.S2R_ERR_INVALID
    syn = _new_or_skip(num_voices=8, max_frames=64)
    if syn is not None:
        check_ranges(syn)


def check_ranges(syn):
    L, h = syn.L, syn.h
    nan = float("nan")
    for pan, spread in BAD:
        assert L.s2r_set_program_pan(h, 0, pan, spread) == s2s.S2R_ERR_PATCH_RANGE, (pan, spread)
    assert syn.get_program_pan(0) == (0.0, 0.0)                 # a refused call changes nothing
    assert L.s2r_set_program_pan(h, 1, 0.0, 0.0) == s2s.S2R_ERR_INVALID      # a bank of one
    assert L.s2r_set_program_pan(h, 256, 0.0, 0.0) == s2s.S2R_ERR_INVALID
    pan, spread = C.c_float(), C.c_float()
    assert L.s2r_get_program_pan(h, 1, C.byref(pan), C.byref(spread)) == s2s.S2R_ERR_INVALID
    syn.set_program_pan(0, -1.0, 1.0)
    assert syn.get_program_pan(0) == (-1.0, 1.0)
    # the bank grows, shrinks: survivors keep their pans, the rest come back as 0 / 0
    syn.set_patch_bank([s2.default_patch()] * 3)
    assert syn.get_program_pan(0) == (-1.0, 1.0) and syn.get_program_pan(2) == (0.0, 0.0)
    syn.set_program_pan(2, 0.5, -0.25)
    syn.set_patch_bank([s2.default_patch()] * 2)
    assert L.s2r_set_program_pan(h, 2, 0.0, 0.0) == s2s.S2R_ERR_INVALID
    syn.set_patch_bank([s2.default_patch()] * 3)
    assert syn.get_program_pan(2) == (0.0, 0.0) and syn.get_program_pan(0) == (-1.0, 1.0)
    pans = np.zeros(syn.shard_voices, dtype=F)
    for bad in (1.5, -1.5, nan):
        pans[:] = 0.25
        pans[-1] = bad
        assert L.s2r_set_voice_pans(h, pans.ctypes.data_as(s2s._f32p)) == s2s.S2R_ERR_PATCH_RANGE
        assert not syn.voice_pans().any()                       # nothing was changed
    pans[:] = np.linspace(-1, 1, pans.size, dtype=F)
    syn.set_voice_pans(pans)
    assert np.array_equal(bits(syn.voice_pans()), bits(pans))
