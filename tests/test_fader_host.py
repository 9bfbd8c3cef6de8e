"""Live program faders, the host side: the two gains of a voice under a fader pair, held against a numpy
float32 restatement of the rule's op sequence, and the range checks of the entry points that need no device."""
import ctypes as C

import numpy as np

import synth2_amd as s2
from synth2_amd import synth as s2s

F = np.float32
PANS = [-1.0, -0.5, -0.0, 0.0, 1.0 / 3.0, 1.0]
WS = [0.0, 1.0 / 3.0, 0.7, 1.0]
FADERS = [0.0, 2.0 ** -149, 1.0 / 3.0, 1.0]
SHIFTS = [-2.0, -1.0, -0.25, 0.0, 0.25, 2.0]
NAN, INF = float("nan"), float("inf")


def bits(x):
    return np.asarray(x, dtype=F).view(np.uint32)


def np_fader_gains(pan, w, fader, shift):
    """q = pan + shift clamped to [-1, 1] with < / >; (aL, aR) = sqrtf((1 -/+ q) * 0.5f); G_c = (a_c * w) * fader — binary32,
    every operation rounded on its own.  Arrays or scalars (broadcast)."""
    pan, w, fader, shift = (np.asarray(x, dtype=F) for x in (pan, w, fader, shift))
    q = (pan + shift).astype(F)
    q = np.where(q < F(-1.0), F(-1.0), np.where(q > F(1.0), F(1.0), q)).astype(F)
    al = np.sqrt(((F(1.0) - q) * F(0.5)).astype(F), dtype=F)
    ar = np.sqrt(((F(1.0) + q) * F(0.5)).astype(F), dtype=F)
    with np.errstate(under="ignore"):
        return ((al * w).astype(F) * fader).astype(F), ((ar * w).astype(F) * fader).astype(F)


def test_fader_gains_are_the_formula():
    distinct = set()
    for pan in PANS:
        for w in WS:
            for fader in FADERS:
                for shift in SHIFTS:
                    want = np_fader_gains(pan, w, fader, shift)
                    got = s2.fader_gains(pan, w, fader, shift)
                    for c in range(2):
                        assert bits(F(got[c])) == bits(want[c]), (pan, w, fader, shift, c, got, want)
                        assert 0.0 <= got[c] <= 1.0
                        distinct.add(int(bits(F(got[c]))))
    assert len(distinct) > 40                                   # the grid is not a table of zeros and ones


def test_the_order_of_the_two_multiplies_is_pinned():
    """(a * w) * f, not a * (w * f) and not (a * f) * w: the grid holds points where each other order gives other bits"""
    other_a = other_b = 0
    for pan in PANS:
        for w in WS:
            for fader in FADERS:
                q = F(pan)
                a = np.sqrt((F(1.0) - q) * F(0.5), dtype=F)
                with np.errstate(under="ignore"):
                    right = F(F(a * F(w)) * F(fader))
                    other_a += int(bits(F(a * F(F(w) * F(fader)))) != bits(right))
                    other_b += int(bits(F(F(a * F(fader)) * F(w))) != bits(right))
                assert bits(F(s2.fader_gains(pan, w, fader, 0.0)[0])) == bits(right)
    assert other_a > 0 and other_b > 0


def test_defaults_are_the_mixers_gains():
    """fader 1 and shift 0: pan_gains(p) * w, bit for bit — p + 0.0f changes at most the sign of a zero, * 1.0f is exact"""
    for pan in PANS + [0.7, -0.25, 1.0 - 2.0 ** -24]:
        gl, gr = s2.pan_gains(pan)
        for w in WS + [2.0 ** -149, 0.25]:
            got = s2.fader_gains(pan, w, 1.0, 0.0)
            with np.errstate(under="ignore"):
                assert bits(F(got[0])) == bits(F(F(gl) * F(w))) and bits(F(got[1])) == bits(F(F(gr) * F(w))), (pan, w)
            assert np.array_equal(bits(s2.fader_gains(pan, w, 1.0, -0.0)), bits(got))


def test_the_shift_clamps_at_both_ends():
    for pan in PANS:
        for shift, hard in [(2.0, (0.0, 1.0)), (-2.0, (1.0, 0.0))]:
            assert s2.fader_gains(pan, 1.0, 1.0, shift) == hard, (pan, shift)
    assert s2.fader_gains(-1.0, 1.0, 1.0, 2.0) == (0.0, 1.0)    # a shift of 2 takes a hard-left voice hard right
    assert s2.fader_gains(0.5, 1.0, 1.0, 0.75) == (0.0, 1.0) and s2.fader_gains(-0.5, 1.0, 1.0, -0.75) == (1.0, 0.0)
    # just inside the clamp the shifted pan is still the pan law's
    p = float(F(1.0) - F(2.0 ** -24))
    assert s2.fader_gains(0.0, 1.0, 1.0, p) == s2.pan_gains(p) and s2.fader_gains(0.0, 1.0, 1.0, p)[0] > 0.0
    # either pointer may be null
    L = s2.load_library()
    g = C.c_float(-1.0)
    L.s2r_fader_gains(0.25, 0.5, 0.5, 0.25, None, C.byref(g))
    assert g.value == s2.fader_gains(0.25, 0.5, 0.5, 0.25)[1]
    L.s2r_fader_gains(0.25, 0.5, 0.5, 0.25, C.byref(g), None)
    assert g.value == s2.fader_gains(0.25, 0.5, 0.5, 0.25)[0]


def _past(x, up):
    """the binary32 next to x, above or below"""
    return float(np.nextafter(F(x), F(INF if up else -INF), dtype=F))


# each float one past its border, NaN and +-Inf
BAD = [(_past(1.0, True), 0.0), (_past(0.0, False), 0.0), (NAN, 0.0), (INF, 0.0), (-INF, 0.0),
       (1.0, _past(2.0, True)), (1.0, _past(-2.0, False)), (1.0, NAN), (1.0, INF), (1.0, -INF), (0.5, 2.5), (1.5, 0.0)]
GOOD = [(1.0, 0.0), (0.0, -2.0), (1.0, 2.0), (2.0 ** -149, -0.0), (_past(1.0, False), _past(2.0, False))]


def _new_or_skip(**kw):
    try:
        return s2.Synth(**kw)
    except s2.S2rError as e:
        if e.status == s2s.S2R_ERR_NO_DEVICE:
            return None
        raise


def test_range_errors_and_program_bounds():
    """s2r_set_program_fader looks at the values before it looks at the handle, so the range check answers without a device;
    S2R_ERR_INVALID is what no handle gets for values in range.  With a device the cases run on a real handle (check_ranges,
    also called by tests/test_gpu_faders.py)."""
    L = s2.load_library()
    assert _past(0.0, False) < 0.0 and _past(1.0, True) > 1.0
    for fader, shift in BAD:
        assert L.s2r_set_program_fader(None, 0, fader, shift) == s2s.S2R_ERR_PATCH_RANGE, (fader, shift)
    for fader, shift in GOOD:
        assert L.s2r_set_program_fader(None, 0, fader, shift) == s2s.S2R_ERR_INVALID, (fader, shift)
    f = C.c_float()
    assert L.s2r_get_program_fader(None, 0, C.byref(f), None, None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_snap_program_faders(None) == s2s.S2R_ERR_INVALID
    syn = _new_or_skip(num_voices=8, max_frames=64)
    if syn is not None:
        check_ranges(syn)


def check_ranges(syn):
    L, h = syn.L, syn.h
    assert syn.get_program_fader(0) == (1.0, 0.0, 1.0, 0.0)     # a fresh handle: target and applied at the defaults
    for setting in [(1.0, 0.0), (0.25, -1.5)]:
        syn.set_program_fader(0, *setting)
        for fader, shift in BAD:
            assert L.s2r_set_program_fader(h, 0, fader, shift) == s2s.S2R_ERR_PATCH_RANGE, (fader, shift)
            assert syn.get_program_fader(0) == setting + (1.0, 0.0)     # a refused call changes nothing
    assert L.s2r_set_program_fader(h, 1, 1.0, 0.0) == s2s.S2R_ERR_INVALID    # a bank of one
    assert L.s2r_set_program_fader(h, 256, 0.5, 0.0) == s2s.S2R_ERR_INVALID
    f = C.c_float()
    assert L.s2r_get_program_fader(h, 1, C.byref(f), None, None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_program_fader(h, 0, None, None, None, None) == s2s.S2R_OK       # any pointer may be null
    assert L.s2r_get_program_fader(h, 0, None, None, C.byref(f), None) == s2s.S2R_OK and f.value == 1.0
    for fader, shift in GOOD:
        syn.set_program_fader(0, fader, shift)
        got = syn.get_program_fader(0)
        assert np.array_equal(bits(got[:2]), bits((fader, shift))) and got[2:] == (1.0, 0.0)
    # snap: applied = target, now
    syn.set_program_fader(0, 0.25, -1.5)
    syn.snap_program_faders()
    assert syn.get_program_fader(0) == (0.25, -1.5, 0.25, -1.5)
    syn.set_program_fader(0, 0.5, 0.75)
    assert syn.get_program_fader(0) == (0.5, 0.75, 0.25, -1.5)
    # the bank grows, shrinks: survivors keep both pairs, the rest come back with the defaults
    syn.set_patch_bank([s2.default_patch()] * 3)
    assert syn.get_program_fader(0) == (0.5, 0.75, 0.25, -1.5) and syn.get_program_fader(2) == (1.0, 0.0, 1.0, 0.0)
    syn.set_program_fader(2, 0.125, 2.0)
    syn.snap_program_faders()
    assert syn.get_program_fader(2) == (0.125, 2.0, 0.125, 2.0) and syn.get_program_fader(0) == (0.5, 0.75, 0.5, 0.75)
    syn.set_patch_bank([s2.default_patch()] * 2)
    assert L.s2r_set_program_fader(h, 2, 1.0, 0.0) == s2s.S2R_ERR_INVALID
    syn.set_patch_bank([s2.default_patch()] * 3)
    assert syn.get_program_fader(2) == (1.0, 0.0, 1.0, 0.0) and syn.get_program_fader(0) == (0.5, 0.75, 0.5, 0.75)
