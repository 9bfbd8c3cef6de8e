"""The master section, the host side: s2r_master_reference — the rule restated in plain C++ — held against a numpy
float32 model of the rule written here (np_master and np_meters, which tests/test_gpu_master.py holds the device against too), both
against a float64 evaluation inside a derived bound, and the range checks of the entry points, which answer without a device."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_reverb_host import MIXED, _new_or_skip, _p, bits

F = np.float32
NAN = float("nan")
INF = float("inf")
BLOCK = 256
BAD_LEVEL = [1.5, -0.25, -1e-9, 1.0000001, NAN, INF, -INF]
GOOD_LEVEL = [0.0, 1.0, 0.5, 1.0 / 3.0]
BUSES = [1, 2, 3, 8]
FRAMES = [1, 2, 255, 256, 257, 1000]


def np_ramp(g0, g1, n):
    """g[i] = G0 + (float)i * ((G1 - G0) / (float)N), every operation rounded to binary32; [n]"""
    g0, g1 = F(g0), F(g1)
    d = F(g1 - g0) / F(n)
    assert d.dtype == F
    with np.errstate(under="ignore"):
        return g0 + np.arange(n, dtype=F) * d


def np_master(stems, r0, r1, m0, m1):
    """The rule in numpy float32: stems [n_buses, N, 2]; t = ((+0.0 + r_0 * y_0) + r_1 * y_1) + ... in bus order, every product
    rounded, then every sum; out = m * t.  [N, 2]"""
    y = np.ascontiguousarray(stems, dtype=F)
    n = y.shape[1]
    t = np.zeros((n, 2), dtype=F)
    with np.errstate(under="ignore"):
        for b in range(y.shape[0]):
            p = np_ramp(r0[b], r1[b], n)[:, None] * y[b]
            t = t + p
        out = np_ramp(m0, m1, n)[:, None] * t
    assert out.dtype == F
    return out


def np_energy(v, tree=True):
    """one channel's energy: the squares, rounded; blocks of 256 frames, frames past the end +0.0; every block by the adjacent-pair
    tree, eight levels; the block sums in block order from +0.0.  tree=False: the squares in plain index order (what the rule is NOT)"""
    v = np.ascontiguousarray(v, dtype=F)
    with np.errstate(under="ignore", over="ignore"):
        q = v * v
        total = F(0.0)
        if not tree:
            for x in q:
                total = total + x
            return total
        q = np.concatenate([q, np.zeros(-q.size % BLOCK, dtype=F)]).reshape(-1, BLOCK)
        for _ in range(8):
            q = q[:, 0::2] + q[:, 1::2]
        assert q.shape[1] == 1 and q.dtype == F
        for x in q[:, 0]:
            total = total + x
    return total


def np_meters(stems, master):
    """(peak, energy), each [n_buses + 1, 2]: the buses on the stems, then the master"""
    chans = np.concatenate([np.ascontiguousarray(stems, dtype=F), np.ascontiguousarray(master, dtype=F)[None]], axis=0)
    peak = np.abs(chans).max(axis=1).astype(F)
    energy = np.array([[np_energy(ch[:, c]) for c in range(2)] for ch in chans], dtype=F)
    return peak, energy


def f64_master_and_bound(stems, r0, r1, m0, m1):
    """out64 = m * sum_b r_b * y_b in float64 with no float32 sum or product in it, and the bound that any float32 evaluation of the
    rule keeps against it.  The gains r_b[i] and m[i] are the rule's binary32 ramp values and enter exactly (they are inputs of the
    sum, and a ramp towards 0 cancels: its relative error is no multiple of u).  A term of out then passes through its product with
    the return, at most n_buses sums (the first, onto +0.0, is exact) and the product with the master gain: no more than n =
    n_buses + 3 roundings, each of relative size u = 2^-24 while nothing underflows, so (Higham, Accuracy and Stability of Numerical
    Algorithms, section 3.1) |out - out64| <= gamma_n * |m| * sum_b |r_b| |y_b| with gamma_n = n u / (1 - n u); an operation whose
    result is denormal errs by at most 2^-150 instead, and the n_buses products, n_buses sums and the master's product add at most
    (2 n_buses + 1) * 2^-149 for that, generously.  Returns (out64, bound), float64 [N, 2]."""
    y = np.ascontiguousarray(stems, dtype=F).astype(np.float64)
    nb, n = y.shape[0], y.shape[1]
    r = np.stack([np_ramp(r0[b], r1[b], n) for b in range(nb)]).astype(np.float64)
    m = np_ramp(m0, m1, n).astype(np.float64)
    out64 = m[:, None] * (r[:, :, None] * y).sum(axis=0)
    k = nb + 3
    u = 2.0 ** -24
    gamma = k * u / (1.0 - k * u)
    bound = gamma * np.abs(m)[:, None] * (np.abs(r)[:, :, None] * np.abs(y)).sum(axis=0) + (2 * nb + 1) * 2.0 ** -149
    return out64, bound


def noise_stems(nb, n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (nb, n, 2)).astype(F)


def crafted_stems(nb, n):
    """the magnitudes of tests/test_gpu_reverb_tiles.py's crafted histories — 1e30, -1e30, 2^-126, -2^-140, both zeros, 3.0, 2^-149 —
    every bus and channel starting at another element"""
    return np.stack([np.stack([np.resize(np.roll(MIXED, -(3 * b + c)), n) for c in range(2)], axis=1) for b in range(nb)]).astype(F)


def pairs(nb, moving):
    """(r0, r1, m0, m1): distinct levels, the ends of the range among them; moving: most pairs on their way, bus 1 still"""
    r0 = np.array([1.0 - b / 16.0 for b in range(nb)], dtype=F)
    if not moving:
        return r0, r0.copy(), F(0.7), F(0.7)
    r1 = np.array([[0.0, 1.0 - 1.0 / 16.0, 1.0, 1.0 / 3.0][b % 4] if b != 1 else r0[1] for b in range(nb)], dtype=F)
    return r0, r1, F(0.7), F(0.25)


def _reference_is_model(y, r0, r1, m0, m1, what, energy_finite=True):
    got, peak, energy = s2.master_reference(y, r0, r1, m0, m1)
    want = np_master(y, r0, r1, m0, m1)
    assert_bits_equal_finite(got, want, what + ": master")
    wp, we = np_meters(y, want)
    assert_bits_equal_finite(peak, wp, what + ": peaks")
    if energy_finite:
        assert_bits_equal_finite(energy, we, what + ": energies")
    else:
        assert np.array_equal(bits(energy), bits(we)), what + ": energies"
    return got, peak, energy


@pytest.mark.parametrize("nb", BUSES)
@pytest.mark.parametrize("moving", [False, True])
def test_reference_is_the_rule_on_noise(nb, moving):
    for n in FRAMES:
        y = noise_stems(nb, n, 100 * nb + n)
        r0, r1, m0, m1 = pairs(nb, moving)
        got, _, energy = _reference_is_model(y, r0, r1, m0, m1, "%d buses, %d frames, moving %d" % (nb, n, moving))
        assert bits(got).any() and (energy > 0.0).all()
        if moving and n > 1:                                     # the ramp is visible: not the static expectation at the applied pairs
            assert not np.array_equal(bits(got), bits(np_master(y, r0, r0, m0, m0)))
    assert np.array_equal(bits(s2.Synth.master_reference(y, r0, r1, m0, m1)[0]), bits(got))


@pytest.mark.parametrize("nb", BUSES)
@pytest.mark.parametrize("moving", [False, True])
def test_reference_is_the_rule_on_crafted_magnitudes(nb, moving):
    """terms of 1e30 that cancel beside denormals and both zeros.  The master and the peaks are finite and compared as such; the
    square of 1e30 is +inf in binary32, in the model and in the reference alike, and a sum of squares holds no inf - inf: the energies
    are compared on bits without the finiteness guard, and that they do overflow is asserted."""
    for n in FRAMES:
        y = crafted_stems(nb, n)
        r0, r1, m0, m1 = pairs(nb, moving)
        _, peak, energy = _reference_is_model(y, r0, r1, m0, m1, "crafted, %d buses, %d frames, moving %d" % (nb, n, moving), energy_finite=False)
        assert not np.isnan(energy).any()
        if n >= 8:
            assert np.isinf(energy[:nb]).all() and (peak[:nb] == F(1e30)).all()


@pytest.mark.parametrize("nb", BUSES)
def test_a_one_frame_call_is_the_static_one(nb):
    """its only frame is i = 0: the gains are R0 and M0 whatever the targets are"""
    y = noise_stems(nb, 1, 7 + nb)
    r0, r1, m0, m1 = pairs(nb, True)
    got = s2.master_reference(y, r0, r1, m0, m1)[0]
    assert_bits_equal_finite(got, np_master(y, r0, r0, m0, m0), "one frame, %d buses" % nb)
    assert_bits_equal_finite(got, np_master(y, r0, r1, m0, m1), "one frame, %d buses: the model" % nb)


def test_the_energy_tree_is_not_the_sequential_sum():
    """on the noise stems the adjacent-pair tree and the sum in index order differ in bits, so a wrong order cannot pass the parity
    tests; the reference is the tree"""
    differ = 0
    for n in (255, 256, 257, 1000):
        y = noise_stems(2, n, 31 + n)
        energy = s2.master_reference(y, [1.0, 1.0], [1.0, 1.0], 1.0, 1.0)[2]
        for b in range(2):
            for c in range(2):
                tree, plain = np_energy(y[b, :, c]), np_energy(y[b, :, c], tree=False)
                assert bits(energy[b, c]) == bits(tree)
                differ += int((bits(tree) != bits(plain)).any())
    assert differ >= 8, differ                                   # of sixteen channels


def test_blocks_add_in_block_order():
    """1000 frames are four blocks, the last partial: their sums are added from +0.0 in block order, not by a tree over the blocks"""
    y = noise_stems(1, 1000, 5)
    v = y[0, :, 0]
    sums = [np_energy(v[k:k + BLOCK]) for k in range(0, 1000, BLOCK)]
    seq = ((F(0.0) + sums[0]) + sums[1]) + sums[2]
    seq = seq + sums[3]
    assert bits(np_energy(v)) == bits(F(seq))
    assert bits(s2.master_reference(y, [1.0], [1.0], 1.0, 1.0)[2][0, 0]) == bits(F(seq))


@pytest.mark.parametrize("nb", BUSES)
def test_model_and_reference_are_a_float64_sum(nb):
    """np_master and s2r_master_reference are two restatements of one reading of the rule; the float64 evaluation is none.  Both stay
    inside f64_master_and_bound, which is derived and not measured; a sum over the buses in reverse gains — a misreading of which
    return belongs to which bus — is far outside it."""
    n = 1000
    y = noise_stems(nb, n, 900 + nb)
    for moving in (False, True):
        r0, r1, m0, m1 = pairs(nb, moving)
        out64, bound = f64_master_and_bound(y, r0, r1, m0, m1)
        assert (bound > 0.0).all() and np.abs(out64).max() > 0.01
        for name, got in (("np_master", np_master(y, r0, r1, m0, m1)), ("s2r_master_reference", s2.master_reference(y, r0, r1, m0, m1)[0])):
            ratio = np.abs(got.astype(np.float64) - out64) / bound
            print("%d buses, moving %d, %s: largest error over the bound %.4f" % (nb, moving, name, ratio.max()))
            assert ratio.max() <= 1.0, (nb, moving, name, float(ratio.max()))
    if nb > 1:
        r0, r1, m0, m1 = pairs(nb, False)
        out64, bound = f64_master_and_bound(y, r0, r1, m0, m1)
        assert (np.abs(np_master(y, r0[::-1], r1[::-1], m0, m1).astype(np.float64) - out64) > bound).mean() > 0.9


def test_range_errors_without_a_handle():
    """every entry looks at the values before it looks at the handle, so the range checks answer without a device; S2R_ERR_INVALID is
    what no handle gets for values in range.  With a device the rest runs on a real handle (check_ranges, also called by
    tests/test_gpu_master.py)."""
    L = s2.load_library()
    assert s2.METER_BLOCK == BLOCK
    for level in BAD_LEVEL:
        assert L.s2r_set_bus_return(None, 0, level) == s2s.S2R_ERR_PATCH_RANGE, level
        assert L.s2r_set_master_fader(None, level) == s2s.S2R_ERR_PATCH_RANGE, level
    for level in GOOD_LEVEL:
        assert L.s2r_set_bus_return(None, 0, level) == s2s.S2R_ERR_INVALID, level
        assert L.s2r_set_bus_return(None, 7, level) == s2s.S2R_ERR_INVALID, level
        assert L.s2r_set_master_fader(None, level) == s2s.S2R_ERR_INVALID, level
    f, g = C.c_float(), C.c_float()
    for bus in (8, 255, 0xffffffff):
        assert L.s2r_set_bus_return(None, bus, 0.5) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_get_bus_return(None, bus, C.byref(f), C.byref(g)) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_return(None, 0, C.byref(f), C.byref(g)) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_return(None, 0, None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_master_fader(None, C.byref(f), C.byref(g)) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_master_fader(None, None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_snap_master(None) == s2s.S2R_ERR_INVALID
    buf = np.zeros(64, dtype=F)
    n = C.c_uint32()
    assert L.s2r_fill_master(None, _p(buf), _p(buf), 64, 1, 16, 48000) == s2s.S2R_ERR_INVALID
    assert L.s2r_fill_master(None, _p(buf), None, 0, 1, 16, 48000) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_meters(None, C.byref(n), _p(buf), _p(buf), 64) == s2s.S2R_ERR_INVALID
    # the reference
    y, one, out = np.zeros((2, 3, 2), dtype=F), np.ones(2, dtype=F), np.zeros(6, dtype=F)
    for level in BAD_LEVEL:
        bad = one.copy()
        bad[1] = level
        assert L.s2r_master_reference(_p(y), 2, 3, _p(bad), _p(one), 1.0, 1.0, _p(out), None, None) == s2s.S2R_ERR_PATCH_RANGE, level
        assert L.s2r_master_reference(_p(y), 2, 3, _p(one), _p(bad), 1.0, 1.0, _p(out), None, None) == s2s.S2R_ERR_PATCH_RANGE, level
        assert L.s2r_master_reference(_p(y), 2, 3, _p(one), _p(one), level, 1.0, _p(out), None, None) == s2s.S2R_ERR_PATCH_RANGE, level
        assert L.s2r_master_reference(_p(y), 2, 3, _p(one), _p(one), 1.0, level, _p(out), None, None) == s2s.S2R_ERR_PATCH_RANGE, level
    for nb in (0, 9, 0xffffffff):
        assert L.s2r_master_reference(_p(y), nb, 3, _p(one), _p(one), 1.0, 1.0, _p(out), None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_master_reference(None, 2, 3, _p(one), _p(one), 1.0, 1.0, _p(out), None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_master_reference(_p(y), 2, 3, None, _p(one), 1.0, 1.0, _p(out), None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_master_reference(_p(y), 2, 3, _p(one), None, 1.0, 1.0, _p(out), None, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_master_reference(_p(y), 2, 3, _p(one), _p(one), 1.0, 1.0, None, None, None) == s2s.S2R_OK     # any output may be null
    pk = np.full(6, 7.0, dtype=F)
    assert L.s2r_master_reference(_p(y), 2, 3, _p(one), _p(one), 1.0, 1.0, None, _p(pk), None) == s2s.S2R_OK
    assert not bits(pk).any()
    with pytest.raises(ValueError):
        s2.master_reference(np.zeros((2, 3), dtype=F), one, one, 1.0, 1.0)
    with pytest.raises(s2.S2rError) as err:
        s2.master_reference(y, one, one, 1.5, 1.0)
    assert err.value.status == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_abi_version() == 4
    syn = _new_or_skip(num_voices=8, max_frames=64)
    if syn is not None:
        check_ranges(syn)


def check_ranges(syn):
    """the entries on a real handle: the defaults, refusals that change nothing, getters with null pointers, snap, and that the
    section belongs to the buses and the handle — a new bank and a program change leave it alone"""
    L, h = syn.L, syn.h
    assert all(syn.get_bus_return(b) == (1.0, 1.0) for b in range(s2.MAX_BUSES)) and syn.get_master_fader() == (1.0, 1.0)
    n = C.c_uint32()
    buf = np.zeros(2 * (s2.MAX_BUSES + 1), dtype=F)
    assert L.s2r_get_meters(h, C.byref(n), _p(buf), _p(buf), buf.size) == s2s.S2R_ERR_INVALID      # no master fill yet
    syn.set_bus_return(3, 0.25)
    syn.set_master_fader(0.5)
    for level in BAD_LEVEL:
        assert L.s2r_set_bus_return(h, 3, level) == s2s.S2R_ERR_PATCH_RANGE, level
        assert L.s2r_set_master_fader(h, level) == s2s.S2R_ERR_PATCH_RANGE, level
    assert L.s2r_set_bus_return(h, 8, 0.5) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_return(h, 8, None, None) == s2s.S2R_ERR_PATCH_RANGE
    assert syn.get_bus_return(3) == (0.25, 1.0) and syn.get_master_fader() == (0.5, 1.0)           # targets; nothing applied yet
    assert L.s2r_get_bus_return(h, 3, None, None) == s2s.S2R_OK and L.s2r_get_master_fader(h, None, None) == s2s.S2R_OK
    f = C.c_float()
    assert L.s2r_get_bus_return(h, 3, None, C.byref(f)) == s2s.S2R_OK and f.value == 1.0
    assert L.s2r_get_master_fader(h, C.byref(f), None) == s2s.S2R_OK and f.value == 0.5
    syn.set_patch_bank([s2.default_patch()] * 3)
    syn.program_change(2)
    assert syn.get_bus_return(3) == (0.25, 1.0) and syn.get_master_fader() == (0.5, 1.0)
    syn.snap_master()
    assert syn.get_bus_return(3) == (0.25, 0.25) and syn.get_master_fader() == (0.5, 0.5)
    assert all(syn.get_bus_return(b) == (1.0, 1.0) for b in range(s2.MAX_BUSES) if b != 3)
    for b in range(s2.MAX_BUSES):
        syn.set_bus_return(b, 1.0)
    syn.set_master_fader(1.0)
    syn.snap_master()
