"""The per-bus convolution reverb, the host side: s2r_reverb_reference — the rule restated in plain C++ — held
against a numpy float32 model of the rule written here (np_reverb, which tests/test_gpu_reverb.py holds the device against too),
and the range checks of the entry points, which answer without a device."""
import ctypes as C

import numpy as np
import pytest

import synth2_amd as s2
from synth2_amd import synth as s2s

F = np.float32
NAN = float("nan")
INF = float("inf")
SEG = 256
# (dry, wet)
BAD_MIX = [(1.5, 0.5), (0.5, 1.5), (-0.25, 1.0), (1.0, -1e-9), (1.0000001, 0.0), (NAN, 1.0), (0.0, NAN), (INF, 0.0), (0.0, -INF)]
GOOD_MIX = [(0.0, 1.0), (1.0, 0.5), (0.25, 1.0), (0.0, 0.0), (1.0, 1.0)]


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def np_reverb(ir, x_with_history, frames, dry, wet, segment=SEG):
    """The rule in numpy float32, one channel: per segment of `segment` taps P_s = ((+0.0 + ir[k] * xs(i - k)) + ...) in tap order,
    every product rounded, then every sum; r = ((+0.0 + P_0) + P_1) + ...; y = dry * x + wet * r.  A loop over the taps, vector
    operations over the frames.  x_with_history: K - 1 samples of history (oldest first), then `frames` dry samples."""
    ir = np.ascontiguousarray(ir, dtype=F)
    x = np.ascontiguousarray(x_with_history, dtype=F)
    K = ir.size
    assert x.size == K - 1 + frames
    r = np.zeros(frames, dtype=F)
    with np.errstate(under="ignore"):
        for k0 in range(0, K, segment):
            p = np.zeros(frames, dtype=F)
            for k in range(k0, min(K, k0 + segment)):
                p = p + ir[k] * x[K - 1 - k:K - 1 - k + frames]
            r = r + p
        y = F(dry) * x[K - 1:] + F(wet) * r
    assert y.dtype == F
    return y


def f64_reverb_and_bound(ir, line, frames, dry, wet):
    """One channel with no float32 arithmetic and no segments in it: y64 = dry * x + wet * np.convolve(line, ir)[K - 1 : K - 1 +
    frames] in float64 over line = K - 1 samples of history, then `frames` dry samples, and the bound that any float32 evaluation of
    the rule keeps against it.  The rule adds at most min(K, 256) rounded products in a segment, then ceil(K / 256) segment sums,
    then takes two products and one sum for the mix: no term of y passes through more than n = min(K, 256) + ceil(K / 256) + 2
    roundings, each of relative size u = 2^-24 while nothing underflows, so (Higham, Accuracy and Stability of Numerical
    Algorithms, section 3.1) |y - y64| <= gamma_n * (dry * |x| + wet * (|ir| conv |line|)) with gamma_n = n u / (1 - n u); an
    operation whose result is denormal errs by at most 2^-150 instead, and K products, K sums and the three operations of the mix
    add at most (K + 3) * 2^-149 for that, generously.  Returns (y64, bound), float64 [frames]."""
    ir64 = np.ascontiguousarray(ir, dtype=F).astype(np.float64)
    line64 = np.ascontiguousarray(line, dtype=F).astype(np.float64)
    K = ir64.size
    assert line64.size == K - 1 + frames
    d, w = float(F(dry)), float(F(wet))
    x = line64[K - 1:]
    y64 = d * x + w * np.convolve(line64, ir64)[K - 1:K - 1 + frames]
    n = min(K, SEG) + (K + SEG - 1) // SEG + 2
    u = 2.0 ** -24
    gamma = n * u / (1.0 - n * u)
    bound = gamma * (d * np.abs(x) + w * np.convolve(np.abs(line64), np.abs(ir64))[K - 1:K - 1 + frames]) + (K + 3) * 2.0 ** -149
    return y64, bound


def crafted_denormal(K, seed):
    """a response scaled by 2^-70 and a history of K - 1 uniform samples scaled by 2^-68, one channel: every product is a denormal
    (or zero) and so is every sum of them"""
    ir, x = _case(K, 0, seed)
    return (ir * F(2.0 ** -70)).astype(F), (x * F(2.0 ** -68)).astype(F)


MIXED = np.array([1e30, -1e30, 2.0 ** -126, -2.0 ** -140, -0.0, 0.0, 3.0, 2.0 ** -149], dtype=F)


def crafted_mixed(K, seed, shift=0):
    """a response scaled by 1e-8 and a history of K - 1 samples that repeats MIXED from its element `shift` on, one channel: huge
    terms that cancel, the smallest normal, denormals, both zeros and an ordinary sample under one segment's taps"""
    ir, _ = _case(K, 0, seed)
    return (ir * F(1e-8)).astype(F), np.resize(np.roll(MIXED, -shift), K - 1).astype(F)


def _case(K, frames, seed):
    rng = np.random.default_rng(seed)
    ir = (rng.standard_normal(K) * np.exp(-np.arange(K) / max(K / 3.0, 1.0))).astype(F)
    x = rng.uniform(-1.0, 1.0, K - 1 + frames).astype(F)
    return ir, x


@pytest.mark.parametrize("K", [1, 2, 255, 256, 257, 511, 513, 600])
def test_reference_is_the_rule(K):
    for n, frames in enumerate([1, 16, 17, 1000]):
        ir, x = _case(K, frames, 1000 * K + n)
        for dry, wet in [(0.0, 1.0), (1.0, 0.5), (0.25, 1.0)]:
            got = s2.reverb_reference(ir, x, frames, dry, wet)
            want = np_reverb(ir, x, frames, dry, wet)
            assert np.isfinite(want).all()
            assert np.array_equal(bits(got), bits(want)), (K, frames, dry, wet)
    assert np.array_equal(bits(s2.Synth.reverb_reference(ir, x, frames, 0.25, 1.0)), bits(want))


def test_reference_keeps_denormal_products():
    K, frames = 300, 64
    ir, x = _case(K, frames, 7)
    ir = (ir * F(2.0 ** -70)).astype(F)
    x = (x * F(2.0 ** -68)).astype(F)
    want = np_reverb(ir, x, frames, 0.0, 1.0)
    mag = np.abs(want.astype(np.float64))
    assert ((mag > 0.0) & (mag < 2.0 ** -126)).all()            # every sample is a denormal sum of denormal products
    assert np.array_equal(bits(s2.reverb_reference(ir, x, frames, 0.0, 1.0)), bits(want))
    assert np.array_equal(bits(s2.reverb_reference(ir, x, frames, 1.0, 1.0)), bits(np_reverb(ir, x, frames, 1.0, 1.0)))


def test_the_segmented_sum_is_not_the_plain_sum():
    """K = 600 over 1000 frames: most samples of the segmented sum differ in bits from the sum in plain index order, so a wrong order
    cannot pass the parity tests; the reference is the segmented one"""
    K, frames = 600, 1000
    ir, x = _case(K, frames, 11)
    seg = np_reverb(ir, x, frames, 0.0, 1.0)
    plain = np_reverb(ir, x, frames, 0.0, 1.0, segment=K)
    assert (bits(seg) != bits(plain)).mean() > 0.5
    got = s2.reverb_reference(ir, x, frames, 0.0, 1.0)
    assert np.array_equal(bits(got), bits(seg)) and not np.array_equal(bits(got), bits(plain))


def test_the_longest_response():
    K, frames = s2.MAX_IR_TAPS, 64
    ir, x = _case(K, frames, 13)
    assert np.array_equal(bits(s2.reverb_reference(ir, x, frames, 0.25, 1.0)), bits(np_reverb(ir, x, frames, 0.25, 1.0)))


@pytest.mark.parametrize("K", [1, 5, 600, 1300, 2049])
def test_model_and_reference_are_a_float64_convolution(K):
    """np_reverb and s2r_reverb_reference are two restatements of one reading of the rule; a plain float64 convolution is none.
    Both stay inside the summation bound of f64_reverb_and_bound over 2500 frames, which is derived and not measured: a worst
    case, of which the model uses about a third at K = 1 and under 1 % at K = 2049, so this catches a misreading of the rule — a
    wrong tap order against the samples, a history off by one, dry and wet swapped — and not a single dropped term."""
    frames = 2500
    ir, x = _case(K, frames, 31 * K)
    for dry, wet in [(0.0, 1.0), (1.0, 0.5), (0.25, 1.0)]:
        y64, bound = f64_reverb_and_bound(ir, x, frames, dry, wet)
        assert (bound > 0.0).all() and np.abs(y64).max() > 0.01
        for name, got in (("np_reverb", np_reverb(ir, x, frames, dry, wet)), ("s2r_reverb_reference", s2.reverb_reference(ir, x, frames, dry, wet))):
            ratio = np.abs(got.astype(np.float64) - y64) / bound
            print("K %d dry %g wet %g %s: largest error over the bound %.4f" % (K, dry, wet, name, ratio.max()))
            assert ratio.max() <= 1.0, (K, dry, wet, name, int(ratio.argmax()), float(ratio.max()))
    # the bound has teeth where it is meant to: the response against the samples in the wrong order is far outside it
    if K > 1:
        y64, bound = f64_reverb_and_bound(ir, x, frames, 0.0, 1.0)
        assert (np.abs(np_reverb(ir[::-1], x, frames, 0.0, 1.0).astype(np.float64) - y64) > bound).mean() > 0.9


def test_reference_on_the_crafted_lines():
    """the two lines that tests/test_gpu_reverb_tiles.py puts in front of the device through s2r_set_bus_reverb_history, at its K
    and call length, over an idle bus (+0.0 behind the history) and a sounding one: the reference is the model on bits, so the device
    test rests on a model that was checked at these inputs.  The conditions the device test states on the model are held here too."""
    K, frames = 1300, 1500
    rng = np.random.default_rng(5)
    for tail in (np.zeros(frames, dtype=F), rng.uniform(-3.0, 3.0, frames).astype(F)):
        ir, hist = crafted_denormal(K, 41)
        line = np.concatenate([hist, tail])
        for dry, wet in [(0.0, 1.0), (0.0, 0.5), (0.25, 1.0)]:
            want = np_reverb(ir, line, frames, dry, wet)
            assert np.array_equal(bits(s2.reverb_reference(ir, line, frames, dry, wet)), bits(want)), ("denormal", dry, wet)
            if not tail.any():                                   # every frame that still sees the history is a denormal, none is flushed
                mag = np.abs(want[:K - 1].astype(np.float64))
                assert ((mag > 0.0) & (mag < 2.0 ** -126)).mean() >= 0.9, (dry, wet)
                assert not bits(want[K - 1:]).any()
        for shift in (0, 3):
            ir, hist = crafted_mixed(K, 43, shift)
            line = np.concatenate([hist, tail])
            want = np_reverb(ir, line, frames, 0.25, 1.0)
            assert np.isfinite(want).all() and 1e20 < np.abs(want).max() < 1e25
            assert np.array_equal(bits(s2.reverb_reference(ir, line, frames, 0.25, 1.0)), bits(want)), ("mixed", shift)


def _new_or_skip(**kw):
    try:
        return s2.Synth(**kw)
    except s2.S2rError as e:
        if e.status == s2s.S2R_ERR_NO_DEVICE:
            return None
        raise


def _p(a):
    return a.ctypes.data_as(s2s._f32p)


def test_range_errors_without_a_handle():
    """every entry looks at the values before it looks at the handle, so the range checks answer without a device; S2R_ERR_INVALID is
    what no handle gets for values in range.  With a device the rest runs on a real handle (check_ranges, also called by
    tests/test_gpu_reverb.py)."""
    L = s2.load_library()
    assert s2.MAX_IR_TAPS == 65536 and s2.IR_SEGMENT == SEG
    ir = np.linspace(1.0, 0.1, 5, dtype=F)
    for dry, wet in BAD_MIX:
        assert L.s2r_set_bus_reverb(None, 0, _p(ir), None, 5, dry, wet) == s2s.S2R_ERR_PATCH_RANGE, (dry, wet)
        assert L.s2r_set_bus_reverb_mix(None, 0, dry, wet) == s2s.S2R_ERR_PATCH_RANGE, (dry, wet)
    for dry, wet in GOOD_MIX:
        assert L.s2r_set_bus_reverb(None, 0, _p(ir), None, 5, dry, wet) == s2s.S2R_ERR_INVALID, (dry, wet)
        assert L.s2r_set_bus_reverb(None, 7, _p(ir), _p(ir), 5, dry, wet) == s2s.S2R_ERR_INVALID, (dry, wet)
        assert L.s2r_set_bus_reverb_mix(None, 7, dry, wet) == s2s.S2R_ERR_INVALID, (dry, wet)
    for bus in (8, 255, 0xffffffff):
        assert L.s2r_set_bus_reverb(None, bus, _p(ir), None, 5, 0.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_reverb(None, bus, None, None, 0, 0.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_reverb_mix(None, bus, 0.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_reverb(None, 0, _p(ir), None, s2.MAX_IR_TAPS + 1, 0.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_reverb(None, 0, None, None, 0xffffffff, 0.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
    for bad in (NAN, INF, -INF):
        tap = ir.copy()
        tap[3] = bad
        assert L.s2r_set_bus_reverb(None, 0, _p(tap), None, 5, 0.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_reverb(None, 0, _p(ir), _p(tap), 5, 0.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_reverb(None, 0, None, None, 5, 0.0, 1.0) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_reverb(None, 0, None, None, 0, 0.0, 1.0) == s2s.S2R_ERR_INVALID
    k, d, w = C.c_uint32(), C.c_float(), C.c_float()
    assert L.s2r_get_bus_reverb(None, 0, C.byref(k), C.byref(d), C.byref(w)) == s2s.S2R_ERR_INVALID
    buf = np.zeros(8, dtype=F)
    assert L.s2r_get_bus_reverb_history(None, 0, _p(buf), 8) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_reverb_history(None, 0, _p(buf), 8) == s2s.S2R_ERR_INVALID
    # the reference
    x, out = np.zeros(4 + 3, dtype=F), np.zeros(3, dtype=F)
    for dry, wet in BAD_MIX:
        assert L.s2r_reverb_reference(_p(ir), 5, _p(x), 3, dry, wet, _p(out)) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_reverb_reference(_p(ir), s2.MAX_IR_TAPS + 1, _p(x), 3, 0.0, 1.0, _p(out)) == s2s.S2R_ERR_PATCH_RANGE
    tap = ir.copy()
    tap[0] = NAN
    assert L.s2r_reverb_reference(_p(tap), 5, _p(x), 3, 0.0, 1.0, _p(out)) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_reverb_reference(None, 5, _p(x), 3, 0.0, 1.0, _p(out)) == s2s.S2R_ERR_INVALID
    assert L.s2r_reverb_reference(_p(ir), 0, _p(x), 3, 0.0, 1.0, _p(out)) == s2s.S2R_ERR_INVALID
    assert L.s2r_reverb_reference(_p(ir), 5, None, 3, 0.0, 1.0, _p(out)) == s2s.S2R_ERR_INVALID
    assert L.s2r_reverb_reference(_p(ir), 5, _p(x), 3, 0.0, 1.0, None) == s2s.S2R_ERR_INVALID
    assert L.s2r_reverb_reference(_p(ir), 5, _p(x), 3, 0.0, 1.0, _p(out)) == s2s.S2R_OK
    with pytest.raises(ValueError):
        s2.reverb_reference(ir, x, 4, 0.0, 1.0)                  # x holds K - 1 + 3 samples
    with pytest.raises(s2.S2rError) as err:
        s2.reverb_reference(ir, x, 3, 1.5, 1.0)
    assert err.value.status == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_abi_version() == 4
    syn = _new_or_skip(num_voices=8, max_frames=64)
    if syn is not None:
        check_ranges(syn)


def check_ranges(syn):
    L, h = syn.L, syn.h
    ir = np.linspace(1.0, 0.1, 5, dtype=F)
    assert all(syn.get_bus_reverb(b) == (0, 0.0, 0.0) for b in range(s2.MAX_BUSES))      # a fresh handle: no reverb anywhere
    for dry, wet in BAD_MIX:
        assert L.s2r_set_bus_reverb(h, 0, _p(ir), None, 5, dry, wet) == s2s.S2R_ERR_PATCH_RANGE, (dry, wet)
    assert L.s2r_set_bus_reverb(h, 8, _p(ir), None, 5, 0.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_reverb(h, 0, _p(ir), None, s2.MAX_IR_TAPS + 1, 0.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
    tap = ir.copy()
    tap[4] = INF
    assert L.s2r_set_bus_reverb(h, 0, _p(tap), None, 5, 0.0, 1.0) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_reverb(h, 0, None, None, 5, 0.0, 1.0) == s2s.S2R_ERR_INVALID
    assert syn.get_bus_reverb(0) == (0, 0.0, 0.0)               # a refused call changes nothing
    buf = np.zeros(16, dtype=F)
    # the mix and the history entries on a bus without a reverb
    assert L.s2r_set_bus_reverb_mix(h, 0, 0.5, 0.5) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_reverb_history(h, 0, _p(buf), 16) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_reverb_history(h, 0, _p(buf), 8) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_bus_reverb_history(h, 8, _p(buf), 16) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_reverb(h, 8, None, None, None) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_get_bus_reverb(h, 0, None, None, None) == s2s.S2R_OK         # any pointer may be null
    syn.clear_bus_reverb(3)                                      # removing what is not there is no error
    syn.set_bus_reverb(3, ir, 0.25, 1.0)
    assert syn.get_bus_reverb(3) == (5, 0.25, 1.0) and syn.get_bus_reverb(0) == (0, 0.0, 0.0)
    hist = syn.bus_reverb_history(3)
    assert hist.shape == (4, 2) and not bits(hist).any()        # +0.0 everywhere right after the reverb is set
    for count in (0, 6, 7, 9, 16):
        assert L.s2r_set_bus_reverb_history(h, 3, _p(buf), count) == s2s.S2R_ERR_INVALID, count
    for cap in (0, 7):
        assert L.s2r_get_bus_reverb_history(h, 3, _p(buf), cap) == s2s.S2R_ERR_INVALID, cap
    assert L.s2r_get_bus_reverb_history(h, 3, _p(buf), 16) == s2s.S2R_OK      # a larger buffer will do
    new = np.arange(8, dtype=F).reshape(4, 2) - F(3.5)
    syn.set_bus_reverb_history(3, new)
    assert np.array_equal(bits(syn.bus_reverb_history(3)), bits(new))
    for dry, wet in BAD_MIX:
        assert L.s2r_set_bus_reverb_mix(h, 3, dry, wet) == s2s.S2R_ERR_PATCH_RANGE
    assert syn.get_bus_reverb(3) == (5, 0.25, 1.0)
    syn.set_bus_reverb_mix(3, 1.0, 0.5)
    assert syn.get_bus_reverb(3) == (5, 1.0, 0.5)
    assert np.array_equal(bits(syn.bus_reverb_history(3)), bits(new))        # the mix keeps the history
    # a reverb belongs to the bus: a new bank and a program change leave it alone
    syn.set_patch_bank([s2.default_patch()] * 3)
    syn.program_change(2)
    assert syn.get_bus_reverb(3) == (5, 1.0, 0.5) and np.array_equal(bits(syn.bus_reverb_history(3)), bits(new))
    syn.set_bus_reverb(3, np.stack([ir, ir[::-1]], axis=1), 0.0, 1.0)        # [K, 2]; setting it again zeroes the history
    assert syn.get_bus_reverb(3) == (5, 0.0, 1.0) and not bits(syn.bus_reverb_history(3)).any()
    syn.set_bus_reverb(7, ir[:1])                                # K = 1: no history at all
    assert syn.get_bus_reverb(7) == (1, 0.0, 1.0) and syn.bus_reverb_history(7).shape == (0, 2)
    syn.set_bus_reverb_history(7, np.zeros((0, 2), dtype=F))
    assert L.s2r_set_bus_reverb_history(h, 7, _p(buf), 2) == s2s.S2R_ERR_INVALID
    with pytest.raises(ValueError):
        syn.set_bus_reverb(0, np.zeros((5, 3), dtype=F))
    with pytest.raises(ValueError):
        syn.set_bus_reverb(0, np.zeros(0, dtype=F))
    syn.clear_bus_reverb(3)
    syn.clear_bus_reverb(7)
    assert all(syn.get_bus_reverb(b) == (0, 0.0, 0.0) for b in range(s2.MAX_BUSES))
