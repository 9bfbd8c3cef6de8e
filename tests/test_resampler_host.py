"""The sample-rate converter's handle-free functions (csrc/s2r_rules.cpp: s2r_resampler_reference, s2r_resampler_count,
s2r_resampler_design) against the numpy binary32 model of the rule that include/s2r.h states (tests/resampler_model.py): the bits of the
outputs, the state and ph; cuts; the answers that need no model; the designer against a float64 restatement and by its response.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import synth2_amd as s2
from synth2_amd import synth as s2s
from resampler_model import MASTER, Model, channels, count_of, design64, response_db

F = np.float32
U = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUTH = json.load(open(os.path.join(ROOT, "profiles", "truth", "resampler_deviation.json")))

# (L, M, T): the ratios of the issue, T 4, and both ends of the table budget (192 x 128 = 24 576 = 320 x 76 + 256)
RATIOS = [(1, 1, 4), (2, 1, 32), (1, 2, 64), (4, 1, 8), (1, 4, 16), (2, 3, 48), (147, 160, 32), (160, 147, 32), (147, 320, 64), (192, 175, 128),
          (320, 147, 76)]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(U)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == F, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaNs"
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), what


def random_table(rng, L, T):
    return rng.uniform(-1.0, 1.0, (L, T)).astype(F)


def signal(rng, nb, n):
    return rng.standard_normal((nb, n, 2)).astype(F), rng.standard_normal((n, 2)).astype(F)


@pytest.mark.parametrize("L,M,T", RATIOS)
def test_reference_is_the_model_on_bits(L, M, T):
    """calls of 0, 1, T - 2, T - 1, T and 1000 frames, the bus count moving among 0, 3 and 8: outputs, count, state and ph"""
    rng = np.random.default_rng(L * 1000 + M)
    table = random_table(rng, L, T)
    m = Model(L, M, table)
    state, ph = None, 0
    empty = 0
    for call, (n, nb) in enumerate(zip([1, 0, T - 2, 1, 1, 1, T - 1, T, 1000, 0, 1, T, 1000], [3, 0, 8, 8, 0, 3, 3, 8, 3, 3, 0, 8, 8])):
        stems, master = signal(rng, nb, n)
        want = m.call(stems, master)
        assert s2.resampler_count(L, M, ph, n) == want.shape[1] == count_of(L, M, ph, n)
        got, state, ph = s2.resampler_reference(stems if nb else None, master, L, M, table, state, ph)
        what = "%d/%d, T %d, call %d of %d frames, %d buses" % (L, M, T, call, n, nb)
        same(got, want, what)
        same(state, m.state, what + ": state")
        assert ph == m.ph and 0 <= ph < M, what
        empty += want.shape[1] == 0 and n > 0
        if n >= T - 1:                                           # the history is the call's last frames, newest first
            same(state, channels(stems, master)[:, ::-1][:, :T - 1], what + ": the history")
    if (L, M) == (1, 4):
        assert empty >= 2                                        # single frames that made nothing


def test_a_stream_cut_three_ways():
    """5000 frames at 147/160 and T 32 in one call, in calls of 250 and in 34 calls of 0 to 1000 frames; and 2/3, 1/4 and 4/1 in
    single frames"""
    rng = np.random.default_rng(5)
    for (L, M, T, total, cuts) in [(147, 160, 32, 5000, None), (2, 3, 8, 300, [1] * 300), (1, 4, 16, 300, [1] * 300), (4, 1, 4, 100, [1] * 100)]:
        table = s2.resampler_design(L, M, T)
        stems, master = signal(rng, 8, total)
        whole, st0, ph0 = s2.resampler_reference(stems, master, L, M, table)
        if cuts is None:
            r = rng.integers(0, 1001, 33).tolist()
            while sum(r) > total:
                r[int(np.argmax(r))] //= 2
            ways = ([250] * 20, r + [total - sum(r)])
            assert len(ways[1]) == 34 and 0 in (ways[1] + [0])
        else:
            ways = (cuts,)
        for way in ways:
            assert sum(way) == total
            state, ph, at, parts = None, 0, 0, []
            for n in way:
                got, state, ph = s2.resampler_reference(stems[:, at:at + n], master[at:at + n], L, M, table, state, ph)
                parts.append(got)
                at += n
            same(np.concatenate(parts, axis=1), whole, "%d/%d cut into %d calls" % (L, M, len(way)))
            same(state, st0, "state")
            assert ph == ph0
        if (L, M) == (4, 1):
            assert whole.shape[1] == 4 * total
        if (L, M) == (1, 4):
            assert whole.shape[1] == total // 4


def test_the_identity_table_returns_the_input():
    """{1, 0, 0, 0} at 1/1: x + 0 + 0 + 0 in the rule's order is x for every finite x but -0.0 (no model in the loop)"""
    rng = np.random.default_rng(6)
    stems, master = signal(rng, 8, 777)
    tiny = (rng.integers(1, 1 << 22, 40).astype(U)).view(F)
    master[5:45, 0] = tiny
    table = np.array([[1.0, 0.0, 0.0, 0.0]], dtype=F)
    got, state, ph = s2.resampler_reference(stems, master, 1, 1, table)
    assert ph == 0 and got.shape == (9, 777, 2)
    assert np.array_equal(bits(got[:8]), bits(stems)) and np.array_equal(bits(got[MASTER]), bits(master))
    assert np.array_equal(bits(state), bits(channels(stems, master)[:, ::-1][:, :3]))


def test_non_finite_denormal_and_negative_zero_inputs():
    rng = np.random.default_rng(7)
    L, M, T = 2, 3, 8
    table = random_table(rng, L, T)
    table[0, 3] = 0.0
    stems, master = signal(rng, 3, 200)
    master[10, 0], master[50, 1], stems[0, 20, 0], stems[1, 30, 1] = np.nan, np.inf, -np.inf, -0.0
    stems[2, 40:80] = (rng.integers(1, 1 << 22, (40, 2)).astype(U) | U(0x80000000)).view(F)
    stems[2, 100:140] = -0.0
    m = Model(L, M, table)
    with np.errstate(invalid="ignore"):
        want = m.call(stems, master)
    got, state, ph = s2.resampler_reference(stems, master, L, M, table)
    same(got, want, "non-finite input")
    same(state, m.state, "state")
    assert np.isnan(got[MASTER, :, 0]).any() and np.isinf(got[MASTER, :, 1]).any() and np.isinf(got[0, :, 0]).any() and np.isfinite(got[2]).all()
    # denormal products are kept: a denormal input through a tap of 0.5 stays a non-zero denormal
    d = np.zeros((50, 2), dtype=F)
    d[:] = np.array([1 << 10], dtype=U).view(F)[0]
    out, _, _ = s2.resampler_reference(None, d, 1, 1, np.array([[0.5, 0.0, 0.0, 0.0]], dtype=F))
    assert (bits(out[MASTER]) == (1 << 9)).all()
    # -0.0 into a sum that starts from +0.0 is +0.0
    z = np.full((10, 2), -0.0, dtype=F)
    out, _, _ = s2.resampler_reference(None, z, 1, 1, np.array([[1.0, 0.0, 0.0, 0.0]], dtype=F))
    assert not bits(out).any()


def test_the_four_chains_are_the_rule_not_the_plain_sum():
    """a table and a signal on which the four chains and the plain ascending sum round differently: the reference is the former"""
    rng = np.random.default_rng(8)
    L, M, T = 3, 2, 16
    table = random_table(rng, L, T)
    stems, master = signal(rng, 8, 400)
    four, plain = Model(L, M, table).call(stems, master), Model(L, M, table, chains=1).call(stems, master)
    assert (bits(four) != bits(plain)).mean() > 0.2
    got, _, _ = s2.resampler_reference(stems, master, L, M, table)
    same(got, four, "the four chains")


def test_refusals():
    Lb = s2.load_library()
    good = np.zeros(320 * 128, dtype=F)
    gp = good.ctypes.data_as(s2s._f32p)
    m = np.zeros((100, 2), dtype=F)
    mp = m.ctypes.data_as(s2s._f32p)
    out = np.full(9 * 2 * 500, 7.0, dtype=F)
    op = out.ctypes.data_as(s2s._f32p)
    n, ph = C.c_size_t(7), C.c_uint32(0)

    def ref(L, M, T, table=gp, stems=None, nb=0, master=mp, frames=100, state=True, php=True, o=op, cap=500, cnt=True, ph0=0):
        st = np.zeros(18 * 127, dtype=F)
        ph.value = ph0
        return Lb.s2r_resampler_reference(L, M, T, table, stems, nb, master, frames, st.ctypes.data_as(s2s._f32p) if state else None,
                                          C.byref(ph) if php else None, o, cap, C.byref(n) if cnt else None)
    R, I = s2s.S2R_ERR_PATCH_RANGE, s2s.S2R_ERR_INVALID
    for L, M, T in [(0, 1, 4), (1, 0, 4), (321, 320, 4), (320, 321, 4), (2, 4, 4), (6, 4, 8), (5, 1, 4), (1, 5, 4), (1, 1, 0), (1, 1, 3), (1, 1, 6), (1, 1, 132),
                    (193, 175, 128), (320, 147, 80)]:
        assert ref(L, M, T) == R, (L, M, T)
        assert Lb.s2r_resampler_design(L, M, T, 10.0, 0.9, gp) == R, (L, M, T)
    for L, M in [(0, 1), (1, 0), (321, 320), (2, 4), (5, 1), (1, 5)]:
        assert Lb.s2r_resampler_count(L, M, 0, 10, C.byref(n)) == R
    assert Lb.s2r_resampler_count(2, 3, 3, 10, C.byref(n)) == R and Lb.s2r_resampler_count(2, 3, 2, 10, None) == I
    for bad in (np.nan, np.inf, 4.5, -4.5):
        t = np.zeros(8, dtype=F)
        t[5] = bad
        assert ref(2, 1, 4, table=t.ctypes.data_as(s2s._f32p)) == R
    assert ref(2, 3, 4, nb=9, stems=mp) == R and ref(2, 3, 4, ph0=3) == R
    assert ref(2, 3, 4, table=None) == I and ref(2, 3, 4, master=None) == I and ref(2, 3, 4, nb=2, stems=None) == I
    assert ref(2, 3, 4, state=False) == I and ref(2, 3, 4, php=False) == I and ref(2, 3, 4, cnt=False) == I and ref(2, 3, 4, o=None) == I
    assert ref(2, 3, 4, cap=66) == I and ref(2, 3, 4, cap=67) == s2s.S2R_OK and n.value == 67
    assert ref(1, 1, 4, frames=0, master=None, o=None, cap=0) == s2s.S2R_OK and n.value == 0
    for beta, roll in [(-0.1, 0.9), (20.5, 0.9), (np.nan, 0.9), (10.0, 0.0), (10.0, 1.01), (10.0, np.nan)]:
        assert Lb.s2r_resampler_design(2, 1, 8, beta, roll, gp) == R
    assert Lb.s2r_resampler_design(2, 1, 8, 10.0, 0.9, None) == I
    assert not good.any() and (out[9 * 2 * 67:] == 7.0).all()         # (the successful call wrote [9][67][2])


@pytest.mark.parametrize("L,M,T", [(147, 160, 32), (2, 1, 32), (1, 2, 64), (320, 147, 76)])
def test_deviation_from_a_float64_sum_stays_within_the_derived_bound(L, M, T):
    """each chain adds T / 4 products, each rounded once, and the tree two more sums: against the exact sum the error of an output is at
    most (T / 4 + 3) * 2^-24 * sum_k |h[p][k]| * max |x| to first order (every partial sum is bounded by sum |h| max |x|)"""
    rng = np.random.default_rng(9)
    table = s2.resampler_design(L, M, T)
    master = rng.uniform(-1.0, 1.0, (1000, 2)).astype(F)
    got, _, _ = s2.resampler_reference(None, master, L, M, table)
    xs = np.concatenate([np.zeros((T - 1, 2)), master.astype(np.float64)])
    u = np.arange(got.shape[1], dtype=np.int64) * M
    n, p = u // L, u % L
    exact = np.zeros((got.shape[1], 2))
    for k in range(T):
        exact += table[p, k].astype(np.float64)[:, None] * xs[T - 1 + n - k]
    bound = (T / 4 + 3) * 2.0 ** -24 * np.abs(table.astype(np.float64)).sum(axis=1)[p] * float(np.abs(master).max())
    err = np.abs(got[MASTER].astype(np.float64) - exact).max(axis=1)
    print("%d/%d T %d: worst deviation %.3g, bound at it %.3g" % (L, M, T, err.max(), bound[int(np.argmax(err))]))
    assert (err <= bound).all()


DESIGNS = [(147, 160, 32, 10.0, 0.9), (160, 147, 32, 10.0, 0.9), (1, 2, 64, 10.0, 0.9), (2, 1, 32, 10.0, 0.9), (2, 3, 48, 10.0, 0.9), (147, 320, 64, 10.0, 0.9),
           (147, 160, 48, 12.0, 0.92)]


@pytest.mark.parametrize("L,M,T,beta,rolloff", DESIGNS + [(1, 1, 4, 0.0, 1.0), (192, 175, 128, 20.0, 0.5), (320, 147, 76, 5.0, 1.0), (4, 1, 8, 3.0, 0.7)])
def test_design_is_the_float64_restatement_within_one_ulp(L, M, T, beta, rolloff):
    table = s2.resampler_design(L, M, T, beta, rolloff)
    _, h = design64(L, M, T, beta, rolloff)
    want = h.astype(F)
    assert table.shape == (L, T) and np.isfinite(table).all() and np.abs(table).max() <= 4.0
    ulp = np.maximum(np.spacing(np.abs(want)), np.spacing(F(2.0 ** -60)))          # (entries below 2^-60 are held to that grid)
    assert (np.abs(table.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    assert np.abs(table.astype(np.float64).sum(axis=1) - 1.0).max() < T * 2.0 ** -24      # no phase has a DC error
    assert np.allclose(table, table[::-1, ::-1], rtol=0.0, atol=2e-7)          # linear phase: h[p][k] = h[L - 1 - p][T - 1 - k]


@pytest.mark.parametrize("L,M,T,beta,rolloff", DESIGNS)
def test_design_by_its_response(L, M, T, beta, rolloff):
    """the interleaved prototype's response from a 2^18-point FFT: the passband up to 0.8 of the lower Nyquist, the stopband from 1.2 of it,
    against what the float64 restatement measured (profiles/truth/resampler_deviation.json) plus 0.05 dB and 3 dB"""
    truth = TRUTH["designs"]["%d/%d T%d beta%g rolloff%g" % (L, M, T, beta, rolloff)]
    hi, lo, stop = response_db(s2.resampler_design(L, M, T, beta, rolloff), L, M)
    print("%d/%d T %d: passband %+.4f / %+.4f dB, stopband %.1f dB (model %+.4f / %+.4f, %.1f)" % (L, M, T, hi, lo, stop, truth["passband_high_db"],
                                                                                                truth["passband_low_db"], truth["stopband_db"]))
    assert hi <= truth["passband_high_db"] + 0.05 and lo >= truth["passband_low_db"] - 0.05
    assert stop <= truth["stopband_db"] + 3.0


def test_a_sine_from_48_to_44_1_khz():
    """1 kHz at 48 kHz through 147/160 sits within 2e-5 of the ideal sine delayed by (L T - 1) / (2 L) input frames, once the history is full"""
    L, M, T = 147, 160, 48
    table = s2.resampler_design(L, M, T, 12.0, 0.92)
    n = np.arange(6000)
    w = 2.0 * np.pi * 1000.0 / 48000.0
    x = np.stack([np.sin(w * n), np.cos(w * n)], axis=1).astype(F)
    got, _, _ = s2.resampler_reference(None, x, L, M, table)
    t = np.arange(got.shape[1]) * (M / L) - (L * T - 1) / (2.0 * L)          # the outputs' positions in input frames
    ideal = np.stack([np.sin(w * t), np.cos(w * t)], axis=1)
    settled = t >= T
    err = np.abs(got[MASTER].astype(np.float64) - ideal)[settled].max()
    print("1 kHz, 48 -> 44.1 kHz: worst deviation %.3g" % err)
    assert settled.sum() > 5000 and err <= 2e-5
