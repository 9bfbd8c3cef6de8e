"""The loudness and true-peak meters, the host side: s2r_loudness_design against the table ITU-R BS.1770 prints and
against the bilinear formulas in numpy float64 (np_design); s2r_loudness_reference — the device rule restated in plain C++ — on bits
against a numpy float32 model of the rule written here (np_loudness: a loop over frames, vectorised over the 18 channels; the true
peak vectorised over frames); s2r_loudness_readings against a numpy float64 model of the host rule (np_readings); and two known
answers, held to the binary64 model of the same rule (f64_loudness) within twice the deviation that tools/loudness_truth.py measured
and committed in profiles/truth/loudness_deviation.json.  Nothing here needs a device."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_gpu_loudness import BLOCK, CALLS, PARITY, T, walker_distances       # (the device file imports without a device)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUTH = os.path.join(ROOT, "profiles", "truth", "loudness_deviation.json")
F = np.float32
CH = s2.LOUDNESS_CHANNELS
# ITU-R BS.1770-4, tables 1 and 2: the pre-filter's two stages at 48 kHz, (b0, b1, b2, a1, a2)
BS1770 = [[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
          [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]]
# the signals of the known answers and of the committed deviations: (name, sample rate, frames)
SIGNALS = [("sine_997_full_scale_left", 48000, 144000), ("sine_fs4_phase_45", 48000, 24000), ("tone_50_minus_40_db", 48000, 96000),
           ("noise", 48000, 96000)]


def _p(a):
    return a.ctypes.data_as(s2s._f32p)


def np_design(sr):
    """the bilinear forms of s2r.h in numpy float64, not rounded"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / sr)
    Vh = np.power(10.0, G / 20.0)
    Vb = np.power(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
             (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    return np.array([shelf, [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]], dtype=np.float64)


def np_taps():
    """g = 4 h from the library's prototype (tests/test_drive_host.py holds s2r_drive_taps to its design)"""
    return (F(4.0) * s2.drive_taps()).astype(F)


def _channels(stems, master, dtype):
    """[frames, 18]: bus b at 2 b, 2 b + 1 (+0.0 past the call's buses), the master at 16, 17"""
    n = master.shape[0]
    v = np.zeros((n, CH), dtype=dtype)
    for b in range(0 if stems is None else stems.shape[0]):
        v[:, 2 * b:2 * b + 2] = stems[b]
    v[:, 16:18] = master
    return v


def np_loudness(coeffs, hop, stems, master, state=None, pos=0, dtype=F):
    """the device rule in numpy, every operation rounded to `dtype` on its own: returns (rows [k, 18], state [122], pos, true_peak [2])"""
    c = np.asarray(coeffs, dtype=dtype).reshape(2, 5)
    master = np.asarray(master, dtype=dtype)
    v = _channels(None if stems is None else np.asarray(stems, dtype=dtype), master, dtype)
    state = np.zeros(s2.LOUDNESS_STATE, dtype=dtype) if state is None else np.array(state, dtype=dtype)
    filt = state[:72].reshape(CH, 2, 2).copy()
    s = [[filt[:, k, 0].copy(), filt[:, k, 1].copy()] for k in range(2)]
    e = state[72:90].copy()
    rows = []
    for n in range(v.shape[0]):
        x = v[n]
        for k in range(2):
            q = c[k]
            y = q[0] * x + s[k][0]
            s[k][0] = ((q[1] * x) - (q[3] * y)) + s[k][1]
            s[k][1] = (q[2] * x) - (q[4] * y)
            x = y
        e = e + x * x
        pos += 1
        if pos == hop:
            rows.append(e)
            e = np.zeros(CH, dtype=dtype)
            pos = 0
    # the true peak: the state's 16 frames, then the call
    g = np_taps().astype(dtype)
    xs = np.concatenate([state[90:].reshape(16, 2), master])
    N = master.shape[0]
    tp = np.zeros(2, dtype=dtype)
    if N:
        tp = np.abs(master).max(axis=0)
        for p in range(4):
            u = np.zeros((N, 2), dtype=dtype)
            for j in range(17):
                if p + 4 * j < s2.DRIVE_TAPS:
                    u = u + g[p + 4 * j] * xs[16 - j:16 - j + N]
            tp = np.maximum(tp, np.abs(u).max(axis=0))
    out = np.empty(s2.LOUDNESS_STATE, dtype=dtype)
    for k in range(2):
        filt[:, k, 0], filt[:, k, 1] = s[k][0], s[k][1]
    out[:72], out[72:90], out[90:] = filt.reshape(-1), e, xs[N:].reshape(-1)
    return np.array(rows, dtype=dtype).reshape(-1, CH), out, pos, tp.astype(dtype)


def np_readings(rows, hop, programme, detail=False):
    """the host rule in numpy float64: (momentary, short-term, integrated); with detail also the counts of blocks, of blocks above the
    absolute gate and of blocks above both"""
    rows = np.asarray(rows, dtype=F).reshape(-1, CH)
    t = rows[:, 2 * programme].astype(np.float64) + rows[:, 2 * programme + 1].astype(np.float64)
    n = len(t)

    def loud(m):
        return -0.691 + 10.0 * math.log10(m) if m > 0.0 else -math.inf

    def block(j):
        return (((t[j - 3] + t[j - 2]) + t[j - 1]) + t[j]) / (4.0 * hop)

    mom = loud(block(n - 1)) if n >= 4 else -math.inf
    short = -math.inf
    if n >= 30:
        acc = 0.0
        for i in range(n - 30, n):
            acc = acc + t[i]
        short = loud(acc / (30.0 * hop))
    ms = [block(j) for j in range(3, n)]
    kept = [m for m in ms if loud(m) > -70.0]
    integ, both = -math.inf, []
    if kept:
        acc = 0.0
        for m in kept:
            acc = acc + m
        rel = loud(acc / len(kept)) - 10.0
        both = [m for m in kept if loud(m) > rel]
        if both:
            acc = 0.0
            for m in both:
                acc = acc + m
            integ = loud(acc / len(both))
    if detail:
        return (mom, short, integ), (len(ms), len(kept), len(both))
    return mom, short, integ


def f64_loudness(coeffs, hop, master):
    """the same rule in binary64 throughout, from the binary32 coefficients and the binary32 taps: (readings of the master, true peak)"""
    rows, _, _, tp = np_loudness(np.asarray(coeffs, dtype=np.float64), hop, None, np.asarray(master, dtype=np.float64), dtype=np.float64)
    t = rows[:, 16] + rows[:, 17]
    n = len(t)
    ms = np.array([(((t[j - 3] + t[j - 2]) + t[j - 1]) + t[j]) / (4.0 * hop) for j in range(3, n)])

    def loud(m):
        return -0.691 + 10.0 * math.log10(m) if m > 0.0 else -math.inf

    ls = np.array([loud(m) for m in ms])
    kept = ms[ls > -70.0]
    integ = -math.inf
    if len(kept):
        rel = loud(kept.mean()) - 10.0
        both = ms[(ls > -70.0) & (ls > rel)]
        integ = loud(both.mean()) if len(both) else -math.inf
    return (loud(ms[-1]) if n >= 4 else -math.inf, loud(t[-30:].sum() / (30.0 * hop)) if n >= 30 else -math.inf, integ), tp


def signal(name, sr, frames):
    """[frames, 2] float32"""
    t = np.arange(frames, dtype=np.float64)
    x = np.zeros((frames, 2), dtype=np.float64)
    if name == "sine_997_full_scale_left":
        x[:, 0] = np.sin(2.0 * np.pi * 997.0 * t / sr)
    elif name == "sine_fs4_phase_45":
        x[:, 0] = x[:, 1] = np.sin(2.0 * np.pi * 0.25 * t + np.pi / 4.0)
    elif name == "tone_50_minus_40_db":
        x[:, 0] = x[:, 1] = 0.01 * np.sin(2.0 * np.pi * 50.0 * t / sr)
    elif name == "noise":
        x[:] = np.random.default_rng(1770).standard_normal((frames, 2)) * 0.1
    else:
        raise ValueError(name)
    return x.astype(F)


def measure(name, sr, frames):
    """the library's binary32 rule beside the binary64 model on one signal: the deviations of the three readings in LU and of the true
    peak relative to the model's (tools/loudness_truth.py commits them; the tests below hold the library to twice each)"""
    c, hop, x = s2.loudness_design(sr), sr // 10, signal(name, sr, frames)
    rows, _, _, tp = s2.loudness_reference(c, hop, None, x)
    got = s2.loudness_readings(rows, hop, s2.MAX_BUSES)
    want, tp64 = f64_loudness(c, hop, x)
    return {"name": name, "sample_rate": sr, "frames": frames, "readings": list(got), "model_readings": list(want),
            "true_peak": [float(v) for v in tp], "model_true_peak": [float(v) for v in tp64],
            "reference_deviation_lu": max(abs(g - w) for g, w in zip(got, want) if not g == w == -math.inf),
            "reference_deviation_true_peak": max(abs(float(g) - float(w)) / float(w) for g, w in zip(tp, tp64) if w > 0.0)}


# ---------------------------------------------------------------- the design

def test_design_at_48_khz_is_the_printed_table():
    """each coefficient is the table's value rounded to binary32: within half a binary32 ulp of it, plus the table's fourteen places"""
    c = s2.loudness_design(48000.0)
    assert c.dtype == F and c.shape == (2, 5)
    for k in range(2):
        for i in range(5):
            want = BS1770[k][i]
            assert abs(float(c[k, i]) - want) <= float(np.spacing(F(abs(want)))) / 2.0 + 5e-15, (k, i, float(c[k, i]), want)
    assert np.abs(np_design(48000.0) - np.array(BS1770)).max() < 2e-14           # the formulas reproduce the table in binary64


@pytest.mark.parametrize("sr", [44100.0, 96000.0, 8000.0, 768000.0])
def test_design_is_the_formula_in_float64(sr):
    """each coefficient equal or adjacent in binary32 to the numpy float64 formulas rounded once: the two libms may differ in the last
    place before the one rounding"""
    got, want = s2.loudness_design(sr), np_design(sr).astype(F)
    for g, w in zip(got.reshape(-1), want.reshape(-1)):
        assert abs(int(np.array(g).view(np.int32)) - int(np.array(w).view(np.int32))) <= 1, (sr, float(g), float(w))


def test_design_range_checks():
    L = s2.load_library()
    buf = np.full(10, 7.0, dtype=F)
    for sr in (float("nan"), float("inf"), -48000.0, 0.0, 7999.9, 768000.1):
        assert L.s2r_loudness_design(sr, _p(buf)) == s2s.S2R_ERR_PATCH_RANGE, sr
    assert L.s2r_loudness_design(48000.0, None) == s2s.S2R_ERR_INVALID
    assert (buf == 7.0).all()
    assert L.s2r_abi_version() == 4


# ---------------------------------------------------------------- the reference against the float32 model

def _stream(frames, nb, seed):
    rng = np.random.default_rng(seed)
    stems = (rng.standard_normal((nb, frames, 2)) * 0.2).astype(F)
    master = (rng.standard_normal((frames, 2)) * 0.5).astype(F)
    return stems, master


def _run(fn, coeffs, hop, stems, master, cuts):
    """the stream in calls of the given lengths: all rows, the final state and position, the call's true peaks"""
    state, pos, at, rows, tps = None, 0, 0, [], []
    for n in cuts:
        st = None if stems is None else stems[:, at:at + n]
        r, state, pos, tp = fn(coeffs, hop, st, master[at:at + n], state, pos)
        rows.append(r), tps.append(tp)
        at += n
    assert at == master.shape[0]
    return np.concatenate(rows), state, pos, tps


@pytest.mark.parametrize("hop", [16, 17, 48, 4800])
def test_reference_is_the_float32_model(hop):
    """calls of 0, 1, 15, 16, 17 frames and one of many hops, state and position carried: rows, state, position and the true peak of
    every call on bits; three buses"""
    c = s2.loudness_design(48000.0)
    cuts = [0, 1, 15, 16, 17, 0, 2 * hop + 5 if hop > 100 else 40 * hop + 3]
    stems, master = _stream(sum(cuts), 3, hop)
    got = _run(s2.loudness_reference, c, hop, stems, master, cuts)
    want = _run(np_loudness, c, hop, stems, master, cuts)
    assert got[2] == want[2] == sum(cuts) % hop and len(want[0]) == sum(cuts) // hop
    assert_bits_equal_finite(got[0], want[0], "rows")
    assert_bits_equal_finite(got[1], want[1], "state")
    for k, (g, w) in enumerate(zip(got[3], want[3])):
        assert_bits_equal_finite(g, w, "true peak of call %d" % k)
    assert (want[0][:, :6] > 0.0).all() and (want[0][:, 16:] > 0.0).all()


def test_a_stream_cut_three_ways_gives_the_same_rows_and_state():
    c = s2.loudness_design(44100.0)
    stems, master = _stream(3000, 8, 5)
    runs = [_run(s2.loudness_reference, c, 100, stems, master, cuts) for cuts in ([3000], [1, 999, 1000, 1000], [99, 100, 101, 2700])]
    assert len(runs[0][0]) == 30
    for r in runs[1:]:
        assert_bits_equal_finite(r[0], runs[0][0], "rows")
        assert_bits_equal_finite(r[1], runs[0][1], "state")
        assert r[2] == runs[0][2] == 0
    # the true peak of the whole is the maximum of the parts'
    for r in runs[1:]:
        assert_bits_equal_finite(np.max(r[3], axis=0), runs[0][3][0], "true peak")


def test_two_buses_leave_programmes_2_to_7_on_zeros():
    """a call of n_buses = 2 feeds +0.0 to buses 2 .. 7: from the initial state their rows and filter values are +0.0 in every bit; from
    a state that holds values their filters ring down as the model says"""
    c = s2.loudness_design(48000.0)
    stems, master = _stream(500, 2, 9)
    rows, state, pos, _ = s2.loudness_reference(c, 48, stems, master)
    assert len(rows) == 10 and pos == 20
    assert not rows[:, 4:16].view(np.uint32).any() and not state[16:64].view(np.uint32).any() and not state[72 + 4:72 + 16].view(np.uint32).any()
    assert (rows[:, :4] > 0.0).all() and (rows[:, 16:] > 0.0).all()
    stems8, master8 = _stream(300, 8, 10)
    _, state8, pos8, _ = s2.loudness_reference(c, 48, stems8, master8)
    got = s2.loudness_reference(c, 48, stems, master, state8, pos8)
    want = np_loudness(c, 48, stems, master, state8, pos8)
    assert_bits_equal_finite(got[0], want[0], "rows")
    assert_bits_equal_finite(got[1], want[1], "state")
    assert (got[0][:, 4:16] > 0.0).any()                         # the ring-down of what the eight-bus call left


def test_reference_refusals_touch_nothing():
    L = s2.load_library()
    c = np.ascontiguousarray(s2.loudness_design(48000.0)).reshape(-1)
    bad = c.copy()
    bad[2] = np.inf
    state, master, stems, rows, tp = np.full(122, 3.0, dtype=F), np.ones(2 * 16, dtype=F), np.ones(2 * 16, dtype=F), np.full(18, 3.0, dtype=F), np.full(2, 3.0, dtype=F)
    pos, n = C.c_uint32(5), C.c_size_t(77)

    def call(cp=c, hop=16, st=stems, nb=1, ms=master, frames=16, sp=state, pp=C.byref(pos), rp=rows, cap=18, np_=C.byref(n)):
        return L.s2r_loudness_reference(None if cp is None else _p(cp), hop, None if st is None else _p(st), nb, None if ms is None else _p(ms), frames,
                                        None if sp is None else _p(sp), pp, None if rp is None else _p(rp), cap, np_, _p(tp))

    assert call(hop=15) == s2s.S2R_ERR_PATCH_RANGE and call(hop=(1 << 20) + 1) == s2s.S2R_ERR_PATCH_RANGE
    assert call(cp=bad) == s2s.S2R_ERR_PATCH_RANGE and call(nb=9) == s2s.S2R_ERR_PATCH_RANGE
    pos.value = 16
    assert call() == s2s.S2R_ERR_PATCH_RANGE
    pos.value = 5
    for kw in (dict(cp=None), dict(st=None), dict(ms=None), dict(sp=None), dict(pp=None), dict(np_=None), dict(cap=17), dict(rp=None)):
        assert call(**kw) == s2s.S2R_ERR_INVALID, kw
    assert (state == 3.0).all() and (rows == 3.0).all() and (tp == 3.0).all() and pos.value == 5 and n.value == 77
    assert call() == s2s.S2R_OK and n.value == 1 and pos.value == 5 and not (rows == 3.0).any()


# ---------------------------------------------------------------- what the device matrix meets of the walkers' schedule

def test_the_parity_matrix_meets_the_walkers_block_boundary():
    """The kernel's walkers take a block of eight frames without a hop test when hop - pos > 8 (s2r_loudness.hip).  A distance of
    exactly 8 — the hop ends on the block's last frame — is the one value at which `>` and `>=` differ, and a wrong comparison there
    loses the hop for good: pos steps past hop.  Replayed on the books over the matrix's calls (test_gpu_loudness.walker_distances),
    hop 17 starts a full block at every distance from 1 to 9 and at some beyond, and the matrix runs it with all eight buses fed; the
    matrix's other hops never meet 8, which is why 17 is in it."""
    met = {hop: walker_distances(hop, CALLS)[0] for _, hop in PARITY}
    assert met[17] >= set(range(1, 10)) and max(met[17]) > 9, sorted(met[17])
    assert any(nb == s2.MAX_BUSES and BLOCK in met[hop] for nb, hop in PARITY)
    assert all(BLOCK not in met[hop] for hop in (16, 48, 100, 4800))
    assert (s2.MAX_BUSES, 16) in PARITY                          # the smallest hop with all 18 lanes fed
    # the replay itself: a call shorter than a block has none, a tile's tail is walked frame by frame, pos is carried
    assert walker_distances(17, [7]) == (set(), 0, 7)
    assert walker_distances(17, [8, 8, 8]) == ({17, 9, 1}, 3, 7)
    assert walker_distances(16, [T + 9]) == ({16, 8}, T // BLOCK + 1, 9) and walker_distances(100, [T + 9], 99)[0] >= {1, 93, 5}
    blocks = sum(n // T * (T // BLOCK) + n % T // BLOCK for n in CALLS)
    assert all(walker_distances(hop, CALLS)[1:] == (blocks, sum(CALLS) % hop) for _, hop in PARITY)


# ---------------------------------------------------------------- the readings against the float64 model

def _rows(levels, hop, programme=s2.MAX_BUSES):
    """hop rows whose two channels of one programme carry the given mean squares, split 3 : 1 between L and R"""
    rows = np.zeros((len(levels), CH), dtype=F)
    ms = np.asarray(levels, dtype=np.float64) * hop
    rows[:, 2 * programme], rows[:, 2 * programme + 1] = 0.75 * ms, 0.25 * ms
    return rows


def _close(got, want):
    for g, w in zip(got, want):
        assert g == w or abs(g - w) <= 1e-12, (got, want)        # (one log10 of each libm: the last place may differ)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 29, 30, 31, 64])
def test_readings_with_few_hops(n):
    rng = np.random.default_rng(n)
    rows = _rows(10.0 ** rng.uniform(-3.0, -1.0, n), 4800, 2)
    got = s2.loudness_readings(rows, 4800, 2)
    _close(got, np_readings(rows, 4800, 2))
    assert (got[0] == -math.inf) == (n < 4) and (got[1] == -math.inf) == (n < 30) and (got[2] == -math.inf) == (n < 4)
    assert s2.loudness_readings(rows, 4800, 3) == (-math.inf,) * 3            # another programme: silence


def test_readings_of_silence():
    rows = np.zeros((40, CH), dtype=F)
    assert s2.loudness_readings(rows, 48, 8) == (-math.inf, -math.inf, -math.inf)
    assert np_readings(rows, 48, 8) == (-math.inf, -math.inf, -math.inf)


def test_both_gates_remove_blocks():
    """a programme of 20 loud hops at a mean square of 0.1, 20 at 0.001 (20 dB below: under the relative gate, above the absolute one)
    and 20 at 1e-9 (under the absolute gate at -70): asserted on the model, both gates remove blocks, and the integrated reading is the
    loud section's, not the mean's"""
    levels = [0.1] * 20 + [1e-3] * 20 + [1e-9] * 20
    rows = _rows(levels, 4800)
    want, (blocks, kept, both) = np_readings(rows, 4800, 8, detail=True)
    assert blocks == 57 and blocks > kept > both > 0, (blocks, kept, both)
    got = s2.loudness_readings(rows, 4800, 8)
    _close(got, want)
    assert abs(got[2] - (-0.691 + 10.0 * math.log10(0.1))) < 0.5 and got[0] < -70.0 and got[2] > got[1]
    ungated = -0.691 + 10.0 * math.log10(np.mean(levels))
    assert got[2] > ungated + 2.0


def test_the_window_of_hops():
    """what a handle that keeps max_hops = 32 rows reads: the readings over the last 32 rows alone"""
    rng = np.random.default_rng(32)
    rows = _rows(10.0 ** rng.uniform(-4.0, -0.5, 100), 480, 0)
    for n in (31, 32, 33, 100):
        window = rows[:n][-32:]
        _close(s2.loudness_readings(window, 480, 0), np_readings(window, 480, 0))
    assert s2.loudness_readings(rows[-32:], 480, 0)[2] != s2.loudness_readings(rows, 480, 0)[2]


def test_readings_refusals():
    L = s2.load_library()
    rows, out = np.ones(18, dtype=F), (C.c_double * 3)(2.0, 2.0, 2.0)
    assert L.s2r_loudness_readings(_p(rows), 1, 15, 0, out) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_loudness_readings(_p(rows), 1, (1 << 20) + 1, 0, out) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_loudness_readings(_p(rows), 1, 16, 9, out) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_loudness_readings(None, 1, 16, 0, out) == s2s.S2R_ERR_INVALID
    assert L.s2r_loudness_readings(_p(rows), 1, 16, 0, None) == s2s.S2R_ERR_INVALID
    assert list(out) == [2.0, 2.0, 2.0]


# ---------------------------------------------------------------- known answers

def test_the_committed_bounds_are_the_measurement():
    """profiles/truth/loudness_deviation.json lists these signals, and each bound is twice the deviation recorded beside it; the
    deviations are binary32's against binary64: below 1e-3 LU and 1e-5 of the true peak"""
    doc = json.load(open(TRUTH))
    assert [(r["name"], r["sample_rate"], r["frames"]) for r in doc["signals"]] == SIGNALS
    for r in doc["signals"]:
        assert r["bound_lu"] == 2.0 * r["reference_deviation_lu"] and 0.0 <= r["reference_deviation_lu"] < 1e-3, r
        assert r["bound_true_peak"] == 2.0 * r["reference_deviation_true_peak"] and 0.0 <= r["reference_deviation_true_peak"] < 1e-5, r


@pytest.mark.parametrize("i", range(len(SIGNALS)))
def test_the_binary32_rule_is_within_twice_its_measured_deviation_of_binary64(i):
    row = json.load(open(TRUTH))["signals"][i]
    m = measure(*SIGNALS[i])
    print("%s: readings %s, model %s; deviation %.3e LU (bound %.3e), true peak %.3e (bound %.3e)" % (
        m["name"], m["readings"], m["model_readings"], m["reference_deviation_lu"], row["bound_lu"], m["reference_deviation_true_peak"],
        row["bound_true_peak"]))
    assert m["reference_deviation_lu"] <= row["bound_lu"] and m["reference_deviation_true_peak"] <= row["bound_true_peak"]


def test_a_997_hz_sine_at_full_scale_reads_minus_3_01_lkfs():
    """BS.1770: a 997 Hz sine at 0 dB FS in one channel reads -3.01 LKFS.  The binary64 model of the rule reads it to the two places
    the recommendation states; the library's binary32 rule is within its committed bound of the model"""
    row = json.load(open(TRUTH))["signals"][0]
    m = measure(*SIGNALS[0])
    for got, want in zip(m["readings"], m["model_readings"]):
        assert abs(want - (-3.01)) < 0.005 and abs(got - want) <= row["bound_lu"], (got, want)


def test_an_fs4_sine_at_45_degrees_has_a_true_peak_near_1():
    """a sine at a quarter of the sample rate with a phase of 45 degrees: every sample is +-0.7071, the peaks lie between them.  In
    the steady state — a second call, behind the first call's onset — the 4x interpolated peak is 0.9999 of full scale"""
    sr, frames = SIGNALS[1][1], SIGNALS[1][2]
    c, x = s2.loudness_design(sr), signal(*SIGNALS[1])
    _, state, pos, _ = s2.loudness_reference(c, sr // 10, None, x[:frames // 2])
    _, _, _, tp = s2.loudness_reference(c, sr // 10, None, x[frames // 2:], state, pos)
    row = json.load(open(TRUTH))["signals"][1]
    _, _, _, tp64 = np_loudness(c.astype(np.float64), sr // 10, None, x[frames // 2:].astype(np.float64), state.astype(np.float64), pos, dtype=np.float64)
    print("sample peak %.6f, true peak %.6f (binary64 model %.6f)" % (np.abs(x).max(), tp[0], tp64[0]))
    assert abs(float(np.abs(x).max()) - math.sqrt(0.5)) < 1e-7
    assert abs(tp64[0] - 1.0) < 1e-3 and (np.abs(tp.astype(np.float64) - tp64) <= row["bound_true_peak"] * tp64).all()
