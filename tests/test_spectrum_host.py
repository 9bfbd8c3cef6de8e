"""The spectrum meter's host functions (s2r.h: s2r_set_master_spectrum), without a device: the twiddle and window tables,
s2r_spectrum_reference against a numpy float32 model of the rule — one vectorised statement per operation of a radix-2 layer, so
that every operation is rounded on its own —, its deviation from a float64 FFT, the readings and band readings against float64 numpy
models, and every refusal the header lists."""
import json
import math
import os

import numpy as np
import pytest

import synth2_amd as s2

F = np.float32
P = s2.SPECTRUM_PROGRAMMES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVIATION = os.path.join(ROOT, "profiles", "truth", "spectrum_deviation.json")


SIZES = (256, 512, 1024, 2048, 4096, 8192)                       # every size the meter takes: log2 N of 8 .. 13, each its own split into passes on the device


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def same_bits(got, want, what):
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    assert got.shape == want.shape, what
    assert np.array_equal(bits(got), bits(want)), what


def bitrev(n):
    L = n.bit_length() - 1
    i = np.arange(n)
    r = np.zeros(n, dtype=np.int64)
    for b in range(L):
        r |= ((i >> b) & 1) << (L - 1 - b)
    return r


def model_row(window, tw, x):
    """the rule in numpy float32: x [N, 2], oldest first; returns p [N / 2 + 1]"""
    n = len(window)
    zr, zi = (window * x[:, 0]).astype(F), (window * x[:, 1]).astype(F)
    r = bitrev(n)
    vr, vi = np.empty(n, dtype=F), np.empty(n, dtype=F)
    vr[r], vi[r] = zr, zi
    m = 2
    while m <= n:
        h = m // 2
        j = np.arange(h)
        wr, wi = tw[j * (n // m), 0], tw[j * (n // m), 1]
        ar, ai = vr.reshape(-1, m)[:, :h], vi.reshape(-1, m)[:, :h]
        br, bi = vr.reshape(-1, m)[:, h:], vi.reshape(-1, m)[:, h:]
        p0, p1, p2, p3 = wr * br, wi * bi, wr * bi, wi * br
        tr, ti = p0 - p1, p2 + p3
        nr = np.concatenate([ar + tr, ar - tr], axis=1)
        ni = np.concatenate([ai + ti, ai - ti], axis=1)
        assert nr.dtype == F and ni.dtype == F
        vr, vi = nr.reshape(-1), ni.reshape(-1)
        m *= 2
    k = np.arange(n // 2 + 1)
    kk = (n - k) % n
    sa = vr[k] * vr[k] + vi[k] * vi[k]
    sb = vr[kk] * vr[kk] + vi[kk] * vi[kk]
    return ((sa + sb) * F(0.5)).astype(F)


class Model:
    """the stream of the rule in numpy: state [9, N, 2], pos; feed() returns the rows of a call"""

    def __init__(self, n, hop, window):
        self.n, self.hop, self.w, self.tw = n, hop, np.asarray(window, dtype=F), s2.spectrum_twiddles(n)
        self.state, self.pos = np.zeros((P, n, 2), dtype=F), 0

    def feed(self, stems, master):
        frames, nb = len(master), 0 if stems is None else len(stems)
        made = (self.pos + frames) // self.hop
        rows = np.zeros((made, P, self.n // 2 + 1), dtype=F)
        for p in range(P):
            fed = p == 8 or p < nb
            call = master if p == 8 else (stems[p] if fed else np.zeros((frames, 2), dtype=F))
            x = np.concatenate([self.state[p], call])
            for r in range(made):
                first = (r + 1) * self.hop - self.pos
                if fed:
                    rows[r, p] = model_row(self.w, self.tw, x[first:first + self.n])
            self.state[p] = x[frames:]
        self.pos = (self.pos + frames) % self.hop
        return rows


def stream(rng, nb, frames):
    stems = rng.uniform(-1, 1, (nb, frames, 2)).astype(F)
    master = rng.uniform(-1, 1, (frames, 2)).astype(F)
    return stems, master


def run_reference(n, hop, window, stems, master, cuts):
    """the stream through s2r_spectrum_reference in calls of `cuts` frames (cycled): (rows, state, pos)"""
    state, pos, at, rows, i = None, 0, 0, [], 0
    while at < len(master):
        c = min(cuts[i % len(cuts)], len(master) - at)
        r, state, pos = s2.spectrum_reference(n, hop, window, stems[:, at:at + c], master[at:at + c], state, pos)
        rows.append(r)
        at += c
        i += 1
    return np.concatenate(rows), state, pos


@pytest.mark.parametrize("n", SIZES)
def test_twiddles(n):
    t = s2.spectrum_twiddles(n)
    assert t.shape == (n // 2, 2) and t.dtype == F
    assert t[0, 0] == 1.0 and t[0, 1] == 0.0 and not np.signbit(t[0, 1])
    assert t[n // 4, 0] == 0.0 and t[n // 4, 1] == -1.0
    q = n // 4
    j = np.arange(n // 8 + 1, q + 1)
    same_bits(t[j, 0], -t[q - j, 1], "re, second octant")
    same_bits(t[j, 1], -t[q - j, 0], "im, second octant")
    j = np.arange(q + 1, n // 2)
    same_bits(t[j, 0], t[j - q, 1], "re, second quadrant")
    same_bits(t[j, 1], -t[j - q, 0], "im, second quadrant")
    j = np.arange(n // 2)
    c, s = np.cos(2 * np.pi * j / n), -np.sin(2 * np.pi * j / n)
    for got, want in ((t[:, 0], c), (t[:, 1], s)):
        ulp = np.spacing(np.abs(got).astype(F)).astype(np.float64)
        near = np.abs(want) > 1e-12                              # (float64 cos at a quarter turn is 6e-17, the table's exact 0 is nearer the truth)
        assert (np.abs(got.astype(np.float64) - want)[near] <= 0.5 * ulp[near] * (1 + 1e-6)).all()
        assert (got[~near] == 0.0).all()


@pytest.mark.parametrize("n", [256, 1024, 8192])
def test_windows(n):
    x = 2 * np.pi * np.arange(n) / n
    want = {"rect": np.ones(n), "hann": 0.5 - 0.5 * np.cos(x), "hamming": 0.54 - 0.46 * np.cos(x),
            "blackman-harris": 0.35875 - 0.48829 * np.cos(x) + 0.14128 * np.cos(2 * x) - 0.01168 * np.cos(3 * x)}
    for kind, w in want.items():
        got = s2.spectrum_window(kind, n)
        assert got.dtype == F and got.shape == (n,)
        # (libm's cos and numpy's may differ in the last place of binary64: one binary32 place at a rounding tie at most)
        assert (np.abs(got.astype(np.float64) - w) <= 0.5 * np.spacing(np.abs(got)).astype(np.float64) * (1 + 1e-6) + 1e-16).all(), kind
    same_bits(s2.spectrum_window(s2.WINDOW_HANN, n), s2.spectrum_window("hann", n), "kinds by number")


CASES = [(n, hop) for n in SIZES for hop in (n // 8, n // 2, n, n + 37)]


@pytest.mark.parametrize("n,hop", CASES)
def test_reference_is_the_numpy_model(n, hop):
    """random window (not symmetric), L != R, three buses: rows and state on bits, the stream cut into calls of 1, hop - 1, hop + 1
    and N + 3 frames in turn"""
    rng = np.random.default_rng(n * 7 + hop)
    window = rng.uniform(-1, 1, n).astype(F)
    total = n + 3 + 2 * hop + 1 if n >= 2048 else 2 * (n + 3) + 3 * hop
    stems, master = stream(rng, 3, total)
    cuts = [1, hop - 1, hop + 1, n + 3]
    m, at, i = Model(n, hop, window), 0, 0
    state, pos, n_rows = None, 0, 0
    while at < total:
        c = min(cuts[i % 4], total - at)
        want = m.feed(stems[:, at:at + c], master[at:at + c])
        got, state, pos = s2.spectrum_reference(n, hop, window, stems[:, at:at + c], master[at:at + c], state, pos)
        same_bits(got, want, "rows of call %d" % i)
        same_bits(state, m.state, "state after call %d" % i)
        assert pos == m.pos
        assert not bits(got[:, 3:8]).any()                       # buses past n_buses: +0.0
        n_rows += len(got)
        at += c
        i += 1
    assert n_rows == total // hop and n_rows >= 1


def test_cuts_do_not_matter():
    n, hop = 512, 200
    rng = np.random.default_rng(5)
    window = rng.uniform(0, 1, n).astype(F)
    stems, master = stream(rng, 2, 3000)
    whole = run_reference(n, hop, window, stems, master, [3000])
    for cuts in ([1, 7, 300], [hop], [511, 513, 64]):
        got = run_reference(n, hop, window, stems, master, cuts)
        same_bits(got[0], whole[0], "rows")
        same_bits(got[1], whole[1], "state")
        assert got[2] == whole[2]
    assert len(whole[0]) == 15


def test_a_bus_count_that_changes_keeps_the_history():
    n, hop = 256, 64
    rng = np.random.default_rng(6)
    window = s2.spectrum_window("hann", n)
    stems, master = stream(rng, 4, 400)
    m = Model(n, hop, window)
    state, pos = None, 0
    for nb, (a, b) in zip((4, 1, 3), ((0, 150), (150, 230), (230, 400))):
        want = m.feed(stems[:nb, a:b], master[a:b])
        got, state, pos = s2.spectrum_reference(n, hop, window, stems[:nb, a:b], master[a:b], state, pos)
        same_bits(got, want, "rows")
        same_bits(state, m.state, "state")


def deviation_cases():
    """the cases of tools/spectrum_truth.py: (name, n, hop, window kind)"""
    return [("n%d_%s" % (n, kind), n, n // 2, kind) for n in (256, 2048, 8192) for kind in ("hann", "blackman-harris")]


def measure_deviation(n, hop, kind):
    """the largest |p - truth| / max(truth) over the rows of a seeded stream, the truth numpy's float64 FFT of the same windowed frames"""
    rng = np.random.default_rng(n)
    window = s2.spectrum_window(kind, n)
    stems, master = stream(rng, 1, 2 * n)
    rows, _, _ = s2.spectrum_reference(n, hop, window, stems, master)
    worst = 0.0
    for r in range(len(rows)):
        end = (r + 1) * hop
        for p, src in ((0, stems[0]), (8, master)):
            x = np.concatenate([np.zeros((n, 2)), src.astype(np.float64)])[end:end + n]
            z = np.fft.fft(window.astype(np.float64) * x[:, 0] + 1j * window.astype(np.float64) * x[:, 1])
            k = np.arange(n // 2 + 1)
            truth = (np.abs(z[k]) ** 2 + np.abs(z[(n - k) % n]) ** 2) * 0.5
            worst = max(worst, float(np.max(np.abs(rows[r, p].astype(np.float64) - truth)) / truth.max()))
    return worst


def test_deviation_from_the_float64_truth():
    with open(DEVIATION) as f:
        committed = json.load(f)["cases"]
    for name, n, hop, kind in deviation_cases():
        got = measure_deviation(n, hop, kind)
        print(name, got, committed[name])
        assert got <= 2.0 * committed[name], name
        assert committed[name] < n.bit_length() * 2.0 ** -21     # (a committed figure that is an error of the transform, not of the test)


def committed_db_bound():
    """what the committed deviation allows a full-scale bin to read off, in dB"""
    with open(DEVIATION) as f:
        worst = max(json.load(f)["cases"].values())
    return 10 * math.log10(1 + 2 * worst) + 1e-9


def model_q(rows, window, programme, n_avg):
    n = len(window)
    s1 = 0.0
    for w in window.astype(np.float64):
        s1 = s1 + w
    p = rows[len(rows) - n_avg:, programme].astype(np.float64)
    total = np.zeros(n // 2 + 1)
    for r in p:
        total = total + r
    c = np.full(n // 2 + 1, 2.0)
    c[0] = c[-1] = 0.5
    return c * (total / n_avg) / (s1 * s1)


def model_bands(q, n, sample_rate, bpo):
    df = sample_rate / n
    out, centres = [], []
    for i in range(-64 * bpo, 64 * bpo + 1):
        fc = 1000.0 * 2.0 ** (i / bpo)
        lo, hi = fc * 2.0 ** (-1 / (2 * bpo)), fc * 2.0 ** (1 / (2 * bpo))
        if not (lo >= df and hi <= sample_rate / 2):
            continue
        power = 0.0
        for k in range(n // 2 + 1):
            a, b = max(lo, (k - 0.5) * df), min(hi, (k + 0.5) * df)
            if b > a:
                power = power + q[k] * ((b - a) / df)
        out.append(power)
        centres.append(fc)
    return np.array(out), np.array(centres)


def test_readings_are_the_float64_model():
    n, hop = 512, 256
    rng = np.random.default_rng(9)
    window = s2.spectrum_window("hamming", n)
    stems, master = stream(rng, 2, 5 * hop)
    rows, _, _ = s2.spectrum_reference(n, hop, window, stems, master)
    assert len(rows) == 5
    for programme, n_avg in ((0, 1), (1, 3), (8, 5)):
        q = model_q(rows, window, programme, n_avg)
        got = s2.spectrum_readings(rows, window, programme, n_avg)
        np.testing.assert_allclose(got, 10 * np.log10(q), rtol=0, atol=1e-11)
        for bpo in (1, 3, 6, 12):
            db, fc = s2.spectrum_band_readings(rows, window, programme, 48000.0, bpo, n_avg)
            power, centres = model_bands(q, n, 48000.0, bpo)
            np.testing.assert_allclose(fc, centres, rtol=1e-14)
            np.testing.assert_allclose(db, 10 * np.log10(power), rtol=0, atol=1e-10)
    with np.errstate(divide="ignore"):
        assert (s2.spectrum_readings(rows, window, 5, 1) == -np.inf).all()       # a bus that was not fed: silence
        assert (s2.spectrum_band_readings(rows, window, 5, 48000.0, 3)[0] == -np.inf).all()


@pytest.mark.parametrize("kind", ["hann", "blackman-harris", "rect"])
def test_a_sine_reads_0_db_and_one_channel_3_db_less(kind):
    n = 2048
    window = s2.spectrum_window(kind, n)
    t = np.arange(n)
    tol = committed_db_bound() + 1e-6                            # (the input's own rounding to binary32: 6e-8 relative, 3e-7 dB)
    for k in (5, 37, n // 4, n // 2 - 5):                      # (2 k clear of the window's own bins 0 .. 3, so the mirror term vanishes)
        sine = np.sin(2 * np.pi * k * t / n + 0.3).astype(F)
        both = np.stack([sine, sine], axis=1)
        one = np.stack([sine, np.zeros(n, dtype=F)], axis=1)
        for master, want in ((both, 0.0), (one, 10 * math.log10(0.5))):
            rows, _, _ = s2.spectrum_reference(n, n, window, None, master)
            db = s2.spectrum_readings(rows, window, 8, 1)
            assert abs(db[k] - want) <= tol, (kind, k, db[k], want)
    dc = np.ones((n, 2), dtype=F)
    rows, _, _ = s2.spectrum_reference(n, n, window, None, dc)
    assert abs(s2.spectrum_readings(rows, window, 8, 1)[0]) <= tol
    rows, _, _ = s2.spectrum_reference(n, n, window, None, np.zeros((n, 2), dtype=F))
    with np.errstate(divide="ignore"):
        assert (s2.spectrum_readings(rows, window, 8, 1) == -np.inf).all()


@pytest.mark.parametrize("bpo,count,lowest,highest", [(1, 9, -4, 4), (3, 29, -15, 13), (6, 59, -31, 27), (12, 119, -64, 54)])
def test_band_counts_and_centres_at_48k_2048(bpo, count, lowest, highest):
    """48 kHz, N = 2048: bins of 23.4375 Hz.  The lowest band kept is the first whose lower edge 1000 * 2^((i - 1/2) / bpo) reaches
    23.4375 Hz, i >= bpo * log2(0.0234375) + 1/2 = -5.415 bpo + 1/2; the highest the last whose upper edge stays within 24 kHz,
    i <= bpo * log2(24) - 1/2 = 4.585 bpo - 1/2."""
    assert lowest == math.ceil(bpo * math.log2(0.0234375) + 0.5) and highest == math.floor(bpo * math.log2(24.0) - 0.5)
    assert count == highest - lowest + 1
    n = 2048
    rng = np.random.default_rng(bpo)
    window = s2.spectrum_window("hann", n)
    noise = rng.uniform(-1, 1, (n, 2)).astype(F)
    rows, _, _ = s2.spectrum_reference(n, n, window, None, noise)
    db, fc = s2.spectrum_band_readings(rows, window, 8, 48000.0, bpo)
    assert len(db) == len(fc) == count
    np.testing.assert_allclose(fc, 1000.0 * 2.0 ** (np.arange(lowest, highest + 1) / bpo), rtol=1e-14)
    # white noise: the bands tile [lower edge of the first, upper edge of the last], so their powers add up to q times the covered fractions
    q = model_q(rows, window, 8, 1)
    df = 48000.0 / n
    lo, hi = fc[0] * 2.0 ** (-1 / (2 * bpo)), fc[-1] * 2.0 ** (1 / (2 * bpo))
    k = np.arange(n // 2 + 1)
    frac = np.clip(np.minimum(hi, (k + 0.5) * df) - np.maximum(lo, (k - 0.5) * df), 0, None) / df
    np.testing.assert_allclose(np.sum(10 ** (db / 10)), np.sum(q * frac), rtol=1e-12)


def rc_of(call):
    with pytest.raises(s2.S2rError) as e:
        call()
    return e.value.status


def test_refusals_of_the_pure_functions():
    from synth2_amd import synth as s2s
    RANGE, INVALID = s2s.S2R_ERR_PATCH_RANGE, s2s.S2R_ERR_INVALID
    L = s2.load_library()
    w = s2.spectrum_window("hann", 256)
    master = np.zeros((10, 2), dtype=F)
    for n in (0, 128, 255, 300, 16384):
        assert rc_of(lambda: s2.spectrum_window("hann", n)) == RANGE
        assert rc_of(lambda: s2.spectrum_twiddles(n)) == RANGE
    assert rc_of(lambda: s2.spectrum_window(4, 256)) == RANGE
    assert L.s2r_spectrum_window(1, 256, None) == INVALID and L.s2r_spectrum_twiddles(256, None) == INVALID
    for hop in (0, 31, (1 << 20) + 1):
        assert rc_of(lambda: s2.spectrum_reference(256, hop, w, None, master)) == RANGE
    s2.spectrum_reference(256, 32, w, None, master)
    s2.spectrum_reference(256, 1 << 20, w, None, master)
    assert rc_of(lambda: s2.spectrum_reference(2048, 255, s2.spectrum_window("hann", 2048), None, master)) == RANGE
    for bad in (np.nan, np.inf, -np.inf):
        wb = w.copy()
        wb[255] = bad
        assert rc_of(lambda: s2.spectrum_reference(256, 32, wb, None, master)) == RANGE
    assert rc_of(lambda: s2.spectrum_reference(256, 32, w, np.zeros((9, 10, 2), dtype=F), master)) == RANGE
    assert rc_of(lambda: s2.spectrum_reference(256, 32, w, None, master, None, 32)) == RANGE
    # a row buffer too small, checked before anything is changed
    import ctypes as C
    fp = C.POINTER(C.c_float)
    state, pos, n_rows = np.ones(18 * 256, dtype=F), C.c_uint32(30), C.c_size_t(7)
    rows = np.zeros(9 * 129 - 1, dtype=F)
    rc = L.s2r_spectrum_reference(256, 32, w.ctypes.data_as(fp), None, 0, master.ctypes.data_as(fp), 10, state.ctypes.data_as(fp), C.byref(pos),
                                  rows.ctypes.data_as(fp), rows.size, C.byref(n_rows))
    assert rc == INVALID and (state == 1).all() and pos.value == 30 and n_rows.value == 7
    rc = L.s2r_spectrum_reference(256, 32, None, None, 0, master.ctypes.data_as(fp), 10, state.ctypes.data_as(fp), C.byref(pos), rows.ctypes.data_as(fp),
                                  rows.size, C.byref(n_rows))
    assert rc == INVALID
    good = np.zeros((2, 9, 129), dtype=F)
    assert rc_of(lambda: s2.spectrum_readings(good, w, 9, 1)) == RANGE
    assert rc_of(lambda: s2.spectrum_readings(good, w, 0, 0)) == RANGE
    assert rc_of(lambda: s2.spectrum_readings(good, w, 0, 3)) == RANGE
    for bpo in (0, 2, 4, 24):
        assert rc_of(lambda: s2.spectrum_band_readings(good, w, 0, 48000.0, bpo)) == RANGE
    for sr in (0.0, -1.0, np.nan, np.inf):
        assert rc_of(lambda: s2.spectrum_band_readings(good, w, 0, sr, 3)) == RANGE
    dp = C.POINTER(C.c_double)
    out = np.zeros(129)
    assert L.s2r_spectrum_readings(good.ctypes.data_as(fp), 2, 256, w.ctypes.data_as(fp), 0, 1, out.ctypes.data_as(dp), 128) == INVALID
    assert L.s2r_spectrum_readings(good.ctypes.data_as(fp), 2, 256, w.ctypes.data_as(fp), 0, 1, None, 129) == INVALID
    assert L.s2r_spectrum_readings(None, 2, 256, w.ctypes.data_as(fp), 0, 1, out.ctypes.data_as(dp), 129) == INVALID
    nb = C.c_size_t(0)
    assert L.s2r_spectrum_band_readings(good.ctypes.data_as(fp), 2, 256, w.ctypes.data_as(fp), 0, 1, 48000.0, 3, out.ctypes.data_as(dp), None, 2,
                                        C.byref(nb)) == INVALID
