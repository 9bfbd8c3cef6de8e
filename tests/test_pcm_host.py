"""The PCM stage's handle-free functions (csrc/s2r_rules.cpp: s2r_pcm_reference, s2r_pcm_dither, s2r_pcm_pack, s2r_pcm_shaper) against a
numpy binary32 model of the rule that include/s2r.h states: the integers, the state bits and the clip counts; the dither's statistics;
the shapers' noise transfer; the packing.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import synth2_amd as s2

F = np.float32
U = np.uint32
CH, TAPS = s2.PCM_CHANNELS, s2.PCM_MAX_TAPS
DITHERS = ("none", "rect", "tpdf")
T_WRAP = 0xfffffff0


def mix(u):
    u = np.asarray(u, dtype=U).copy()
    with np.errstate(over="ignore"):
        u ^= u >> U(16); u *= U(0x7feb352d); u ^= u >> U(15); u *= U(0x846ca68b); u ^= u >> U(16)
    return u


def model_dither(seed, t, n, kind):
    """[18, n] float32: the rule's step 4 for frames t .. t + n - 1 mod 2^32"""
    with np.errstate(over="ignore"):
        tn = (np.arange(n, dtype=np.uint64) + np.uint64(t)).astype(U)
        inner = mix(tn ^ U(seed))
        k = mix(inner[None, :] + np.arange(CH, dtype=U)[:, None])
    r1, r2 = (k >> U(16)).astype(np.int64), (k & U(0xffff)).astype(np.int64)
    if kind == "tpdf":
        return (r1 - r2).astype(F) * F(2.0 ** -16)
    if kind == "rect":
        return (2 * r1 - 65535).astype(F) * F(2.0 ** -17)
    return np.zeros((CH, n), dtype=F)


def channels(stems, master):
    n = master.shape[0]
    x = np.zeros((CH, n), dtype=F)
    for p in range(0 if stems is None else stems.shape[0]):
        x[2 * p], x[2 * p + 1] = stems[p, :, 0], stems[p, :, 1]
    x[16], x[17] = master[:, 0], master[:, 1]
    return x


def model(stems, master, bits, dither, taps, seed, state=None, t=0, transposed=False):
    """the rule in numpy binary32, a frame at a time over the 18 channels: (pcm [9, n, 2], state [18, 9], t, clips [18], max |y - w|)"""
    taps = np.asarray(taps, dtype=F)
    K, n = taps.size, master.shape[0]
    G = F(2.0 ** (bits - 1))
    x = channels(stems, master)
    with np.errstate(invalid="ignore"):
        xc = np.where(np.isnan(x), F(0.0), np.minimum(np.maximum(x, F(-2.0)), F(2.0))).astype(F)
    s = xc * G
    d = model_dither(seed, t, n, dither)
    e = np.zeros((CH, TAPS), dtype=F) if state is None else np.array(state, dtype=F).reshape(CH, TAPS)
    if transposed:                               # Q[:, i]: the sum for the frame i ahead, over the errors known so far
        Q = np.zeros((CH, max(K, 1)), dtype=F)
        for i in range(K):
            f = np.zeros(CH, dtype=F)
            for j in range(K, i, -1):
                f = f + taps[j - 1] * e[:, j - 1 - i]
            Q[:, i] = f
    y_all = np.zeros((CH, n), dtype=np.int32)
    clips = np.zeros(CH, dtype=U)
    worst = 0.0
    for i in range(n):
        if transposed:
            f = Q[:, 0].copy() if K else np.zeros(CH, dtype=F)
        else:
            f = np.zeros(CH, dtype=F)
            for k in range(K, 0, -1):
                f = f + taps[k - 1] * e[:, k - 1]
        w = s[:, i] - f
        v = w + d[:, i]
        r = np.rint(v)
        y = np.minimum(np.maximum(r, -G), G - F(1.0))
        clips += (y != r).astype(U)
        y_all[:, i] = y.astype(np.int32)
        diff = y - w
        worst = max(worst, float(np.max(np.abs(diff))))
        en = np.minimum(np.maximum(diff, F(-2.0)), F(2.0))
        if transposed and K:
            for j in range(K - 1):
                Q[:, j] = Q[:, j + 1] + taps[j] * en
            Q[:, K - 1] = F(0.0) + taps[K - 1] * en
        if n:
            e[:, 1:] = e[:, :-1].copy()
            e[:, 0] = en
            e[:, K:] = F(0.0)
    pcm = np.stack([y_all[0::2], y_all[1::2]], axis=-1)
    return pcm, e, (t + n) & 0xffffffff, clips, worst


def signal(rng, n_buses, n, amp=0.9):
    stems = (rng.uniform(-amp, amp, (n_buses, n, 2))).astype(F) if n_buses else None
    master = rng.uniform(-amp, amp, (n, 2)).astype(F)
    return stems, master


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=F).view(U), np.asarray(b, dtype=F).view(U))


def shaper_of_k(K):
    return {0: s2.pcm_shaper(0), 1: s2.pcm_shaper(1), 2: s2.pcm_shaper(2), 5: s2.pcm_shaper(4), 9: s2.pcm_shaper(5)}[K]


@pytest.mark.parametrize("dither", DITHERS)
@pytest.mark.parametrize("bits", [8, 16, 24])
@pytest.mark.parametrize("K", [0, 1, 2, 5, 9])
def test_reference_matches_the_numpy_model(K, bits, dither):
    """integers, state bits and counts, over a stream of calls of 0, 1, K - 1, K, K + 1 and 1000 frames whose t wraps"""
    taps = shaper_of_k(K)
    n_buses = [0, 2, 8][([0, 1, 2, 5, 9].index(K) + bits // 8 + DITHERS.index(dither)) % 3]
    rng = np.random.default_rng(1000 * K + bits + DITHERS.index(dither))
    st_ref, t_ref, st_mod, t_mod = None, T_WRAP, None, T_WRAP
    for n in (0, 1, max(K - 1, 0), K, K + 1, 1000):
        stems, master = signal(rng, n_buses, n)
        pcm, st_ref, t_ref, clips = s2.pcm_reference(stems, master, bits, dither, taps, 77, st_ref, t_ref)
        want, st_mod, t_mod, wclips, worst = model(stems, master, bits, dither, taps, 77, st_mod, t_mod)
        assert pcm.shape == (9, n, 2) and np.array_equal(pcm, want)
        assert same_bits(st_ref, st_mod) and t_ref == t_mod and np.array_equal(clips, wclips)
        # an unclipped stream: the clamp of step 6 is idle.  (|y - w| < 1.5 in exact arithmetic; at 24 bits w has an ulp of 0.5 and
        # w + d rounds, so exactly 1.5 is reached there — still far from the clamp's 2.)
        assert (worst < 1.5 if bits < 24 else worst <= 1.5) and not clips.any()
    assert t_ref == (T_WRAP + 1002 + max(K - 1, 0) + 2 * K) & 0xffffffff and t_ref < T_WRAP
    assert not st_ref[:, K:].any() and (K == 0 or st_ref[16:, :K].any())


def test_a_silent_bus_is_dithered_like_any_other():
    """a bus at or past n_buses is fed +0.0, not skipped: with dither its samples are the dither's -1, 0 and 1"""
    rng = np.random.default_rng(5)
    stems, master = signal(rng, 2, 500)
    pcm, _, _, _ = s2.pcm_reference(stems, master, 16, "tpdf", 0, 3)
    assert set(np.unique(pcm[2:8])) == {-1, 0, 1}
    want = model(stems, master, 16, "tpdf", [], 3)[0]
    assert np.array_equal(pcm, want)


@pytest.mark.parametrize("K", [1, 2, 5, 9])
def test_the_transposed_form_is_the_descending_sum(K):
    """acc[n + k] += h[k - 1] * e[n], each sum started from +0.0 by its oldest error: every bit of the direct form"""
    rng = np.random.default_rng(K)
    taps = shaper_of_k(K)
    stems, master = signal(rng, 3, 400, amp=1.2)    # (with clips: the clamp runs in both forms)
    st = rng.uniform(-2.0, 2.0, (CH, TAPS)).astype(F)
    st[:, K:] = 0.0
    a = model(stems, master, 12, "tpdf", taps, 9, st, 5)
    b = model(stems, master, 12, "tpdf", taps, 9, st, 5, transposed=True)
    assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and np.array_equal(a[3], b[3]) and a[3].any()
    ref = s2.pcm_reference(stems, master, 12, "tpdf", taps, 9, st, 5)
    assert np.array_equal(ref[0], a[0]) and same_bits(ref[1], a[1]) and np.array_equal(ref[3], a[3])


@pytest.mark.parametrize("cut_seed", [11, 12, 13])
def test_one_call_equals_the_stream_cut_anywhere(cut_seed):
    rng = np.random.default_rng(2)
    stems, master = signal(rng, 8, 700)
    taps = s2.pcm_shaper(5)
    whole = s2.pcm_reference(stems, master, 16, "tpdf", taps, 21, None, T_WRAP)
    cuts = np.sort(np.random.default_rng(cut_seed).choice(np.arange(1, 700), size=12, replace=False))
    edges = [0] + list(cuts) + [700]
    st, t, parts, clips = None, T_WRAP, [], np.zeros(CH, dtype=U)
    for a, b in zip(edges[:-1], edges[1:]):
        pcm, st, t, c = s2.pcm_reference(stems[:, a:b], master[a:b], 16, "tpdf", taps, 21, st, t)
        parts.append(pcm); clips += c
    assert np.array_equal(np.concatenate(parts, axis=1), whole[0])
    assert same_bits(st, whole[1]) and t == whole[2] and np.array_equal(clips, whole[3])


def test_special_inputs():
    """NaN is +0.0, infinities and +-2.5 clamp to +-2 and clip, denormals and -0.0 go through the rule as any value"""
    tiny = np.float32(1e-45)
    vals = np.array([np.nan, np.inf, -np.inf, 2.5, -2.5, tiny, -tiny, np.float32(1.1754942e-38), -0.0, 0.0, 0.3, -0.3], dtype=F)
    master = np.stack([vals, vals[::-1]], axis=-1)
    stems = np.stack([master, -master])
    for K in (0, 2, 9):
        for dither in DITHERS:
            got = s2.pcm_reference(stems, master, 16, dither, shaper_of_k(K), 4)
            want = model(stems, master, 16, dither, shaper_of_k(K), 4)
            assert np.array_equal(got[0], want[0]) and same_bits(got[1], want[1]) and np.array_equal(got[3], want[3])
    pcm, st, _, clips = s2.pcm_reference(stems, master, 16, "none", 0, 0)
    assert list(pcm[8, :5, 0]) == [0, 32767, -32768, 32767, -32768] and list(pcm[8, 5:10, 0]) == [0] * 5
    assert pcm[8, 10, 0] == 9830 and pcm[8, 11, 0] == -9830
    assert clips[16] == 4 and clips[17] == 4 and clips[0] == 4 and not clips[4:16].any()
    assert np.isfinite(st).all()


def test_clips_on_both_rails_and_the_error_clamp():
    """a square wave at 1.5 through the nine-tap set: every frame clips, the output sits on the rails, every error is clamped to +-2,
    and the loop is back to normal within K frames of the signal's return"""
    n, G = 4096, 32768
    sq = np.where((np.arange(n) // 32) % 2 == 0, 1.5, -1.5).astype(F)
    quiet = (0.25 * np.sin(2 * np.pi * 997.0 / 44100.0 * np.arange(2048))).astype(F)
    master = np.stack([np.concatenate([sq, quiet])] * 2, axis=-1)
    taps = s2.pcm_shaper(5)
    pcm, st, t, clips = s2.pcm_reference(None, master, 16, "tpdf", taps, 1)
    want = model(None, master, 16, "tpdf", taps, 1)
    assert np.array_equal(pcm, want[0]) and same_bits(st, want[1]) and np.array_equal(clips, want[3])
    assert want[4] > 2.0                          # the clamp ran
    assert clips[16] >= n - 1 and clips[17] >= n - 1 and clips[16] < n + 9 and not clips[:16].any()
    assert set(np.unique(pcm[8, :n, 0])) == {-G, G - 1}
    # behind the square wave: the state after it is clamped errors, and 2 K frames later the error is an unclipped stream's
    _, st_mid, t_mid, _ = s2.pcm_reference(None, master[:n], 16, "tpdf", taps, 1)
    assert np.all(np.abs(st_mid[16:]) == 2.0)
    tail = model(None, master[n + 18:], 16, "tpdf", taps, 1, s2.pcm_reference(None, master[:n + 18], 16, "tpdf", taps, 1)[1], t_mid + 18)
    assert tail[4] < 1.5 and not tail[3].any()
    err = pcm[8, n + 18:, 0].astype(np.float64) - master[n + 18:, 0].astype(np.float64) * G
    assert 0.5 * 17.5 < err.var() < 2.0 * 17.5   # the nine-tap set's total error variance, 17.5 LSB^2


def dither_series(seed, q, kind, n):
    L = s2.load_library()
    d = C.c_float()
    fn, k, ref = L.s2r_pcm_dither, {"rect": 1, "tpdf": 2}[kind], C.byref(d)
    out = np.empty(n, dtype=F)
    for t in range(n):
        fn(seed, t, q, k, ref)
        out[t] = d.value
    return out


def test_dither_statistics():
    """2^20 frames of s2r_pcm_dither: the grid, the range, mean, variance, and the correlation at lag 1 and between two channels"""
    n = 1 << 20
    tri, tri2, rect = dither_series(12345, 0, "tpdf", n), dither_series(12345, 1, "tpdf", n), dither_series(12345, 0, "rect", n)
    # (the numpy model of the hash is the function's, on every one of these values)
    m = model_dither(12345, 0, n, "tpdf")
    assert same_bits(tri, m[0]) and same_bits(tri2, m[1]) and same_bits(rect, model_dither(12345, 0, n, "rect")[0])
    for x, step, half, var in ((tri, 2.0 ** -16, 1.0, 1.0 / 6.0), (tri2, 2.0 ** -16, 1.0, 1.0 / 6.0), (rect, 2.0 ** -17, 0.5, 1.0 / 12.0)):
        x = x.astype(np.float64)
        assert np.array_equal(x / step, np.rint(x / step))
        assert x.min() > -half and x.max() < half
        print("dither mean %.3g variance %.6g" % (x.mean(), x.var()))
        assert abs(x.mean()) <= 0.002
        assert abs(x.var() / var - 1.0) <= 0.01

    def corr(a, b):
        a, b = a.astype(np.float64) - a.mean(), b.astype(np.float64) - b.mean()
        return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))
    c = corr(tri[1:], tri[:-1]), corr(rect[1:], rect[:-1]), corr(tri, tri2)
    print("dither correlations %.3g %.3g %.3g" % c)
    assert max(abs(v) for v in c) <= 0.01
    assert s2.pcm_dither(12345, 7, 0, "none") == 0.0 and s2.pcm_dither(1, 2, 3, "tpdf") == float(model_dither(1, 2, 1, "tpdf")[3, 0])


BANDS = ((200.0, 2000.0), (2000.0, 5000.0), (8000.0, 12000.0), (15000.0, 22050.0))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_shapers_move_the_noise_as_their_transfer_says(seed):
    """44.1 kHz, 16 bits, triangular dither, 2^15 frames of a 997 Hz sine at 0.25, Hann window: per band, the error's mean power over
    kind 0's with the same seed lies within 1.5 dB of the band's mean |1 - sum h z^-k|^2, computed in binary64 from the binary32 taps"""
    n, fs, G = 1 << 15, 44100.0, 32768.0
    x = (0.25 * np.sin(2 * np.pi * 997.0 / fs * np.arange(n))).astype(F)
    master = np.stack([x, x], axis=-1)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)
    freqs = np.arange(n // 2 + 1) * fs / n

    def band_powers(kind):
        pcm, _, _, clips = s2.pcm_reference(None, master, 16, "tpdf", kind, seed)
        assert not clips.any()
        err = pcm[8, :, 0].astype(np.float64) - x.astype(np.float64) * G
        p = np.abs(np.fft.rfft(err * win)) ** 2
        return err, [p[(freqs >= lo) & (freqs <= hi)].mean() for lo, hi in BANDS]

    err0, flat = band_powers(0)
    assert abs(err0.var() / 0.25 - 1.0) <= 0.05
    for kind in range(1, 6):
        taps = s2.pcm_shaper(kind).astype(np.float64)
        z = np.exp(-2j * np.pi * freqs / fs)
        ntf = np.abs(1.0 - sum(taps[k] * z ** (k + 1) for k in range(taps.size))) ** 2
        _, shaped = band_powers(kind)
        for (lo, hi), ps, p0 in zip(BANDS, shaped, flat):
            want = 10 * np.log10(ntf[(freqs >= lo) & (freqs <= hi)].mean())
            got = 10 * np.log10(ps / p0)
            print("kind %d band %5.0f-%5.0f: %.2f dB, transfer %.2f dB" % (kind, lo, hi, got, want))
            assert abs(got - want) <= 1.5, (kind, lo, hi, got, want)


def test_shaper_tables():
    want = {0: [], 1: [1], 2: [2, -1], 3: [1.623, -0.982, 0.109], 4: [2.033, -2.165, 1.959, -1.590, 0.6149],
            5: [2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847]}
    for kind, taps in want.items():
        assert same_bits(s2.pcm_shaper(kind), np.array(taps, dtype=F))
    with pytest.raises(s2.S2rError) as e:
        s2.pcm_shaper(6)
    assert e.value.status == -5


def test_pack():
    rng = np.random.default_rng(3)
    p16 = np.concatenate([rng.integers(-32768, 32768, 1000), [-32768, 32767, -1, 0, 1]]).astype(np.int32)
    assert s2.pcm_pack(p16, 16, 2).tobytes() == p16.astype("<i2").tobytes()
    p24 = np.concatenate([rng.integers(-(1 << 23), 1 << 23, 1000), [-(1 << 23), (1 << 23) - 1, -1, 0, 1]]).astype(np.int32)
    by = np.stack([p24 & 0xff, (p24 >> 8) & 0xff, (p24 >> 16) & 0xff], axis=-1).astype(np.uint8)
    assert np.array_equal(s2.pcm_pack(p24, 24, 3), by.reshape(-1))
    assert s2.pcm_pack(p24, 24, 4).tobytes() == (p24.astype(np.int64) << 8).astype("<i4").tobytes()
    by = np.stack([np.zeros_like(p16), p16 & 0xff, (p16 >> 8) & 0xff], axis=-1).astype(np.uint8)    # 16 bits in 3 bytes: the low byte is 0
    assert np.array_equal(s2.pcm_pack(p16, 16, 3), by.reshape(-1))
    p8 = np.arange(-128, 128, dtype=np.int32)
    assert s2.pcm_pack(p8, 8, 2).tobytes() == (p8 << 8).astype("<i2").tobytes()
    assert s2.pcm_pack(p20 := np.array([-(1 << 19), (1 << 19) - 1], dtype=np.int32), 20, 3).tobytes() == bytes([0, 0, 0x80, 0xf0, 0xff, 0x7f]) and p20.size == 2
    assert s2.pcm_pack(np.zeros(0, dtype=np.int32), 16, 2).size == 0
    for pcm, bits, width in ((p24, 24, 2), (p16, 17, 2), (p16, 16, 1), (p16, 16, 5), (p16, 7, 2), (p16, 25, 4), (p24, 16, 2), (np.array([128], dtype=np.int32), 8, 2),
                             (np.array([-129], dtype=np.int32), 8, 2)):
        with pytest.raises(s2.S2rError) as e:
            s2.pcm_pack(pcm, bits, width)
        assert e.value.status == -5


def test_refusals_change_nothing():
    L = s2.load_library()
    f32p, u32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    rng = np.random.default_rng(4)
    stems, master = signal(rng, 2, 16)
    taps = s2.pcm_shaper(5)
    state = rng.uniform(-1, 1, s2.PCM_STATE).astype(F)

    def call(bits=16, dither=2, taps=taps, n_taps=9, n_buses=2, state=state, stems=stems, master=master, with_t=True, with_pcm=True):
        st = None if state is None else state.copy()
        t, pcm, clips = C.c_uint32(41), np.full((9, 16, 2), 7, dtype=np.int32), np.full(CH, 7, dtype=U)
        rc = L.s2r_pcm_reference(bits, dither, None if taps is None else taps.ctypes.data_as(f32p), n_taps, 5, None if stems is None else stems.ctypes.data_as(f32p),
                                 n_buses, None if master is None else master.ctypes.data_as(f32p), 16, None if st is None else st.ctypes.data_as(f32p),
                                 C.byref(t) if with_t else None, pcm.ctypes.data_as(i32p) if with_pcm else None, clips.ctypes.data_as(u32p))
        if rc != 0:
            assert (st is None or same_bits(st, state)) and t.value == 41 and (pcm == 7).all() and (clips == 7).all()
        return rc
    assert call() == 0
    bad_tap, nan_tap = taps.copy(), taps.copy()
    bad_tap[8], nan_tap[0] = 16.5, np.nan
    bad_state, nan_state = state.copy(), state.copy()
    bad_state[161], nan_state[0] = 2.5, np.nan
    assert call(bits=7) == call(bits=25) == call(dither=3) == call(n_taps=10) == call(taps=bad_tap) == call(taps=nan_tap) == call(n_buses=9) == -5
    assert call(state=bad_state) == call(state=nan_state) == call(taps=np.array([-16.25], dtype=F), n_taps=1) == -5
    assert call(taps=np.array([16.0, -16.0], dtype=F), n_taps=2) == 0
    assert call(taps=None) == call(state=None) == call(stems=None) == call(master=None) == call(with_t=False) == call(with_pcm=False) == -1
    assert call(taps=None, n_taps=0) == 0 and call(stems=None, n_buses=0) == 0
    d = C.c_float(9.0)
    assert L.s2r_pcm_dither(1, 2, 18, 2, C.byref(d)) == -5 and L.s2r_pcm_dither(1, 2, 0, 3, C.byref(d)) == -5 and L.s2r_pcm_dither(1, 2, 0, 2, None) == -1
    assert d.value == 9.0
    n = C.c_uint32(9)
    assert L.s2r_pcm_shaper(0, None, C.byref(n)) == -1 and L.s2r_pcm_shaper(0, taps.ctypes.data_as(f32p), None) == -1 and n.value == 9
    assert L.s2r_pcm_pack(None, 4, 16, 2, None) == -1 and L.s2r_pcm_pack(None, 0, 16, 2, None) == 0
    with pytest.raises(ValueError):
        s2.pcm_reference(stems, master[:8])
    with pytest.raises(ValueError):
        s2.pcm_reference(None, master, dither="blue")


def test_the_abi_version_stays():
    assert s2.load_library().s2r_abi_version() == 4
    assert (s2.PCM_PROGRAMMES, s2.PCM_CHANNELS, s2.PCM_MAX_TAPS, s2.PCM_STATE) == (9, 18, 9, 162)
