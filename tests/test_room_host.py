"""The per-bus room reverb, the host side: s2r_room_reference — the rule restated in plain C++ — held against a numpy
float32 model of the rule written here (np_room: a loop over frames), calls that concatenate, the degenerate settings (damp 0 and 1,
feedback 0, gain 0), the first frames after a set with no model in the loop, the state's layout and count, s2r_room_design against its
formula in numpy float64, the range checks of the entry points, which answer without a device, and the reference against a binary64
evaluation of the same recurrences.  Comparisons of signals and states are on bits (helpers.assert_bits_equal_finite).

Run as a program (PYTHONPATH=.:tests python tests/test_room_host.py, from the repository's root) this file measures how far the numpy
float32 model is from the binary64 evaluation on the test's inputs, and writes that and twice that — the bound the library is held
to — into profiles/truth/room_deviation.json."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_reverb_host import _new_or_skip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUTH = os.path.join(ROOT, "profiles", "truth", "room_deviation.json")
F = np.float32
NAN = float("nan")
INF = float("inf")
M32 = 0xFFFFFFFF
FLAT = ([64] * 8, [64] * 4, 0)                                   # every line at the least delay
SMALL = ([64, 65, 71, 79, 83, 89, 97, 101], [64, 67, 73, 80], 3)
LEVELS = dict(feedback=0.84, damp=0.2, g=0.5, gain=0.25, dry=0.75, wet=0.5, cross=0.25)
# the cases of the binary64 comparison: (name, delays, levels, frames, seed)
TRUTH_CASES = [("small", SMALL, LEVELS, 3000, 11), ("flat", FLAT, dict(LEVELS, damp=0.5, feedback=0.7), 1500, 12),
               ("design48k", None, dict(LEVELS, feedback=0.9, damp=0.4, gain=0.015, cross=0.0), 6000, 13)]


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def _p(a):
    return a.ctypes.data_as(s2s._f32p)


def _u(a):
    return a.ctypes.data_as(s2s._u32p)


def _signal(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((n, 2)) * scale).astype(F)


def lines(cd, ad, spread):
    """[(length, offset into the flat state, is a comb)] in the state's order: per channel the combs, each with its f behind it, then
    the allpasses"""
    out, at = [], 0
    for c in range(2):
        for d in cd:
            out.append((int(d) + c * spread, at, True))
            at += int(d) + c * spread + 1
        for d in ad:
            out.append((int(d) + c * spread, at, False))
            at += int(d) + c * spread
    return out, at


def np_room(T, cd, ad, spread, lv, x, state):
    """the rule in numpy scalars of type T (np.float32: the model; np.float64: the same recurrences in binary64): one operation per
    line of the rule, each rounded to T; returns (out [frames, 2], the state after the call)"""
    fb, damp, g, gain, dry, wet, cross = (T(F(lv[k])) for k in ("feedback", "damp", "g", "gain", "dry", "wet", "cross"))
    d1 = T(1.0) - damp
    lay, total = lines(cd, ad, spread)
    assert state.size == total
    n_frames = x.shape[0]
    per = []                                                     # per channel: (comb buffers, f, allpass buffers); a buffer is history then the call
    for c in range(2):
        combs, fs, alls = [], [], []
        for (ln, at, comb) in lay[c * 12:(c + 1) * 12]:
            buf = np.concatenate([state[at:at + ln].astype(T), np.zeros(n_frames, dtype=T)])
            if comb:
                combs.append((buf, ln)); fs.append(T(state[at + ln]))
            else:
                alls.append((buf, ln))
        per.append((combs, fs, alls))
    out = np.zeros((n_frames, 2), dtype=T)
    xs = x.astype(T)
    for n in range(n_frames):
        inp = (xs[n, 0] + xs[n, 1]) * gain
        v = [None, None]
        for c in range(2):
            combs, fs, alls = per[c]
            acc = T(0.0)
            for i, (buf, ln) in enumerate(combs):
                o = buf[n]
                fs[i] = o * d1 + fs[i] * damp
                buf[ln + n] = inp + fs[i] * fb
                acc = acc + o
            for (buf, ln) in alls:
                b = buf[n]
                y = b - acc
                buf[ln + n] = acc + b * g
                acc = y
            v[c] = acc
        for c in range(2):
            out[n, c] = dry * xs[n, c] + (wet * v[c] + cross * v[1 - c])
    new = np.zeros(total, dtype=T)
    for c in range(2):
        combs, fs, alls = per[c]
        k = 0
        for (ln, at, comb) in lay[c * 12:(c + 1) * 12]:
            if comb:
                new[at:at + ln] = combs[k][0][n_frames:]; new[at + ln] = fs[k]; k += 1
        for (buf, ln), (_, at, _) in zip(alls, lay[c * 12 + 8:(c + 1) * 12]):
            new[at:at + ln] = buf[n_frames:]
    return out, new


def ref(delays, lv, x, state=None):
    return s2.room_reference(delays[0], delays[1], delays[2], lv["feedback"], lv["damp"], lv["g"], lv["gain"], lv["dry"], lv["wet"], lv["cross"], x, state)


def zeros(delays):
    return np.zeros(s2.room_state_floats(*delays), dtype=F)


def _truth_delays(case):
    return case[1] if case[1] is not None else tuple(s2.room_design(48000.0))


def deviation(out, want):
    """the largest distance from the binary64 evaluation, as a fraction of its peak"""
    return float(np.max(np.abs(out.astype(np.float64) - want)) / np.max(np.abs(want)))


def measure():
    rows = []
    for case in TRUTH_CASES:
        name, _, lv, frames, seed = case
        d = _truth_delays(case)
        x = _signal(frames, seed)
        st = zeros(d)
        got, _ = np_room(F, d[0], d[1], d[2], lv, x, st)
        want, _ = np_room(np.float64, d[0], d[1], d[2], lv, x, st)
        dev = deviation(got, want)
        rows.append({"case": name, "frames": frames, "seed": seed, "reference_deviation": dev, "bound": 2.0 * dev})
    return {"what": "largest distance of the numpy float32 model of the room's rule (tests/test_room_host.py: np_room) from the same recurrences "
                    "evaluated in binary64, over all frames and both channels, as a fraction of the binary64 output's peak; bound = 2 x that; "
                    "s2r_room_reference is held to the bound on the same inputs",
            "cases": rows}


@pytest.mark.parametrize("frames", [0, 1, 2, 5, 1000])
@pytest.mark.parametrize("delays", [FLAT, SMALL], ids=["flat", "small"])
def test_reference_is_the_numpy_model(frames, delays):
    """from a state with nothing regular about it, so that every line and every f is read from the first frame on"""
    x = _signal(frames, 100 + frames)
    st = (np.random.default_rng(7).standard_normal(s2.room_state_floats(*delays)) * 0.25).astype(F)
    want, wst = np_room(F, delays[0], delays[1], delays[2], LEVELS, x, st)
    got, gst = ref(delays, LEVELS, x, st)
    assert np.isfinite(want).all()
    assert_bits_equal_finite(got, want, "out")
    assert_bits_equal_finite(gst, wst, "state")
    if frames == 0:
        assert_bits_equal_finite(gst, st, "no frames: nothing moves")


def test_the_issue_s_model_run():
    """3000 frames from silence, delays of 64 to 101 frames, spread 3, feedback 0.84, damp 0.2: the output stays finite, and one call
    cut in two gives identical bits"""
    x = _signal(3000, 5)
    whole, wst = ref(SMALL, LEVELS, x)
    assert np.isfinite(whole).all() and float(np.abs(whole).max()) < 100.0
    want, _ = np_room(F, SMALL[0], SMALL[1], SMALL[2], LEVELS, x, zeros(SMALL))
    assert_bits_equal_finite(whole, want, "the model")
    a, st = ref(SMALL, LEVELS, x[:1234])
    b, st = ref(SMALL, LEVELS, x[1234:], st)
    assert_bits_equal_finite(np.concatenate([a, b]), whole, "two calls")
    assert_bits_equal_finite(st, wst, "state")


@pytest.mark.parametrize("cuts", [(1,), (63, 64, 65), (5, 70, 300, 301), tuple(range(100, 900, 100))])
def test_calls_of_any_lengths_concatenate(cuts):
    x = _signal(1000, 21)
    whole, wst = ref(SMALL, LEVELS, x)
    st, parts, at = None, [], 0
    for c in cuts + (1000,):
        o, st = ref(SMALL, LEVELS, x[at:c], st)
        parts.append(o); at = c
    assert_bits_equal_finite(np.concatenate(parts), whole, str(cuts))
    assert_bits_equal_finite(st, wst, "state")


@pytest.mark.parametrize("change", [dict(damp=0.0), dict(damp=1.0), dict(feedback=0.0), dict(g=0.0), dict(g=-0.75), dict(wet=0.0), dict(dry=0.0, cross=1.0)])
def test_degenerate_levels_are_the_model_too(change):
    """no operation is skipped for a zero coefficient: the model, which skips none, gives the bits"""
    lv = dict(LEVELS, **change)
    x = _signal(400, 31)
    st = (np.random.default_rng(8).standard_normal(s2.room_state_floats(*SMALL)) * 0.25).astype(F)
    want, wst = np_room(F, SMALL[0], SMALL[1], SMALL[2], lv, x, st)
    got, gst = ref(SMALL, lv, x, st)
    assert_bits_equal_finite(got, want, str(change))
    assert_bits_equal_finite(gst, wst, str(change))


def test_damp_one_freezes_f_and_damp_zero_makes_it_the_line():
    x = _signal(200, 41)
    st = (np.random.default_rng(9).standard_normal(s2.room_state_floats(*FLAT)) * 0.25).astype(F)
    lay, _ = lines(*FLAT)
    _, frozen = ref(FLAT, dict(LEVELS, damp=1.0), x, st)         # f = o * 0 + f * 1
    _, follows = ref(FLAT, dict(LEVELS, damp=0.0), x[:10], st)   # f = o * 1 + f * 0: the line's frame of 64 frames ago
    for (ln, at, comb) in lay:
        if comb:
            assert bits(frozen[at + ln]) == bits(st[at + ln] + F(0.0))
            assert bits(follows[at + ln]) == bits(st[at + 9] + F(0.0))


def test_gain_zero_and_dry_one_pass_the_input():
    """from silence with gain 0 nothing ever enters a line: the output is the input up to the sign of zero"""
    x = _signal(300, 51)
    x[7] = [0.0, -0.0]
    out, st = ref(SMALL, dict(LEVELS, gain=0.0, dry=1.0), x)
    assert np.array_equal(out, x)
    assert_bits_equal_finite(out, x + F(0.0), "x + 0")
    assert not st.any()


@pytest.mark.parametrize("delays", [FLAT, SMALL], ids=["flat", "small"])
def test_the_first_frames_after_a_set_are_dry(delays):
    """no model in the loop: until the shortest line turns over every o and b is +0.0, so v is +0.0 and out = fl(dry * x) + 0"""
    x = _signal(200, 61)
    out, _ = ref(delays, LEVELS, x)
    m = min(min(delays[0]), min(delays[1]))
    want = F(LEVELS["dry"]) * x[:m] + F(0.0)
    assert_bits_equal_finite(out[:m], want, "dry")
    assert (out[m:m + 40] != F(LEVELS["dry"]) * x[m:m + 40]).any()


def test_the_state_layout_and_its_count():
    """an impulse of known size from silence with feedback 0 and damp 0: every comb line holds in at its last-but-k frame, f is that frame's o"""
    for delays in (FLAT, SMALL, ([8192] * 8, [8192] * 4, 0), ([64] * 8, [8169] * 4, 23)):
        cd, ad, sp = delays
        assert s2.room_state_floats(cd, ad, sp) == 2 * (sum(cd) + sum(ad) + 8) + 12 * sp == lines(cd, ad, sp)[1]
    assert s2.room_state_floats([63] + [64] * 7, [64] * 4, 0) == 0 and s2.room_state_floats([64] * 8, [8192] * 4, 1) == 0
    x = np.zeros((10, 2), dtype=F)
    x[3] = [0.5, 0.25]
    lv = dict(LEVELS, feedback=0.0, damp=0.0, gain=1.0)
    _, st = ref(SMALL, lv, x)
    lay, total = lines(*SMALL)
    assert st.size == total
    want = np.zeros(total, dtype=F)
    for (ln, at, comb) in lay:
        if comb:
            want[at + ln - 10 + 3] = 0.75                        # the line's last 10 frames are the call's: in at frame 3, oldest frame first
    assert_bits_equal_finite(st, want, "combs hold the impulse, allpasses and f nothing yet")
    # and the allpass lines: run on until the combs' outputs have reached them
    _, st2 = ref(SMALL, lv, np.zeros((100, 2), dtype=F), st)
    _, wst2 = np_room(F, SMALL[0], SMALL[1], SMALL[2], lv, np.zeros((100, 2), dtype=F), st)
    assert_bits_equal_finite(st2, wst2, "after 100 more frames")
    for (ln, at, comb) in lay:
        if not comb:
            assert st2[at:at + ln].any()


@pytest.mark.parametrize("sr", [44100.0, 48000.0, 192000.0])
def test_design_is_the_formula_in_float64(sr):
    for size in (1.0, 0.5, 1.1):
        k = np.float64(sr) / np.float64(44100.0) * np.float64(size)
        want_c = np.rint(np.array([1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617], dtype=np.float64) * k)
        want_a = np.rint(np.array([556, 441, 341, 225], dtype=np.float64) * k)
        want_s = np.rint(np.float64(23.0) * k)
        top = max(want_c.max(), want_a.max()) + want_s
        if top > 8192 or min(want_c.min(), want_a.min()) < 64:
            with pytest.raises(s2.S2rError) as err:
                s2.room_design(sr, size)
            assert err.value.status == s2s.S2R_ERR_PATCH_RANGE
            continue
        cd, ad, sp = s2.room_design(sr, size)
        assert cd.dtype == np.uint32 and (cd == want_c).all() and (ad == want_a).all() and sp == want_s, (sr, size)
        assert s2.room_state_floats(cd, ad, sp) > 0
    if sr == 44100.0:
        cd, ad, sp = s2.room_design(sr)
        assert list(cd) == [1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617] and list(ad) == [556, 441, 341, 225] and sp == 23


def test_design_range_checks():
    L = s2.load_library()
    cd, ad, sp = np.full(8, 9, dtype=np.uint32), np.full(4, 9, dtype=np.uint32), C.c_uint32(9)
    for sr, size in [(NAN, 1.0), (48000.0, NAN), (0.0, 1.0), (-1.0, 1.0), (48000.0, 0.0), (INF, 1.0), (48000.0, INF), (8000.0, 1.0), (44100.0, 6.0),
                     (192000.0, 1.5), (44100.0, 0.25)]:
        assert L.s2r_room_design(sr, size, _u(cd), _u(ad), C.byref(sp)) == s2s.S2R_ERR_PATCH_RANGE, (sr, size)
    assert (cd == 9).all() and (ad == 9).all() and sp.value == 9
    assert L.s2r_room_design(48000.0, 1.0, None, _u(ad), C.byref(sp)) == s2s.S2R_ERR_INVALID
    assert L.s2r_room_design(48000.0, 1.0, _u(cd), None, C.byref(sp)) == s2s.S2R_ERR_INVALID
    assert L.s2r_room_design(48000.0, 1.0, _u(cd), _u(ad), None) == s2s.S2R_ERR_INVALID


def test_the_committed_bounds_are_the_measurement():
    doc = json.load(open(TRUTH))
    assert [(r["case"], r["frames"], r["seed"]) for r in doc["cases"]] == [(c[0], c[3], c[4]) for c in TRUTH_CASES]
    for r in doc["cases"]:
        assert r["bound"] == 2.0 * r["reference_deviation"] and 0.0 < r["reference_deviation"] < 1e-4, r


@pytest.mark.parametrize("i", range(len(TRUTH_CASES)))
def test_reference_against_binary64(i):
    """the library's rule is as close to the recurrences in binary64 as twice the numpy float32 model's own deviation on the same
    input (measured on the CPU, committed)"""
    case = TRUTH_CASES[i]
    row = json.load(open(TRUTH))["cases"][i]
    d = _truth_delays(case)
    x = _signal(case[3], case[4])
    got, _ = ref(d, case[2], x)
    want, _ = np_room(np.float64, d[0], d[1], d[2], case[2], x, zeros(d))
    dev = deviation(got, want)
    print("%s: deviation %.3e, bound %.3e" % (case[0], dev, row["bound"]))
    assert dev <= row["bound"], (case[0], dev, row["bound"])


GOOD = (0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5)
# (index into the seven levels, values out of its range)
BAD_LEVELS = [(0, [NAN, INF, -INF, 1.0, -1e-30, 2.0]), (1, [NAN, INF, -1e-30, float(np.nextafter(F(1.0), F(2.0)))]), (2, [NAN, 1.0, -1.0, INF, -2.0]),
              (3, [NAN, -1e-30, 1.5]), (4, [NAN, -1e-30, 1.5]), (5, [NAN, -1e-30, 1.5]), (6, [NAN, -1e-30, 1.5, -INF])]
EDGE_LEVELS = [(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (float(np.nextafter(F(1.0), F(0.0))), 1.0, float(np.nextafter(F(1.0), F(0.0))), 1.0, 1.0, 1.0, 1.0),
               (0.5, 0.5, float(np.nextafter(F(-1.0), F(0.0))), 0.5, 0.5, 0.5, 0.5)]


def bad_delays():
    """(cd, ad, spread) with one effective delay out of range"""
    out = []
    for k in range(12):
        for v, sp in ((63, 0), (0, 0), (8193, 0), (8192, 1), (M32, 0), (M32 - 1, 3), (8170, 23)):
            d = np.full(12, 100, dtype=np.uint32)
            d[k] = v
            out.append((d[:8].copy(), d[8:].copy(), sp))
    out.append((np.full(8, 100, dtype=np.uint32), np.full(4, 100, dtype=np.uint32), M32))
    out.append((np.full(8, 100, dtype=np.uint32), np.full(4, 100, dtype=np.uint32), 8093))
    return out


def test_range_errors_without_a_handle():
    """every entry looks at the values before it looks at the handle, so the range checks answer without a device, and a refused
    reference call leaves state and output alone; S2R_ERR_INVALID is what no handle gets for values in range"""
    L = s2.load_library()
    cd, ad = np.full(8, 100, dtype=np.uint32), np.full(4, 100, dtype=np.uint32)
    for (c, a, sp) in bad_delays():
        assert L.s2r_set_bus_room(None, 0, _u(c), _u(a), sp, *GOOD) == s2s.S2R_ERR_PATCH_RANGE, (c, a, sp)
        assert L.s2r_room_state_floats(_u(c), _u(a), sp) == 0
    for k, vals in BAD_LEVELS:
        for v in vals:
            lv = list(GOOD); lv[k] = v
            assert L.s2r_set_bus_room(None, 0, _u(cd), _u(ad), 0, *lv) == s2s.S2R_ERR_PATCH_RANGE, (k, v)
            assert L.s2r_set_bus_room_params(None, 0, *lv) == s2s.S2R_ERR_PATCH_RANGE, (k, v)
    for bus in (8, 255, M32):
        assert L.s2r_set_bus_room(None, bus, _u(cd), _u(ad), 0, *GOOD) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_room_params(None, bus, *GOOD) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_clear_bus_room(None, bus) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_get_bus_room(None, bus, None, None, None, None, None) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_get_bus_room_state(None, bus, None, 0) == s2s.S2R_ERR_PATCH_RANGE
        assert L.s2r_set_bus_room_state(None, bus, None, 0) == s2s.S2R_ERR_PATCH_RANGE
    for lv in EDGE_LEVELS:
        assert L.s2r_set_bus_room(None, 7, _u(np.full(8, 64, dtype=np.uint32)), _u(np.full(4, 8192, dtype=np.uint32)), 0, *lv) == s2s.S2R_ERR_INVALID, lv
        assert L.s2r_set_bus_room(None, 7, _u(np.full(8, 8169, dtype=np.uint32)), _u(np.full(4, 64, dtype=np.uint32)), 23, *lv) == s2s.S2R_ERR_INVALID, lv
        assert L.s2r_set_bus_room_params(None, 7, *lv) == s2s.S2R_ERR_INVALID, lv
    assert L.s2r_set_bus_room(None, 0, None, _u(ad), 0, *GOOD) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_room(None, 0, _u(cd), None, 0, *GOOD) == s2s.S2R_ERR_INVALID
    assert L.s2r_clear_bus_room(None, 0) == s2s.S2R_ERR_INVALID
    n = C.c_uint32(5)
    assert L.s2r_get_bus_room(None, 0, C.byref(n), None, None, None, None) == s2s.S2R_ERR_INVALID and n.value == 5
    buf = np.zeros(4, dtype=F)
    assert L.s2r_get_bus_room_state(None, 0, _p(buf), 4) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_room_state(None, 0, _p(buf), 4) == s2s.S2R_ERR_INVALID
    assert L.s2r_room_state_floats(None, _u(ad), 0) == 0 and L.s2r_room_state_floats(_u(cd), None, 0) == 0
    # the reference: a refusal changes neither the state nor the output
    rf = L.s2r_room_reference
    x, out = _signal(3, 1), np.full((3, 2), 9.0, dtype=F)
    st = np.full(int(L.s2r_room_state_floats(_u(cd), _u(ad), 0)), 0.5, dtype=F)
    for (c, a, sp) in bad_delays():
        assert rf(_u(c), _u(a), sp, *GOOD, _p(x), 3, _p(st), _p(out)) == s2s.S2R_ERR_PATCH_RANGE
    for k, vals in BAD_LEVELS:
        for v in vals:
            lv = list(GOOD); lv[k] = v
            assert rf(_u(cd), _u(ad), 0, *lv, _p(x), 3, _p(st), _p(out)) == s2s.S2R_ERR_PATCH_RANGE, (k, v)
    for v in (NAN, INF, -INF):
        bad = st.copy(); bad[-1] = v
        assert rf(_u(cd), _u(ad), 0, *GOOD, _p(x), 3, _p(bad), _p(out)) == s2s.S2R_ERR_PATCH_RANGE
    assert rf(None, _u(ad), 0, *GOOD, _p(x), 3, _p(st), _p(out)) == s2s.S2R_ERR_INVALID
    assert rf(_u(cd), None, 0, *GOOD, _p(x), 3, _p(st), _p(out)) == s2s.S2R_ERR_INVALID
    assert rf(_u(cd), _u(ad), 0, *GOOD, _p(x), 3, None, _p(out)) == s2s.S2R_ERR_INVALID
    assert rf(_u(cd), _u(ad), 0, *GOOD, None, 3, _p(st), _p(out)) == s2s.S2R_ERR_INVALID
    assert (st == 0.5).all() and (out == 9.0).all()
    assert rf(_u(cd), _u(ad), 0, *GOOD, None, 0, _p(st), None) == s2s.S2R_OK and (st == 0.5).all()      # no frames: nothing moves
    assert rf(_u(cd), _u(ad), 0, *GOOD, _p(x), 3, _p(st), None) == s2s.S2R_OK and not (st == 0.5).all()    # no output: the state alone
    with pytest.raises(ValueError):
        s2.room_reference(cd[:-1], ad, 0, *GOOD, x)
    with pytest.raises(s2.S2rError) as err:
        s2.room_reference(cd, ad, 0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, x)
    assert err.value.status == s2s.S2R_ERR_PATCH_RANGE
    assert s2.Synth.room_reference(cd, ad, 0, *GOOD, x)[0].shape == (3, 2)
    syn = _new_or_skip(num_voices=8, max_frames=64)              # with a device the rest runs on a real handle
    if syn is not None:
        check_ranges(syn)


def test_abi_version_stays():
    assert s2.load_library().s2r_abi_version() == 4


def check_ranges(syn):
    """the setters' range checks on a live handle, and the parameter and state entries on a bus without a room (also called by
    tests/test_gpu_room.py)"""
    L, h = syn.L, syn.h
    cd, ad = np.full(8, 100, dtype=np.uint32), np.full(4, 100, dtype=np.uint32)
    for (c, a, sp) in bad_delays()[::5]:
        assert L.s2r_set_bus_room(h, 0, _u(c), _u(a), sp, *GOOD) == s2s.S2R_ERR_PATCH_RANGE
    for k, vals in BAD_LEVELS:
        lv = list(GOOD); lv[k] = vals[0]
        assert L.s2r_set_bus_room(h, 0, _u(cd), _u(ad), 0, *lv) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_room(h, 8, _u(cd), _u(ad), 0, *GOOD) == s2s.S2R_ERR_PATCH_RANGE
    assert L.s2r_set_bus_room(h, 0, None, _u(ad), 0, *GOOD) == s2s.S2R_ERR_INVALID
    assert syn.get_bus_room(0) is None
    assert L.s2r_set_bus_room_params(h, 0, *GOOD) == s2s.S2R_ERR_INVALID
    buf = np.zeros(4, dtype=F)
    assert L.s2r_get_bus_room_state(h, 0, _p(buf), 4) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_bus_room_state(h, 0, _p(buf), 4) == s2s.S2R_ERR_INVALID
    assert L.s2r_clear_bus_room(h, 0) == s2s.S2R_OK


if __name__ == "__main__":
    doc = measure()
    os.makedirs(os.path.dirname(TRUTH), exist_ok=True)
    with open(TRUTH, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in doc["cases"]:
        print(r)
