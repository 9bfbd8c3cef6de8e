"""The master limiter, the host side: s2r_limiter_reference — the rule restated in plain C++ loops — held against
a numpy float32 model of the rule written here (np_limiter, which tests/test_gpu_limiter.py holds the device against too), the
properties the rule promises with no model in the loop, and the range checks of the entry points, which answer without a device."""
import ctypes as C

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view
import pytest

import synth2_amd as s2
from synth2_amd import synth as s2s
from test_reverb_host import MIXED

F = np.float32
NAN = float("nan")
INF = float("inf")
# (lookahead, hold)
PAIRS = [(1, 0), (5, 3), (48, 0), (64, 100), (240, 480), (1024, 4096), (255, 0), (256, 0), (257, 1)]
CUTS = [7, 293, 1, 1699, 1000]
BAD = [(NAN, 48, 0), (INF, 48, 0), (-0.25, 48, 0), (0.0, 48, 0), (2.0 ** -21, 48, 0), (2.0 ** 20 * 1.0000002, 48, 0), (0.25, 0, 0),
       (0.25, 1025, 0), (0.25, 0xffffffff, 0), (0.25, 48, 4097), (0.25, 48, 0xffffffff)]
GOOD = [(2.0 ** -20, 1, 0), (2.0 ** 20, 1024, 4096), (0.25, 48, 0), (1.0, 240, 480)]


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def np_limiter(x, C, L, H, xh=None, gh=None, oldest_first=False, short_min=False, parts=False):
    """The rule in numpy float32: x [N, 2]; returns (y, s', xh, gh) with the state the call leaves.  oldest_first, short_min: WRONG
    variants for the tests that show the rule's order and window are visible (the sum added oldest first; the minimum over k < L + H).
    parts: (s, g[n - L], x[n - L]) instead — what steps 4 and 5 start from."""
    F = np.float32; N = len(x); C = F(C); W = L + 1; G = 2 * L + H
    xh = np.zeros((L, 2), F) if xh is None else xh
    gh = np.ones(G, F) if gh is None else gh
    p = np.maximum(np.abs(x[:, 0]), np.abs(x[:, 1]))
    with np.errstate(divide="ignore", invalid="ignore", under="ignore", over="ignore"):
        g = np.where(p > C, C / p, F(1)).astype(F)
    ge, xe = np.concatenate([gh, g]), np.concatenate([xh, x])
    if short_min:
        m = sliding_window_view(ge[1:], L + H).min(axis=1)
    else:
        m = sliding_window_view(ge, L + H + 1).min(axis=1)           # m[j] is m[n = j - L]
    acc = np.zeros(N, F)
    with np.errstate(under="ignore"):
        for k in (range(W - 1, -1, -1) if oldest_first else range(W)):
            acc = (acc + m[L - k:L - k + N]).astype(F)
        s = (acc / F(W)).astype(F)
        if parts:
            return s, ge[G - L:G - L + N], xe[:N]
        sp = np.minimum(s, ge[G - L:G - L + N])
        y = np.minimum(np.maximum((xe[:N] * sp[:, None]).astype(F), -C), C)
    assert y.dtype == F and sp.dtype == F
    return y, sp, xe[N:], ge[N:]


def noise(n=3000, seed=1, scale=0.3):
    return (np.random.default_rng(seed).standard_normal((n, 2)) * scale).astype(F)


def _both(x, c, L, H, xh, gh, what):
    """one call through the model and the reference from the same state; everything on bits; returns the model's"""
    want = np_limiter(x, c, L, H, xh, gh)
    got = s2.limiter_reference(x, c, L, H, xh, gh)
    for g, w, name in zip(got, want, ("y", "gain", "xh", "gh")):
        assert g.shape == w.shape, (what, name)
        assert np.isfinite(g).all() and np.array_equal(bits(g), bits(w)), (what, name)
    return want


@pytest.mark.parametrize("L,H", PAIRS)
def test_reference_is_the_rule(L, H):
    """noise of 3000 frames under a ceiling that most of it exceeds: one call, and the same stream cut into calls of 7, 293, 1, 1699
    and 1000 frames with the state carried — every call equal to the model on bits, and the pieces equal to the one call"""
    x = noise()
    y, sp, xh, gh = _both(x, 0.25, L, H, None, None, "one call")
    assert (sp < 1.0).mean() > 0.25
    at, ys, sps, xh2, gh2 = 0, [], [], None, None
    for n in CUTS:
        yy, ss, xh2, gh2 = _both(x[at:at + n], 0.25, L, H, xh2, gh2, "cut at %d" % at)
        ys.append(yy), sps.append(ss)
        at += n
    assert at == len(x)
    assert np.array_equal(bits(np.concatenate(ys)), bits(y)) and np.array_equal(bits(np.concatenate(sps)), bits(sp))
    assert np.array_equal(bits(xh2), bits(xh)) and np.array_equal(bits(gh2), bits(gh))


@pytest.mark.parametrize("L,H", PAIRS)
def test_calls_shorter_than_the_histories(L, H):
    """calls of 1 frame, of fewer frames than L, of L, of fewer than G and of G frames: afterwards xh and gh are the last L and G
    entries of history followed by call"""
    G = 2 * L + H
    x = noise(4 * G + 8, seed=2)
    at, xh, gh = 0, None, None
    hist_x, hist_g = np.zeros((L, 2), F), np.ones(G, F)
    for n in [1, max(1, L - 1), L, 1, max(1, G - 1), G, 2]:
        seg = x[at:at + n]
        _, _, xh, gh = _both(seg, 0.25, L, H, xh, gh, "call of %d frames at %d" % (n, at))
        p = np.abs(seg).max(axis=1)
        hist_x = np.concatenate([hist_x, seg])[-L:]
        hist_g = np.concatenate([hist_g, np.where(p > F(0.25), F(0.25) / p, F(1)).astype(F)])[-G:]
        assert np.array_equal(bits(xh), bits(hist_x)) and np.array_equal(bits(gh), bits(hist_g)), n
        at += n


@pytest.mark.parametrize("L,H", [(5, 3), (64, 100), (257, 1)])
def test_reference_on_crafted_magnitudes(L, H):
    """samples no voice produces — the crafted magnitudes of tests/test_reverb_host.py: huge terms, the smallest normal, denormals and
    both zeros — once as they are under a ceiling of 0.25 and once times 2^28 (still finite) under the smallest ceiling, where
    C / p is a denormal and so are the sums of such gains; and uniform samples times 2^-130, denormals all, which pass as they are"""
    n = 600
    base = np.stack([np.resize(MIXED, n), np.resize(np.roll(MIXED, -3), n)], axis=1).astype(F)
    y, sp, _, _ = _both(base, 0.25, L, H, None, None, "mixed")
    assert (sp < 1.0).mean() > 0.9
    big = (base * F(2.0 ** 28)).astype(F)
    assert np.isfinite(big).all() and np.abs(big).max() > 2.0 ** 127
    y, sp, _, gh = _both(big, 2.0 ** -20, L, H, None, None, "mixed times 2^28")
    assert 0.0 < float(sp.min()) < 2.0 ** -126 and np.abs(y).max() <= F(2.0 ** -20)
    tiny = (np.random.default_rng(3).uniform(-1.0, 1.0, (n, 2)) * 2.0 ** -130).astype(F)
    y, sp, _, _ = _both(tiny, 2.0 ** -20, L, H, None, None, "denormals")
    assert np.array_equal(bits(y[L:]), bits(tiny[:n - L])) and bits(tiny).any()


@pytest.mark.parametrize("L,H", PAIRS)
def test_properties_without_a_model(L, H):
    """the reference alone: no output sample exceeds the ceiling; under a ceiling the signal never exceeds the output is the input
    delayed by L frames in every bit, behind L frames of +0.0, with a gain of exactly 1; the gains lie in (0, 1]"""
    x = noise()
    c = F(0.25)
    y, gain, _, _ = s2.limiter_reference(x, c, L, H)
    assert np.abs(y).max() <= c and (gain > 0.0).all() and (gain <= 1.0).all() and gain.min() < 1.0
    top = float(np.abs(x).max())
    for ceiling in (top, 10.0):
        y, gain, xh, gh = s2.limiter_reference(x, ceiling, L, H)
        assert np.array_equal(bits(y[L:]), bits(x[:len(x) - L])) and not bits(y[:L]).any()
        assert np.array_equal(bits(gain), bits(np.ones(len(x), F))) and np.array_equal(bits(gh), bits(np.ones(2 * L + H, F)))
        assert np.array_equal(bits(xh), bits(x[len(x) - L:]))


@pytest.mark.parametrize("L,H", [(1, 0), (5, 3), (48, 0), (64, 100)])
def test_the_shape_of_a_gain_reduction(L, H):
    """one frame of 1.0 in a signal of 0.125 under a ceiling of 0.5, so g is 0.5 there and 1 elsewhere: the gain is 1 until the
    ramp begins W frames before the peak comes out, falls along a line — k halves among W terms, k / W exactly representable sums —
    is 0.5 exactly from the frame the peak comes out for H frames more, and is back at 1 W frames later; the peak leaves as C"""
    n0, n, W = 700, 2000, L + 1
    x = np.full((n, 2), 0.125, dtype=F)
    x[n0, 1] = -1.0
    y, gain, _, _ = s2.limiter_reference(x, 0.5, L, H)
    out = n0 + L
    assert (gain[:out - L] == 1.0).all() and (gain[out:out + H + 1] == 0.5).all() and (gain[out + H + W:] == 1.0).all()
    down, up = gain[out - L - 1:out + 1], gain[out + H:out + H + W + 1]
    assert down[0] == 1.0 and (np.diff(down) < 0).all() and (np.diff(up) > 0).all()
    want = (F(W) - np.arange(1, W + 1).astype(F) * F(0.5)) / F(W)         # k halves and W - k ones: the sum is exact, the division rounds once
    assert np.array_equal(bits(down[1:]), bits(want))
    assert y[out, 1] == F(-0.5) and y[out, 0] == F(0.0625) and np.abs(y).max() == F(0.5)


@pytest.mark.parametrize("L,H", PAIRS)
def test_the_order_of_the_sum_is_visible(L, H):
    """the W terms added oldest first: s' differs in bits at more than a quarter of the frames for every pair with L >= 5; at L = 1
    it differs nowhere, two terms commute.  So a kernel that adds in another order cannot pass the parity tests."""
    x = noise()
    sp = np_limiter(x, 0.25, L, H)[1]
    other = np_limiter(x, 0.25, L, H, oldest_first=True)[1]
    differ = (bits(sp) != bits(other)).mean()
    if L == 1:
        assert differ == 0.0
    else:
        assert differ > 0.25, differ


@pytest.mark.parametrize("L,H", [(5, 3), (48, 0), (64, 100)])
def test_steps_four_and_five_are_needed(L, H):
    """without the minimum against g[n - L] and the clamp, the product x[n - L] * s[n] exceeds the ceiling in at least one frame: the
    rounded mean can lie above the gain the peak needs.  With them the reference holds the ceiling on the same input."""
    x = noise()
    c = F(0.25)
    s, gd, xd = np_limiter(x, c, L, H, parts=True)
    raw = (xd * s[:, None]).astype(F)
    assert (np.abs(raw).max(axis=1) > c).sum() >= 1
    y, gain, _, _ = s2.limiter_reference(x, c, L, H)
    assert np.abs(y).max() <= c and np.array_equal(bits(gain), bits(np.minimum(s, gd)))


@pytest.mark.parametrize("L,H", PAIRS)
def test_model_and_reference_lie_around_a_float64_evaluation(L, H):
    """the rule with no float32 arithmetic in it: g64 = C / p, the window minima, their plain mean, the minimum against g64[n - L],
    the product, the clamp.  A float32 g errs by one rounding, u = 2^-24 relative; a minimum selects, it does not round; the sum adds
    W non-negative terms with at most W - 1 roundings (the first lands on +0.0) and the division is one more: s lies within
    gamma_n * s64 of s64 with n = W + 1 and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms,
    section 3.1), and min(a, b) moves by no more than the larger move of a and b.  The product adds one rounding, and the clamp
    moves nothing apart.  No gain is below 2^-100 here, so nothing underflows."""
    x = noise()
    c = F(0.25)
    N, W, G = len(x), L + 1, 2 * L + H
    x64, c64 = x.astype(np.float64), float(c)
    p = np.abs(x64).max(axis=1)
    g = np.where(p > c64, c64 / np.maximum(p, 1e-300), 1.0)
    ge, xe = np.concatenate([np.ones(G), g]), np.concatenate([np.zeros((L, 2)), x64])
    m = sliding_window_view(ge, L + H + 1).min(axis=1)
    s64 = np.convolve(m, np.ones(W))[W - 1:W - 1 + N] / W        # the mean of m[j .. j + L], j = n
    gd = ge[G - L:G - L + N]
    sp64 = np.minimum(s64, gd)
    y64 = np.clip(xe[:N] * sp64[:, None], -c64, c64)
    u = 2.0 ** -24
    n_r = W + 1
    gamma = n_r * u / (1.0 - n_r * u)
    bound_s = gamma * np.maximum(s64, gd)
    bound_y = np.abs(xe[:N]) * bound_s[:, None] + u * np.abs(xe[:N]) * (sp64 + bound_s)[:, None]
    assert ge.min() > 2.0 ** -100
    for name, (y, sp, _, _) in (("model", np_limiter(x, c, L, H)), ("reference", s2.limiter_reference(x, c, L, H))):
        assert (np.abs(sp.astype(np.float64) - sp64) <= bound_s).all(), name
        assert (np.abs(y.astype(np.float64) - y64) <= bound_y).all(), name
    assert bound_s.max() < 2e-4                                  # the bound says something: s' lies in (0, 1]


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
    """the setter and the reference look at the values before they look at the handle or the buffers, so the range checks answer
    without a device; S2R_ERR_INVALID is what no handle gets for values in range.  With a device the rest runs on a real handle
    (check_ranges, also called by tests/test_gpu_limiter.py)."""
    L = s2.load_library()
    assert (s2.LIMITER_MAX_LOOKAHEAD, s2.LIMITER_MAX_HOLD, s2.LIMITER_CEILING_LOG2) == (1024, 4096, 20)
    x, y, gain = np.zeros((4, 2), dtype=F), np.zeros((4, 2), dtype=F), np.zeros(4, dtype=F)
    for c, la, hold in BAD:
        assert L.s2r_set_master_limiter(None, c, la, hold) == s2s.S2R_ERR_PATCH_RANGE, (c, la, hold)
        assert L.s2r_limiter_reference(_p(x), 4, c, la, hold, None, None, _p(y), _p(gain)) == s2s.S2R_ERR_PATCH_RANGE, (c, la, hold)
    for c, la, hold in GOOD:
        assert L.s2r_set_master_limiter(None, c, la, hold) == s2s.S2R_ERR_INVALID, (c, la, hold)
        xh, gh = np.zeros((la, 2), dtype=F), np.ones(2 * la + hold, dtype=F)
        assert L.s2r_limiter_reference(_p(x), 4, c, la, hold, None, _p(gh), _p(y), _p(gain)) == s2s.S2R_ERR_INVALID
        assert L.s2r_limiter_reference(_p(x), 4, c, la, hold, _p(xh), None, _p(y), _p(gain)) == s2s.S2R_ERR_INVALID
        assert L.s2r_limiter_reference(None, 4, c, la, hold, _p(xh), _p(gh), _p(y), _p(gain)) == s2s.S2R_ERR_INVALID
        assert L.s2r_limiter_reference(None, 0, c, la, hold, _p(xh), _p(gh), None, None) == s2s.S2R_OK        # no frames: nothing moves
        assert not bits(xh).any() and (gh == 1.0).all()
        assert L.s2r_limiter_reference(_p(x), 4, c, la, hold, _p(xh), _p(gh), None, None) == s2s.S2R_OK       # the outputs may be null
    f, n = C.c_float(), C.c_uint32()
    assert L.s2r_clear_master_limiter(None) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_master_limiter(None, C.byref(f), C.byref(n), C.byref(n)) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_limiter_state(None, _p(x), 8, _p(gain), 4) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_limiter_state(None, _p(x), 8, _p(gain), 4) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_limiter_meters(None, C.byref(f), C.byref(f)) == s2s.S2R_ERR_INVALID
    with pytest.raises(s2.S2rError) as err:
        s2.limiter_reference(x, 0.25, 0, 0)
    assert err.value.status == s2s.S2R_ERR_PATCH_RANGE
    with pytest.raises(ValueError):
        s2.limiter_reference(np.zeros((4, 3), dtype=F), 0.25, 4, 0)
    with pytest.raises(ValueError):
        s2.limiter_reference(x, 0.25, 4, 0, xh=np.zeros((3, 2), dtype=F))
    # the arguments of the Python mirror are not modified: the state comes back as new arrays
    xh, gh = np.zeros((4, 2), dtype=F), np.ones(9, dtype=F)
    s2.limiter_reference(np.ones((6, 2), dtype=F), 0.25, 4, 1, xh, gh)
    assert not bits(xh).any() and (gh == 1.0).all()
    assert L.s2r_abi_version() == 4
    syn = _new_or_skip(num_voices=8, max_frames=64)
    if syn is not None:
        check_ranges(syn)


def check_ranges(syn):
    """the entries on a real handle that makes no fill: the state lives on the host until the first master fill"""
    L, h = syn.L, syn.h
    buf, gbuf = np.zeros(32, dtype=F), np.zeros(32, dtype=F)
    f = C.c_float()
    assert syn.get_master_limiter() == (0.0, 0, 0)               # a fresh handle: off
    assert L.s2r_get_limiter_state(h, _p(buf), 32, _p(gbuf), 32) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_limiter_state(h, _p(buf), 0, _p(gbuf), 0) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_limiter_meters(h, C.byref(f), C.byref(f)) == s2s.S2R_ERR_INVALID
    for c, la, hold in BAD:
        assert L.s2r_set_master_limiter(h, c, la, hold) == s2s.S2R_ERR_PATCH_RANGE, (c, la, hold)
    assert syn.get_master_limiter() == (0.0, 0, 0)               # a refused call changes nothing
    syn.clear_master_limiter()                                   # removing what is not there is no error
    syn.set_master_limiter(0.5, 4, 3)
    assert syn.get_master_limiter() == (0.5, 4, 3)
    assert L.s2r_get_master_limiter(h, None, None, None) == s2s.S2R_OK        # any pointer may be null
    xh, gh = syn.limiter_state()
    assert xh.shape == (4, 2) and gh.shape == (11,) and not bits(xh).any() and (gh == 1.0).all()
    for n_x, n_g in ((7, 11), (9, 11), (8, 10), (8, 12), (0, 0)):
        assert L.s2r_set_limiter_state(h, _p(buf), n_x, _p(gbuf), n_g) == s2s.S2R_ERR_INVALID, (n_x, n_g)
    for n_x, n_g in ((7, 11), (8, 10), (0, 0)):
        assert L.s2r_get_limiter_state(h, _p(buf), n_x, _p(gbuf), n_g) == s2s.S2R_ERR_INVALID, (n_x, n_g)
    assert L.s2r_get_limiter_state(h, _p(buf), 32, _p(gbuf), 32) == s2s.S2R_OK            # larger buffers will do
    assert L.s2r_set_limiter_state(h, None, 8, _p(gbuf), 11) == s2s.S2R_ERR_INVALID
    assert L.s2r_set_limiter_state(h, _p(buf), 8, None, 11) == s2s.S2R_ERR_INVALID
    assert L.s2r_get_limiter_state(h, None, 8, _p(gbuf), 11) == s2s.S2R_ERR_INVALID
    new_x, new_g = np.arange(8, dtype=F).reshape(4, 2) - F(3.5), np.linspace(0.25, 1.0, 11, dtype=F)
    for bad in (1.5, -0.25, NAN):                                # gh holds gains: each in [0, 1]
        g = new_g.copy()
        g[5] = bad
        assert L.s2r_set_limiter_state(h, _p(new_x), 8, _p(g), 11) == s2s.S2R_ERR_PATCH_RANGE
    syn.set_limiter_state(new_x, new_g)
    xh, gh = syn.limiter_state()
    assert np.array_equal(bits(xh), bits(new_x)) and np.array_equal(bits(gh), bits(new_g))
    syn.set_master_limiter(0.25, 4, 3)                           # the ceiling alone: the state stays
    xh, gh = syn.limiter_state()
    assert syn.get_master_limiter() == (0.25, 4, 3) and np.array_equal(bits(xh), bits(new_x)) and np.array_equal(bits(gh), bits(new_g))
    # the limiter belongs to the handle: a new bank and a program change leave it alone
    syn.set_patch_bank([s2.default_patch()] * 3)
    syn.program_change(2)
    xh, gh = syn.limiter_state()
    assert syn.get_master_limiter() == (0.25, 4, 3) and np.array_equal(bits(xh), bits(new_x)) and np.array_equal(bits(gh), bits(new_g))
    syn.set_master_limiter(0.25, 4, 2)                           # another hold: the initial state
    xh, gh = syn.limiter_state()
    assert gh.shape == (10,) and not bits(xh).any() and (gh == 1.0).all()
    syn.set_limiter_state(new_x, new_g[:10])
    syn.set_master_limiter(0.25, 5, 2)                           # another lookahead likewise
    xh, gh = syn.limiter_state()
    assert xh.shape == (5, 2) and gh.shape == (12,) and not bits(xh).any() and (gh == 1.0).all()
    assert L.s2r_get_limiter_meters(h, C.byref(f), C.byref(f)) == s2s.S2R_ERR_INVALID     # no master fill has run it
    syn.clear_master_limiter()
    assert syn.get_master_limiter() == (0.0, 0, 0)
    assert L.s2r_get_limiter_state(h, _p(buf), 32, _p(gbuf), 32) == s2s.S2R_ERR_INVALID
