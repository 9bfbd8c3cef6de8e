"""Plain binary64 models of the blocks that have no reference caller — the dsp_filters.rs filters, the SVF outputs, the DPW
oscillators, the 4x decimator — written from the textbook definitions (bilinear transform of the analog prototypes, RBJ's
cookbook biquads, a windowed sinc, the closed form of a differentiated parabola), NOT from oracle/ or csrc/.  numpy only: this
module imports neither the oracle nor synth2_amd, so that what it says can be held against both.

Also here, because the CPU half (tests/test_truth_blocks.py), the GPU half (tests/test_gpu_truth_blocks.py) and the measuring
script (tools/truth_blocks.py) must agree on it to the letter: the case table, as plain data."""
import collections

import numpy as np

# s2r_filter_kind / s2r_osc_kind (include/s2r.h), restated as data
ONEPOLE, LP1, HP1, LP2, HP2, BP2, SVF_LP, SVF_BP, SVF_HP = range(9)
KIND_NAMES = ["onepole", "lp1", "hp1", "lp2", "hp2", "bp2", "svf_lp", "svf_bp", "svf_hp"]
OSC_SQUARE, OSC_SAW, OSC_TRIANGLE, OSC_SINE, OSC_DPW_SAW, OSC_DPW_SQUARE, OSC_DPW_TRIANGLE = range(7)
USES_Q = (BP2, SVF_LP, SVF_BP, SVF_HP)          # the parameter is lpf_q; LP2 / HP2 take lpf_damping; the others none

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- filters

def coefficients(kind, fc, p, sr):
    """(b[3], a[3]) in binary64, a[0] == 1, of filter `kind` at cutoff `fc` Hz (a float: an f32 value, or the f64 product of
    one with a modulation factor), parameter `p` (an f32 value) and sample rate `sr`."""
    fc, p, sr = float(fc), float(p), float(sr)
    if kind in (SVF_LP, SVF_BP, SVF_HP):
        fc = min(fc, float(F32(0.49)) * sr)
    th = 2.0 * np.pi * fc / sr
    if kind == ONEPOLE:
        x = np.exp(-th)
        return np.array([1.0 - x, 0.0, 0.0]), np.array([1.0, -x, 0.0])
    if kind in (LP1, HP1):
        K = np.tan(th / 2.0)
        b = np.array([K, K, 0.0]) if kind == LP1 else np.array([1.0, -1.0, 0.0])
        return b / (1.0 + K), np.array([1.0, (K - 1.0) / (1.0 + K), 0.0])
    if kind == BP2:
        t = np.tan(th / (2.0 * p))
        return np.array([t, 0.0, -t]) / (1.0 + t), np.array([1.0, -2.0 * np.cos(th) / (1.0 + t), (1.0 - t) / (1.0 + t)])
    Q = 1.0 / p if kind in (LP2, HP2) else p
    c, al = np.cos(th), np.sin(th) / (2.0 * Q)
    a = np.array([1.0, -2.0 * c / (1.0 + al), (1.0 - al) / (1.0 + al)])
    if kind in (LP2, SVF_LP):
        b = np.array([(1.0 - c) / 2.0, 1.0 - c, (1.0 - c) / 2.0])
    elif kind in (HP2, SVF_HP):
        b = np.array([(1.0 + c) / 2.0, -(1.0 + c), (1.0 + c) / 2.0])
    else:
        b = np.array([Q * al, 0.0, -Q * al])
    return b / (1.0 + al), a


def run_biquads(b, a, x):
    """y[c, n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2] in binary64 from zero state.  b, a: (cases, 3);
    x: (frames,) shared by all cases, or (cases, frames)."""
    b, a = np.atleast_2d(np.asarray(b, dtype=np.float64)), np.atleast_2d(np.asarray(a, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64)
    n_cases = b.shape[0]
    if x.ndim == 1:
        x = np.broadcast_to(x, (n_cases, x.size))
    xt = np.ascontiguousarray(x.T)
    y = np.empty_like(xt)
    b0, b1, b2, a1, a2 = b[:, 0].copy(), b[:, 1].copy(), b[:, 2].copy(), a[:, 1].copy(), a[:, 2].copy()
    x1 = x2 = y1 = y2 = np.zeros(n_cases)
    for n in range(xt.shape[0]):
        x0 = xt[n]
        y0 = b0 * x0 + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        y[n] = y0
        x2, x1, y2, y1 = x1, x0, y1, y0
    return np.ascontiguousarray(y.T)


def deviation(rows, truth):
    """per case: max over frames of |row - truth| / running peak of |truth| (tests/test_truth_model.py's unit, as a ratio)"""
    truth = np.atleast_2d(truth)
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    peak = np.maximum.accumulate(np.maximum(np.abs(truth), 1e-30), axis=1)
    return np.max(np.abs(rows - truth) / peak, axis=1)


# ---------------------------------------------------------------------------------------------------------------- case table

Case = collections.namedtuple("Case", "kind lpf_freq p amount")     # amount: mod_env_to_lpf_freq (mod env held at 0.5)
RATES = (48000, 192000)
CUTOFFS = {48000: (300.0, 1000.0, 5000.0, 15000.0), 192000: (1000.0, 5000.0, 15000.0, 30000.0)}
PARAMS = (0.3, 1.41421354, 3.0, 9.0)
INPUTS = (("saw", OSC_SAW, 440.0), ("sine", OSC_SINE, 1234.5))     # the oscillator ahead of the filter, and its pitch in Hz
MOD_SUSTAIN = 0.5
DECOY = 0.77              # what the parameter a kind does NOT read is set to: a filter that reads the wrong one misses every bound
CALLS, CALL_FRAMES = 4, 1024
SINGLE_FC, SINGLE_P, SINGLE_CALLS, SINGLE_VOICES = 1000.0, 3.0, 2, 64
SINGLE_NOTES = tuple(range(36, 36 + SINGLE_VOICES))
SINGLE_OSCS = (OSC_SAW, OSC_SINE, OSC_SQUARE, OSC_TRIANGLE)         # kind k of the single-patch form plays SINGLE_OSCS[k % 4]
BOUND_FACTOR, BOUND_CEILING = 2.0, 1e-3
BOUND_FLOOR = 2.0 ** -24  # an f32 row differs from ANY binary64 value by up to half an ulp of itself, <= 2^-24 of the peak


def case_cutoff(case):
    """the cutoff the truth filters at, in binary64: 2^(amount * 0.5) * lpf_freq"""
    return 2.0 ** (float(F32(case.amount)) * MOD_SUSTAIN) * float(F32(case.lpf_freq))


def filter_cases(sr):
    """All nine kinds at the rate's four cutoffs and four parameters (one case per cutoff for the kinds without a parameter),
    the SVF kinds at 30 kHz (above the 0.49 sr clamp at 48 kHz), less the BP2 cases whose theta / (2 q) reaches pi / 4; six
    cases under a constant modulated cutoff; and the reciprocal pairs SVF(q) / LP2, HP2(d = 1 / q), q a power of two."""
    out = []
    for kind in range(9):
        has_p = kind in (LP2, HP2) + USES_Q
        fcs = list(CUTOFFS[sr])
        if kind in (SVF_LP, SVF_BP, SVF_HP) and 30000.0 not in fcs:
            fcs.append(30000.0)
        for fc in fcs:
            for p in (PARAMS if has_p else (0.0,)):
                if kind == BP2 and 2.0 * np.pi * float(F32(fc)) / sr / (2.0 * float(F32(p))) >= np.pi / 4.0:
                    continue
                out.append(Case(kind, fc, p, 0.0))
    for kind in (ONEPOLE, LP2, SVF_BP):
        out.append(Case(kind, 1000.0, 3.0, 4.0))          # -> 4 kHz
        out.append(Case(kind, 8000.0, 3.0, -6.0))         # -> 1 kHz
    for fc in (1000.0, 5000.0):
        for q in (2.0, 0.5):
            out += [Case(SVF_LP, fc, q, 0.0), Case(LP2, fc, 1.0 / q, 0.0), Case(SVF_HP, fc, q, 0.0), Case(HP2, fc, 1.0 / q, 0.0)]
    assert len(set(out)) == len(out)
    return out


def reciprocal_pairs(cases):
    """index pairs (SVF case, LP2 / HP2 case) of one and the same truth: Q = q = 1 / d exactly"""
    at = {c: i for i, c in enumerate(cases)}
    pairs = []
    for c in cases:
        if c.kind in (SVF_LP, SVF_HP) and c.amount == 0.0 and c.p in (2.0, 0.5):
            twin = Case(LP2 if c.kind == SVF_LP else HP2, c.lpf_freq, 1.0 / c.p, 0.0)
            if twin in at:
                pairs.append((at[c], at[twin]))
    return pairs


def case_key(sr, input_name, case):
    return "%d/%s/%s/fc=%g/p=%.9g/mod=%g" % (sr, input_name, KIND_NAMES[case.kind], case.lpf_freq, float(F32(case.p)), case.amount)


def patch_fields(case, osc_kind):
    """the sc::Layer fields of a case's patch (the rest stay at their defaults): gain 1 from frame 0, the mod envelope a
    constant 0.5, no pitch modulation, the parameter the kind does not read set to DECOY"""
    f = {"osc_kind": osc_kind, "lpf_kind": case.kind, "lpf_freq": case.lpf_freq, "mod_env_to_osc_freq": 0.0,
         "mod_env_to_lpf_freq": case.amount, "lpf_damping": DECOY, "lpf_q": DECOY,
         "amp_env.attack_ms": 0.0, "amp_env.decay_ms": 0.0, "amp_env.sustain": 1.0,
         "mod_env.attack_ms": 0.0, "mod_env.decay_ms": 0.0, "mod_env.sustain": MOD_SUSTAIN}
    if case.kind in USES_Q:
        f["lpf_q"] = case.p
    elif case.kind in (LP2, HP2):
        f["lpf_damping"] = case.p
    return f


PASS_THROUGH = Case(ONEPOLE, 1e9, 0.0, 0.0)   # x = exp(-huge) = 0: y = fma(1, input, +-0) = the filter's input, exactly


def truth_rows(cases, sr, row_a):
    """the binary64 filters of `cases` applied to the pass-through twin's row"""
    ba = [coefficients(c.kind, case_cutoff(c), F32(c.p), sr) for c in cases]
    return run_biquads([x[0] for x in ba], [x[1] for x in ba], row_a)


def bounds_for(table, keys):
    """committed deviations -> the bound of each case: twice the oracle's own, at least what the f32 format costs any row,
    and never above the ceiling (a case that needs more is ill-conditioned in f32 direct form and has no place in the table)"""
    b = np.array([max(BOUND_FACTOR * table[k], BOUND_FLOOR) for k in keys])
    assert np.all(b <= BOUND_CEILING), [k for k, v in zip(keys, b) if v > BOUND_CEILING]
    return b


# ---------------------------------------------------------------------------------------------------------------- decimator

DECIM_TAPS, DECIM_FC = 63, 0.115


def decimator_taps():
    k = np.arange(DECIM_TAPS, dtype=np.float64)
    h = 2.0 * DECIM_FC * np.sinc(2.0 * DECIM_FC * (k - (DECIM_TAPS - 1) // 2)) * np.blackman(DECIM_TAPS)
    return h / h.sum()


def decimate4(x_with_history):
    """x: 62 samples of history followed by 4 n new ones -> (out[n] = sum_k h[k] x[4 n + k], sum_k |h[k]| |x[4 n + k]|)"""
    x = np.asarray(x_with_history, dtype=np.float64)
    n = (x.size - (DECIM_TAPS - 1)) // 4
    assert x.size == DECIM_TAPS - 1 + 4 * n
    idx = 4 * np.arange(n)[:, None] + np.arange(DECIM_TAPS)[None, :]
    h = decimator_taps()
    return x[idx] @ h, np.abs(x[idx]) @ np.abs(h)


DECIM_BOUND_ULPS = 66.0 * 2.0 ** -24      # 63 sequentially accumulated products and the f32 rounding of the taps, first order
DECIM_CALLS = (256, 1, 3, 17, 255)


# ---------------------------------------------------------------------------------------------------------------- DPW

DPW_PAIRS = ((OSC_SAW, OSC_DPW_SAW), (OSC_SQUARE, OSC_DPW_SQUARE), (OSC_TRIANGLE, OSC_DPW_TRIANGLE))
DPW_PITCHES = {48000: (110.0, 220.0, 440.0), 192000: (440.0,)}
DPW_NOTES = {110.0: 45, 220.0: 57, 440.0: 69}
DPW_FRAMES = 4096


NAIVE_AT_PHASE_ZERO = 1.0   # saw 1 - 2 phase, square +1 in the first half, triangle 1 - 4 phase: all start at +1


def dpw_expectation(naive_kind, pitch_hz, sr, n_frames=DPW_FRAMES):
    """(expected DPW row - naive row, frames compared, tolerance): the closed form away from the naive shape's
    discontinuities; the mask comes from the frame index alone."""
    period = float(F32(sr)) / float(F32(pitch_hz))
    n = np.arange(n_frames, dtype=np.float64)
    phase = np.mod(n / period, 1.0)
    guard = 2.0 / period + n_frames * 2.0 ** -23
    dist = np.minimum(phase, 1.0 - phase)
    if naive_kind != OSC_SAW:
        dist = np.minimum(dist, np.abs(phase - 0.5))
    keep = dist > guard
    keep[0] = False                                     # frame 0 is checked on its own: y[0] = 0
    if naive_kind == OSC_SAW:
        want = np.full(n_frames, 1.0 / period)
    elif naive_kind == OSC_SQUARE:
        want = np.zeros(n_frames)
    else:
        want = np.where(phase < 0.5, 2.0 / period, -2.0 / period)
    return want, keep, 4.0 * period * 2.0 ** -24 + 2.0 ** -21


def dpw_compare(dpw_row, naive_row, naive_kind, pitch_hz, sr):
    """(worst error of the compared frames, frame 0's error, both in units of the tolerance; share of frames compared)"""
    want, keep, tol = dpw_expectation(naive_kind, pitch_hz, sr, len(dpw_row))
    d = np.asarray(dpw_row, dtype=np.float64) - np.asarray(naive_row, dtype=np.float64)
    return float(np.abs(d - want)[keep].max() / tol), float(abs(d[0] + NAIVE_AT_PHASE_ZERO) / tol), float(keep.mean())
