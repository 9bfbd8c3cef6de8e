"""The master multiband compressor's rule restated without the library, for tests/test_multiband_host.py and
tools/multiband_truth.py: the crossover's graph, a binary32 frame loop in numpy scalars, and a binary64 evaluation of the tree and of
the allpass cascade the unit-gain band sum equals (scipy.signal.lfilter on float64)."""
import numpy as np
from scipy.signal import lfilter

F = np.float32
POINTS = 513
LO = 0x33800000                                                  # the bits of 2^-24


def sections(B):
    return 4 * (B - 1) + (B - 1) * (B - 2) // 2


def graph(B):
    """([(source section or -1 for x, 'lp' | 'hp' | 'ap', row)], [the section that leaves band j, or -1]) in the state's order"""
    secs = []
    for k in range(B - 1):
        r = 4 * (k - 1) + 3 if k else -1
        secs += [(r, "lp", k), (4 * k, "lp", k), (r, "hp", k), (4 * k + 2, "hp", k)]
    leaf = [4 * j + 1 for j in range(B - 1)] + [4 * (B - 2) + 3 if B > 1 else -1]
    for j in range(B - 2):
        for k in range(j + 1, B - 1):
            secs.append((leaf[j], "ap", k - 1))
            leaf[j] = len(secs) - 1
    assert len(secs) == sections(B)
    return secs, leaf


def design64(sample_rate, splits):
    """cookbook low-pass, high-pass and allpass rows at Q = 1 / sqrt 2 in binary64, (b0, b1, b2, a1, a2) over a0: (lp, hp, ap_all) with
    an allpass row for EVERY split (the rule's ap is ap_all[1:])"""
    lp, hp, ap = [], [], []
    for f in splits:
        w0 = 2.0 * np.pi * f / sample_rate
        cw, alpha = np.cos(w0), np.sin(w0) / np.sqrt(2.0)
        a0, a1, a2 = 1.0 + alpha, -2.0 * cw, 1.0 - alpha
        lp.append(np.array([(1.0 - cw) / 2.0, 1.0 - cw, (1.0 - cw) / 2.0, a1, a2]) / a0)
        hp.append(np.array([(1.0 + cw) / 2.0, -(1.0 + cw), (1.0 + cw) / 2.0, a1, a2]) / a0)
        ap.append(np.array([a2, a1, a0, a1, a2]) / a0)
    return np.array(lp).reshape(-1, 5), np.array(hp).reshape(-1, 5), np.array(ap).reshape(-1, 5)


def _run64(q, x):
    return lfilter(q[:3], np.concatenate([[1.0], q[3:]]), x, axis=0)


def tree64(B, lp, hp, ap, x):
    """the B band signals of the rule's steps 1 and 2 in binary64: [B, frames, 2]; ap is the rule's (rows for splits 1 ..)"""
    rows = {"lp": np.asarray(lp, dtype=np.float64), "hp": np.asarray(hp, dtype=np.float64), "ap": np.asarray(ap, dtype=np.float64)}
    secs, leaf = graph(B)
    x = np.asarray(x, dtype=np.float64)
    v = []
    for src, kind, row in secs:
        v.append(_run64(rows[kind][row], x if src < 0 else v[src]))
    return np.stack([x if l < 0 else v[l] for l in leaf])


def allpass64(ap_all, x):
    """AP_{n-1}( ... AP_1(AP_0(x))) in binary64: what the unit-gain band sum of n + 1 bands equals"""
    y = np.asarray(x, dtype=np.float64)
    for q in np.asarray(ap_all, dtype=np.float64):
        y = _run64(q, y)
    return y


def target32(curve, p):
    """the dynamics' step 2 for one level, in binary32 operations"""
    if not p >= F(2.0 ** -24):
        return curve[0]
    if p >= F(256.0):
        return curve[POINTS - 1]
    u = int(np.array([p], dtype=F).view(np.uint32)[0]) - LO
    i, f = u >> 19, F(u & 0x7FFFF) * F(2.0 ** -19)
    return F(curve[i] + F(f * F(curve[i + 1] - curve[i])))


def np32(B, lp, hp, ap, curves, att, rel, x, state):
    """the whole rule, frame by frame, every operation a binary32 numpy operation (both channels of a section as one array of two):
    (out [frames, 2], the state after the call, the bands' minima, the bands in front of the gains [B, frames, 2])"""
    rows = {"lp": np.asarray(lp, dtype=F).reshape(-1, 5), "hp": np.asarray(hp, dtype=F).reshape(-1, 5), "ap": np.asarray(ap, dtype=F).reshape(-1, 5)}
    secs, leaf = graph(B)
    S = len(secs)
    st = np.array(state, dtype=F)
    s1 = [st[4 * i:4 * i + 2].copy() for i in range(S)]
    s2 = [st[4 * i + 2:4 * i + 4].copy() for i in range(S)]
    y = [F(v) for v in st[4 * S:]]
    x = np.asarray(x, dtype=F)
    n = x.shape[0]
    out, bands, mn = np.empty((n, 2), dtype=F), np.empty((B, n, 2), dtype=F), [F(np.inf)] * B
    curves, att, rel = np.asarray(curves, dtype=F), np.asarray(att, dtype=F), np.asarray(rel, dtype=F)
    with np.errstate(all="ignore"):
        for t in range(n):
            v = []
            for i, (src, kind, row) in enumerate(secs):
                b0, b1, b2, a1, a2 = rows[kind][row]
                xi = x[t] if src < 0 else v[src]
                yi = b0 * xi + s1[i]
                s1[i] = (b1 * xi - a1 * yi) + s2[i]
                s2[i] = b2 * xi - a2 * yi
                v.append(yi)
            acc = None
            for j in range(B):
                band = x[t] if leaf[j] < 0 else v[leaf[j]]
                bands[j, t] = band
                p = np.abs(band).max()
                tg = target32(curves[j], p)
                a = att[j] if tg < y[j] else rel[j]
                y[j] = F(tg + F(a * F(y[j] - tg)))
                mn[j] = y[j] if y[j] < mn[j] else mn[j]
                o = band * y[j]
                acc = o if acc is None else acc + o
            out[t] = acc
    for i in range(S):
        st[4 * i:4 * i + 2], st[4 * i + 2:4 * i + 4] = s1[i], s2[i]
    st[4 * S:] = y
    return out, st, np.array(mn, dtype=F), bands
