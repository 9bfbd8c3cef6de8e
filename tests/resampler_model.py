"""The sample-rate converter's rule (include/s2r.h) restated in numpy for the tests: float32 element-wise, vectorised over
the output frames of a call, every product and every sum an operation of its own; and the designer restated in float64 with np.kaiser
and np.sinc.  Nothing here calls the library."""
import numpy as np

F = np.float32
CH = 18
MASTER = 8


def count_of(L, M, ph, frames):
    return 0 if frames * L <= ph else -(-(frames * L - ph) // M)


def channels(stems, master):
    """[18, frames] float32: row 2 p + c; a bus past the stems' is +0.0"""
    master = np.asarray(master, dtype=F).reshape(-1, 2)
    x = np.zeros((CH, master.shape[0]), dtype=F)
    if stems is not None:
        for p in range(len(stems)):
            x[2 * p], x[2 * p + 1] = stems[p][:, 0], stems[p][:, 1]
    x[16], x[17] = master[:, 0], master[:, 1]
    return x


class Model:
    """state [18, T - 1] newest first and ph, carried from call to call"""

    def __init__(self, L, M, table, chains=4):
        self.L, self.M, self.table = L, M, np.asarray(table, dtype=F)
        self.T = self.table.shape[1]
        self.chains = chains
        self.reset()

    def reset(self):
        self.state, self.ph = np.zeros((CH, self.T - 1), dtype=F), 0

    def call(self, stems, master):
        """[9, count, 2] float32"""
        x = channels(stems, master)
        n_frames, H = x.shape[1], self.T - 1
        xs = np.concatenate([self.state[:, ::-1], x], axis=1)    # oldest first: x[n] = xs[:, H + n]
        count = count_of(self.L, self.M, self.ph, n_frames)
        u = self.ph + np.arange(count, dtype=np.int64) * self.M
        n, p = u // self.L, u % self.L
        acc = [np.zeros((CH, count), dtype=F) for _ in range(self.chains)]
        for k in range(self.T):
            t = self.table[p, k][None, :] * xs[:, H + n - k]
            assert t.dtype == F
            acc[k % self.chains] = acc[k % self.chains] + t
        if self.chains == 4:
            y = (acc[0] + acc[1]) + (acc[2] + acc[3])
        else:
            y = acc[0]
        self.state = xs[:, ::-1][:, :H].copy()
        self.ph = self.ph + count * self.M - n_frames * self.L
        assert 0 <= self.ph < self.M and y.dtype == F
        return np.stack([y[0::2], y[1::2]], axis=2)


def design64(L, M, T, beta, rolloff):
    """the prototype g[L T] and the table h[L, T] in float64, rows of sum 1"""
    N = L * T
    c = (N - 1) / 2.0
    fc = rolloff * 0.5 / max(L, M)
    i = np.arange(N, dtype=np.float64)
    g = 2.0 * fc * L * np.sinc(2.0 * fc * (i - c)) * np.kaiser(N, beta)
    h = g.reshape(T, L).T.copy()
    return g, h / h.sum(axis=1, keepdims=True)


def response_db(table, L, M, n_fft=1 << 18):
    """(worst passband high, worst passband low, worst stopband) in dB of the interleaved prototype g[k L + p] = h[p][k], gain L taken
    out: the passband up to 0.8 of the lower Nyquist, the stopband from 1.2 of it, frequencies in cycles per sample at the rate L times the input's"""
    table = np.asarray(table, dtype=np.float64)
    g = table.T.reshape(-1)
    mag = np.abs(np.fft.rfft(g, n_fft)) / L
    f = np.arange(mag.size) / n_fft
    nyq = 0.5 / max(L, M)
    db = 20.0 * np.log10(np.maximum(mag, 1e-300))
    pb, sb = db[f <= 0.8 * nyq], db[f >= 1.2 * nyq]
    return float(pb.max()), float(pb.min()), float(sb.max())
