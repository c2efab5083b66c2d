"""Float64 NumPy restatements of the three rules of K32 (include/morgana_hip.h, csrc/vocoder.hip), and nothing else: the mel-cepstrum's
log spectrum through the warped cosine basis, the band aperiodicity's interpolation in dB, and the first-order Savitzky-Golay
smoothing of exp(lf0) with its voicing gate.  Written from the header's text, not from the kernel or the Python wrappers."""
import numpy as np


def warped_frequencies(alpha, fft_size):
    """w~_k of the fft_size / 2 + 1 bins: w_k = 2 pi k / F through the all-pass of alpha."""
    w = 2.0 * np.pi * np.arange(fft_size // 2 + 1, dtype=np.float64) / float(fft_size)
    return w + 2.0 * np.arctan(alpha * np.sin(w) / (1.0 - alpha * np.cos(w)))


def basis(order, alpha, fft_size):
    """basis[m, k] = cos(m w~_k), float64."""
    return np.cos(np.arange(order, dtype=np.float64)[:, None] * warped_frequencies(alpha, fft_size)[None, :])


def log_spectrum(c, alpha, fft_size):
    """L[t, k] = sum_m c[t, m] basis[m, k] for c (n, M) -> (n, F / 2 + 1)."""
    c = np.asarray(c, dtype=np.float64)
    return c @ basis(c.shape[1], alpha, fft_size)


def spectrum(c, alpha, fft_size):
    return np.exp(2.0 * log_spectrum(c, alpha, fft_size))


def aperiodicity(bap, sample_rate, fft_size):
    """bap (n, Nb) dB -> (n, F / 2 + 1): clamp to [-60, 0], anchors (0, -60), (3000 i, bap[:, i - 1]), (fs / 2, 0), linear in dB at
    f_k = k fs / F, then exp(dB ln10 / 20)."""
    bap = np.clip(np.asarray(bap, dtype=np.float64), -60.0, 0.0)
    n, nb = bap.shape
    assert 3000 * nb < sample_rate / 2.0
    xs = np.concatenate(([0.0], 3000.0 * np.arange(1, nb + 1), [sample_rate / 2.0]))
    f = np.arange(fft_size // 2 + 1, dtype=np.float64) * float(sample_rate) / float(fft_size)
    out = np.empty((n, f.size), dtype=np.float64)
    for t in range(n):
        ys = np.concatenate(([-60.0], bap[t], [0.0]))
        out[t] = np.exp(np.interp(f, xs, ys) * (np.log(10.0) / 20.0))
    return out


def smooth(y, window):
    """The smoothing rule on one column y (n,) float64: the moving average inside, the least-squares line of the first / last
    `window` values on the first / last h frames; n < window or window == 1: y itself."""
    y = np.asarray(y, dtype=np.float64)
    n, w = y.size, int(window)
    assert w % 2 == 1
    if w == 1 or n < w:
        return y.copy()
    h = (w - 1) // 2
    s = np.empty(n, dtype=np.float64)
    for t in range(h, n - h):
        s[t] = y[t - h:t + h + 1].sum() / w
    j = np.arange(w, dtype=np.float64) - h
    for base, frames in ((0, range(0, h)), (n - w, range(n - h, n))):
        seg = y[base:base + w]
        slope = (j * seg).sum() / (j * j).sum()
        for t in frames:
            s[t] = seg.sum() / w + (t - base - h) * slope
    return s


def smooth_f0(lf0, vuv, window, threshold=0.5):
    """One item: lf0, vuv (n, D) float32 -> f0 (n, D) float64 before the final rounding: smooth(exp(lf0)) gated by vuv > threshold."""
    lf0 = np.asarray(lf0, dtype=np.float32)
    out = np.zeros(lf0.shape, dtype=np.float64)
    for d in range(lf0.shape[1]):
        s = smooth(np.exp(lf0[:, d].astype(np.float64)), window)
        out[:, d] = np.where(np.asarray(vuv)[:, d] > np.float32(threshold), s, 0.0)
    return out
