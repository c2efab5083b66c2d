"""Float64 NumPy restatements of the two rules of K33 (include/morgana_hip.h, csrc/analysis.hip), and nothing else: the mel-cepstrum
of a half log power spectrum by the two-step route - an inverse real FFT, then SPTK's frequency transform per frame - and the coding
of a full-band aperiodicity into 3 kHz bands.  Written from the header's text, not from the kernel, the host table
(ops.mcep_analysis_table) or the Python wrappers."""
import numpy as np


def one_sided_cepstrum(l, fft_size):
    """g (n, F / 2 + 1) of l (n, F / 2 + 1): the inverse real FFT of the even extension is the two-sided cepstrum c_n; g_0 = c_0,
    g_{F/2} = c_{F/2}, g_n = 2 c_n between them - so that l_k = sum_n g_n cos(2 pi n k / F)."""
    l = np.asarray(l, dtype=np.float64)
    half = fft_size // 2
    assert l.shape[1] == half + 1
    c = np.fft.irfft(l, n=fft_size, axis=1)[:, :half + 1]
    g = 2.0 * c
    g[:, 0] = c[:, 0]
    g[:, half] = c[:, half]
    return g


def freqt(g, order, alpha):
    """SPTK's freqt on every sequence of g (n, m1 + 1) -> (n, order) coefficients: the recursion runs per frame, the frames side by
    side (one NumPy operation per step and coefficient instead of one per frame, step and coefficient)."""
    g = np.asarray(g, dtype=np.float64)
    out = np.zeros((order, g.shape[0]), dtype=np.float64)
    for i in range(g.shape[1] - 1, -1, -1):
        d = out.copy()
        out[0] = g[:, i] + alpha * d[0]
        if order > 1:
            out[1] = (1.0 - alpha * alpha) * d[0] + alpha * d[1]
        for j in range(2, order):
            out[j] = d[j - 1] + alpha * (d[j] - out[j - 1])
    return out.T.copy()


def mcep_of_half_log(l, order, alpha, fft_size):
    """c (n, order) of the half log power spectra l (n, F / 2 + 1): the two-step route, frame by frame."""
    return freqt(one_sided_cepstrum(l, fft_size), order, alpha)


def mcep(sp, order, alpha, fft_size, log_input=False):
    """The rule on a power spectrum sp (n, F / 2 + 1): l = 0.5 log(sp), or 0.5 sp itself with log_input."""
    sp = np.asarray(sp, dtype=np.float64)
    with np.errstate(all='ignore'):
        l = 0.5 * (sp if log_input else np.log(sp))
    return mcep_of_half_log(l, order, alpha, fft_size)


def decibels(ap):
    """min(max(20 log10(ap), -60), 0); a NaN (and the logarithm of a negative value) stays a NaN, 0 gives -60."""
    with np.errstate(all='ignore'):
        db = 20.0 * np.log10(np.asarray(ap, dtype=np.float64))
    return np.where(np.isnan(db), np.nan, np.minimum(np.maximum(db, -60.0), 0.0))


def band_aperiodicity(ap, sample_rate, n_bands, fft_size):
    """ap (n, F / 2 + 1) -> (n, n_bands) dB: band b at bin position 3000 (b + 1) F / fs, integer quotient k0 and remainder r,
    dB(k0) + (dB(k0 + 1) - dB(k0)) * (r / fs)."""
    assert n_bands >= 1 and 3000 * n_bands < sample_rate / 2.0
    db = decibels(ap)
    out = np.empty((db.shape[0], n_bands), dtype=np.float64)
    for b in range(n_bands):
        k0, r = divmod(3000 * (b + 1) * int(fft_size), int(sample_rate))
        w = float(r) / float(sample_rate)
        out[:, b] = db[:, k0] + (db[:, k0 + 1] - db[:, k0]) * w
    return out
