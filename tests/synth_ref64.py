"""NumPy float64 restatement of the waveform synthesis of csrc/synth.hip (include/morgana_hip.h, K34), a python-integer pulse
reference, and the error bound the device waveform is held to.  Nothing here imports the package.

Definition, per utterance of n frames (f0 (n,), 0 where unvoiced; sp, ap (n, K), K = F / 2 + 1), sample rate fs, frame period in ms:

1. S = fs * frame_period / 1000 samples per frame; N = floor((n - 1) S) + 1 samples (0 for n = 0).
2. Sample i: u = i / S, j = min(floor(u), n - 1), j1 = min(j + 1, n - 1), w = u - j; v_j = f0_j > 0, g_j = f0_j if v_j else 500;
   v(i) = v_j (w < .5), v_j1 (w > .5), v_j and v_j1 (w == .5); f(i) = min(max(g_j + (g_j1 - g_j) w, fs / F), fs / 2) where v(i), else 500.
3. inc(i) = rint(f(i) 2^32 / fs) as an integer, Phi(i) = sum_{j <= i} inc(j); a pulse at i iff (Phi(i) >> 32) > (Phi(i - 1) >> 32);
   delta = (Phi(i) mod 2^32) / inc(i); T_m = i_{m+1} - i_m, N - i_m for the last pulse.  n < 2: no pulse, the N samples are zero.
4. Pulse m: u = min(max((i_m - delta_m) / S, 0), n - 1), j, j1, w as in 2; s = max(sp_j + (sp_j1 - sp_j) w, 0), a likewise from ap,
   r = clip(a^2, 0, 1) - NaNs are kept.
5. minphase(P): L = .5 ln P, c = irfft(L, F), folded (c[0], 2 c[q] for 0 < q < F / 2, c[F / 2], 0 above), H = exp(rfft(folded)).
6. Voiced pulses: h = irfft(minphase(s (1 - r) + 1e-12) exp(2 pi i k delta / F)); x[p] = h[(p - F / 2 + 1) mod F]; x -= d sum(x) with
   d[p] = .5 - .5 cos(2 pi (p + 1) / (F + 1)) normalised to sum 1; x *= sqrt(T_m).
7. Every pulse: e = z[i_m : i_m + T_m] zero-padded to F (z: the utterance's N(0, 1) track); G = minphase(s r + 1e-12) where voiced,
   minphase(s + 1e-12 + 0 r) where not (0 r changes no bit and lets a NaN aperiodicity through); irfft(rfft(e) G), placed as x.
   The noise segment's mean is not removed (WORLD's newer versions do).
8. y[i_m + t] += x_m[t + F / 2 - 1] for t in [-F / 2 + 1, F / 2] inside [0, N), in ascending m.

The bound (``synthesise(..., want_bound=True)``).  u = 2^-53.  A radix-2 transform of size F has relative l2 error
log2(F) (mu + gamma_4 (sqrt 2 + mu)) (Higham, Accuracy and Stability, theorem 24.2): a butterfly is one complex multiplication by a
twiddle of error mu <= u (four products, two sums: gamma_4 sqrt 2 with the addition behind it) - 6.66 u per stage; the kernel runs two
real sequences through one complex transform and takes them apart with one more addition (u more, against the norm of the PAIR):
eF = C_FFT log2(F) u with C_FFT = 8.  Carried through one pulse, with |.| the l2 norm over the full length F:
  cepstra     L has 2 u |L| (the logarithm); c = ifft: |dc| <= (2 u + eF) |L| / sqrt F; folding doubles it; C = fft(folded):
              |dC| <= sqrt F (2 |dc| + 2 eF |c|) = (4 u + 4 eF) |L|, and every bin's error is at most that l2 norm  (L: the pair)
  spectra     exp turns the absolute error of C into a relative one: dH = dC + 8 u per bin of H (exp, sincos, the delta phase and
              its product), dG = dC + 6 u per bin of G; E = rfft(e): |dE| <= eF sqrt F |e|
  responses   (h, noise) = ifft(H, E G): dOut = dH |h| + max|G| eF |e| + (dG + 2 u) |noise| + eF sqrt(|h|^2 + |noise|^2), every
              sample's error at most that
  placing     the sum over F terms in any order: F u sum|h| <= F^1.5 u |h|, times d[p] <= 2 / (F + 1); the scale and the sums:
              b_m = (sqrt T (1 + 2 / sqrt F) + 1) dOut + 2 u sqrt(T F) |h| + 8 u max|x_m|
A sample's bound is the sum of b_m over the pulses that cover it plus 2 u sum_m |x_m| for the overlap-add, and all of it TWICE: the
device and numpy's own transform are each that far from the exact value.  First order in u throughout.
"""
import math

import numpy as np

C_FFT = 8.
U = 2. ** -53


def samples_per_frame(fs, frame_period):
    return float(fs) * float(frame_period) / 1000.


def n_samples(n, s):
    return 0 if n <= 0 else int(math.floor((n - 1) * s)) + 1


def _frame_pair(u, n):
    j = np.minimum(np.floor(u).astype(np.int64), n - 1)
    return j, np.minimum(j + 1, n - 1), u - j


def sample_f0(f0, fs, frame_period, fft_size):
    """(f (N,), voiced (N,)) of step 2."""
    f0 = np.asarray(f0, np.float64)
    n, s = len(f0), samples_per_frame(fs, frame_period)
    j, j1, w = _frame_pair(np.arange(n_samples(n, s), dtype=np.float64) / s, n)
    v = f0 > 0
    g = np.where(v, f0, 500.)
    voiced = np.where(w < .5, v[j], np.where(w > .5, v[j1], v[j] & v[j1]))
    with np.errstate(invalid='ignore'):
        x = g[j] + (g[j1] - g[j]) * w
        x = np.where(x >= float(fs) / fft_size, x, float(fs) / fft_size)
        x = np.where(x > .5 * float(fs), .5 * float(fs), x)
    return np.where(voiced, x, 500.), voiced


def pulses(f0, fs, frame_period, fft_size):
    """Step 3 in Python integers -> (index int64 (M,), delta float64 (M,), T int64 (M,), voiced bool (M,))."""
    n = len(f0)
    empty = (np.zeros(0, np.int64), np.zeros(0, np.float64), np.zeros(0, np.int64), np.zeros(0, bool))
    if n < 2:
        return empty
    f, voiced = sample_f0(f0, fs, frame_period, fft_size)
    inc = [int(v) for v in np.rint(f * (4294967296. / float(fs)))]
    phi, index, delta = 0, [], []
    for i, step in enumerate(inc):
        before = phi
        phi += step
        if (phi >> 32) > (before >> 32):
            index.append(i)
            delta.append(float(phi & 0xFFFFFFFF) / float(step))
    if not index:
        return empty
    index = np.array(index, np.int64)
    return index, np.array(delta, np.float64), np.diff(np.append(index, len(f))), voiced[index]


def minphase(p, fft_size):
    """Step 5 -> (H (K,) complex, l2 norm of the Hermitian-extended L)."""
    half = fft_size // 2
    log_half = .5 * np.log(p)
    c = np.fft.irfft(log_half, fft_size)
    folded = np.zeros(fft_size)
    folded[0], folded[1:half], folded[half] = c[0], 2. * c[1:half], c[half]
    full = np.sqrt(np.sum(log_half ** 2) + np.sum(log_half[1:half] ** 2))
    return np.exp(np.fft.rfft(folded)), full


def dc_window(fft_size):
    d = .5 - .5 * np.cos(2. * np.pi * (np.arange(fft_size, dtype=np.float64) + 1.) / (fft_size + 1.))
    return d / d.sum()


def synthesise(f0, sp, ap, fs, frame_period, noise, want_bound=False, want_pulses=False):
    """One utterance -> y (N,) float64 [, bound (N,)] [, the pulse arrays]."""
    f0, sp, ap = np.asarray(f0, np.float64), np.asarray(sp, np.float64), np.asarray(ap, np.float64)
    n, bins = len(f0), sp.shape[1]
    fft_size, half = 2 * (bins - 1), bins - 1
    s_per = samples_per_frame(fs, frame_period)
    total = n_samples(n, s_per)
    y, bound = np.zeros(total), np.zeros(total)
    index, delta, period, voiced = pulses(f0, fs, frame_period, fft_size)
    d = dc_window(fft_size)
    e_f = C_FFT * math.log2(fft_size) * U
    order = (np.arange(fft_size) - half + 1) % fft_size
    k = np.arange(bins, dtype=np.float64)
    noise = np.asarray(noise, np.float64)
    for m in range(len(index)):
        i_m, t_m = int(index[m]), int(period[m])
        u = min(max((float(i_m) - delta[m]) / s_per, 0.), float(n - 1))
        j = min(int(math.floor(u)), n - 1)
        j1 = min(j + 1, n - 1)
        w = u - j
        with np.errstate(invalid='ignore', divide='ignore'):
            s = sp[j] + (sp[j1] - sp[j]) * w
            s = np.where(s < 0., 0., s)
            a = ap[j] + (ap[j1] - ap[j]) * w
            r = a * a
            r = np.where(r < 0., 0., r)
            r = np.where(r > 1., 1., r)
            e = np.zeros(fft_size)
            e[:t_m] = noise[i_m:i_m + t_m]
            if voiced[m]:
                h_spec, l_p = minphase(s * (1. - r) + 1e-12, fft_size)
                g_spec, l_a = minphase(s * r + 1e-12, fft_size)
                h = np.fft.irfft(h_spec * np.exp(1j * (2. * np.pi * delta[m] / fft_size) * k), fft_size)
            else:
                g_spec, l_a = minphase(s + 1e-12 + 0. * r, fft_size)
                l_p, h = 0., np.zeros(fft_size)
            shaped = np.fft.irfft(np.fft.rfft(e) * g_spec, fft_size)
            x = h[order]
            if voiced[m]:
                x = (x - d * x.sum()) * math.sqrt(t_m)
            x = x + shaped[order]
        lo, hi = i_m - half + 1, i_m + half + 1                  # the samples of x[0], x[F - 1] + 1
        a0, a1 = max(lo, 0), min(hi, total)
        y[a0:a1] += x[a0 - lo:a1 - lo]
        if want_bound:
            with np.errstate(invalid='ignore'):
                l_pair = math.hypot(l_p, l_a)
                d_c = (4. * U + 4. * e_f) * l_pair
                d_h, d_g = d_c + 8. * U, d_c + 6. * U
                n_h, n_s, n_e = np.linalg.norm(h), np.linalg.norm(shaped), np.linalg.norm(e)
                d_out = d_h * n_h + np.abs(g_spec).max() * e_f * n_e + (d_g + 2. * U) * n_s + e_f * math.hypot(n_h, n_s)
                b_m = ((math.sqrt(t_m) * (1. + 2. / math.sqrt(fft_size)) + 1.) * d_out + 2. * U * math.sqrt(t_m * fft_size) * n_h
                       + 8. * U * np.abs(x).max())
                bound[a0:a1] += b_m + 2. * U * np.abs(x[a0 - lo:a1 - lo])
    out = (y,)
    if want_bound:
        out += (2. * bound,)
    if want_pulses:
        out += ((index, delta, period, voiced),)
    return out[0] if len(out) == 1 else out
