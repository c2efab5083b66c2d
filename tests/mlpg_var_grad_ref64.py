"""Float64 reference of the gradients of MLPG with respect to its means AND its per-frame variances (csrc/mlpg.hip,
mg_mlpg_grad_mv_f32), with dense matrices, the cases the GPU tests run and the bounds they are held to.

One system (utterance b, dimension d) of length len with padding p has n = len + 2p unknowns; padded row s reads frame
f(s) = clamp(s - p, 0, len - 1).  As the kernel forms them, tau_w[s] = float32(1 / var) and (mu tau)_w[s] = float32(mu / var) at that
frame, both widened; everything after that is float64:
    P = sum_w W_w^T diag(tau_w) W_w,      x~ = P^-1 sum_w W_w^T (mu tau)_w  (all n rows),      P lambda = g~ (g on the output rows),
    dL/dmu [b, f, w D + d] = sum_{s: f(s) = f}  tau_w[s] (W_w lambda)[s],
    dL/dvar[b, f, w D + d] = sum_{s: f(s) = f} -tau_w[s]^2 (W_w lambda)[s] (mu_w[s] - (W_w x~)[s]).
(d x~ / d tau_w[s] = P^-1 W_w^T e_s (mu_w[s] - (W_w x~)[s]) and d tau / d var = -tau^2.)  mu in the residual is the float32 mean widened.

Bounds, elementwise:
* grad_means: those of mlpg_grad_ref64 (``bound``): 2^-23 |want| for a float32 output plus SOLVE_FLOOR = 1e-9 of max |want| over the
  element's system.
* grad_variances:  F32_ROUNDING |want|  (float32 output only: one rounding, 2^-24, doubled)  +  SOLVE_FLOOR * scale,
      scale = max over the frames f and windows w of the element's system of  sum_{s: f(s) = f} tau^2 |W_w lambda| (|mu| + |W_w x~|).
  The residual mu - W x~ CANCELS (it is the part of the mean the trajectory does not follow), so an error relative to |want| cannot
  be promised: what the solves deliver is an error relative to the sizes of the factors.  Kernel and reference solve P lambda = g~
  and P x~ = rhs in float64, by LDL^T and by LU; a backward-stable banded solve has a forward error of about c cond(P) 2^-53 relative
  to the largest entry of its solution, c a small multiple of the bandwidth (Higham, Accuracy and Stability of Numerical Algorithms,
  thm. 9.4 / 10.4; c ~ 3 (HB + 1) <= 15 here), and a window pass adds at most 5 products per row.  Each factor of the product
  (W lambda) (mu - W x~) thus carries one solve and one window pass, under 32 cond(P) 2^-52 of its size - the argument
  mlpg_grad_ref64 makes for two solves in a row, here for two side by side - the product twice that, and the sum over a frame's rows
  (increasing s in the kernel, pairwise in numpy) adds (padding + 1) 2^-53 of the sum of the absolute terms, which is far below it.
  The host test holds every GPU case to 64 cond(P) 2^-52 < 1e-9, which makes 1e-9 of ``scale`` an honest floor.
"""
import functools

import numpy as np

from mlpg_grad_ref64 import (CASES, COND_FACTOR, DEFAULT_WINDOWS, F32_ROUNDING, SOLVE_FLOOR, WINDOWS, WINDOWS_5PT, bound as bound_means,
                             system_scale, window_matrix)

__all__ = ['CASES', 'COND_FACTOR', 'DEFAULT_WINDOWS', 'F32_ROUNDING', 'SOLVE_FLOOR', 'WINDOWS', 'WINDOWS_5PT', 'bound_means',
           'system_scale', 'window_matrix']

# one more case with the spread of variances an exp(2 s) output produces: log standard deviations uniform in WIDE_LOG_STD, variances
# within [exp(-5), exp(1)] = [0.0067, 2.7], a ratio of 400 where the standard deviations of [0.2, 0.6] give 9: three nats of log
# standard deviation, about what a trained stream spans between a steady vowel and a transition.  (B, T, D, padding, windows, seq_len).
# On the CPU cond(P) <= 635 at this range (test_gpu_cases_are_well_conditioned prints it), against the 7e4 the floor allows.
WIDE_LOG_STD = (-2.5, 0.5)
VAR_CASES = dict(CASES, wide_spread=(4, 37, 3, 5, 'default', (37, 22, 1, 6)))


def system_grads(windows, length, padding, tau, mu_tau, mu, grad):
    """One system.  tau, mu_tau, mu: (W, length) float64 per frame (tau and mu_tau as the kernel forms them), grad (length,).
    Returns (dL/dmu (W, length), dL/dvar (W, length), scale terms (W, length), x~ on the output rows (length,), cond(P))."""
    n = length + 2 * padding
    frames = np.clip(np.arange(n) - padding, 0, length - 1)
    mats = [window_matrix(w, n) for w in windows]
    p_mat = sum(m.T @ (tau[w][frames][:, None] * m) for w, m in enumerate(mats))
    rhs = sum(m.T @ mu_tau[w][frames] for w, m in enumerate(mats))
    g_pad = np.zeros(n, np.float64)
    g_pad[padding:padding + length] = grad
    x = np.linalg.solve(p_mat, rhs)
    lam = np.linalg.solve(p_mat, g_pad)
    g_mu, g_var, terms = (np.zeros((len(windows), length), np.float64) for _ in range(3))
    for w, m in enumerate(mats):
        t_w, mu_w, w_lam, w_x = tau[w][frames], mu[w][frames], m @ lam, m @ x
        np.add.at(g_mu[w], frames, t_w * w_lam)
        np.add.at(g_var[w], frames, -t_w ** 2 * w_lam * (mu_w - w_x))
        np.add.at(terms[w], frames, t_w ** 2 * np.abs(w_lam) * (np.abs(mu_w) + np.abs(w_x)))
    return g_mu, g_var, terms, x[padding:padding + length], np.linalg.cond(p_mat)


def kernel_inputs(means, variances):
    """float32 means and variances -> (tau, mu tau, mu) float64 as mg_mlpg_f32 / mg_mlpg_grad_mv_f32 form them."""
    means, variances = np.asarray(means, np.float32), np.asarray(variances, np.float32)
    return ((np.float32(1.0) / variances).astype(np.float64), (means / variances).astype(np.float32).astype(np.float64),
            means.astype(np.float64))


def grads_ref(grad_out, means, variances, windows, padding, seq_len=None):
    """grad_out (B, T, D), means and variances (B, T, W D) float32 -> dict of float64 arrays: ``grad_means``, ``grad_variances`` and
    ``scale`` (the floor's scale, broadcast over each system) (B, T, W D), ``trajectory`` (B, T, D), ``cond`` (B, D) (0 for an
    empty item)."""
    grad_out = np.asarray(grad_out, np.float64)
    tau, mu_tau, mu = kernel_inputs(means, variances)
    bsz, t, dim = grad_out.shape
    n_win = len(windows)
    width = n_win * dim
    assert tau.shape == (bsz, t, width), (tau.shape, (bsz, t, width))
    seq_len = [t] * bsz if seq_len is None else [min(max(int(v), 0), t) for v in seq_len]
    out = {k: np.zeros((bsz, t, width), np.float64) for k in ('grad_means', 'grad_variances', 'scale')}
    out['trajectory'], out['cond'] = np.zeros((bsz, t, dim), np.float64), np.zeros((bsz, dim), np.float64)
    for b in range(bsz):
        length = seq_len[b]
        if length <= 0:
            continue
        for d in range(dim):
            cols = np.arange(n_win) * dim + d
            g_mu, g_var, terms, x, cond = system_grads(windows, length, padding, tau[b, :length, cols], mu_tau[b, :length, cols],
                                                       mu[b, :length, cols], grad_out[b, :length, d])
            out['grad_means'][b, :length, cols] = g_mu
            out['grad_variances'][b, :length, cols] = g_var
            out['scale'][b, :, cols] = terms.max()
            out['trajectory'][b, :length, d] = x
            out['cond'][b, d] = cond
    return out


def bound_variances(want, scale, f32):
    floor = SOLVE_FLOOR * scale
    return F32_ROUNDING * np.abs(want) + floor if f32 else floor


def make_inputs(rng, name):
    """(grad_out, means, variances) float32 of a case: standard-normal gradients and means, per-frame variances from standard
    deviations in [0.2, 0.6] (as synthetic.acoustic_normalisers draws them) or, for 'wide_spread', exp(2 s), s uniform in WIDE_LOG_STD."""
    bsz, t, dim, _, windows, _ = VAR_CASES[name]
    width = len(WINDOWS[windows]) * dim
    grad_out = rng.standard_normal((bsz, t, dim)).astype(np.float32)
    means = rng.standard_normal((bsz, t, width)).astype(np.float32)
    if name == 'wide_spread':
        variances = np.exp(np.float32(2.0) * rng.uniform(*WIDE_LOG_STD, size=(bsz, t, width)).astype(np.float32)).astype(np.float32)
    else:
        variances = (rng.uniform(0.2, 0.6, (bsz, t, width)).astype(np.float32) ** 2).astype(np.float32)
    return grad_out, means, variances


@functools.lru_cache(maxsize=None)
def case(name, masked=True):
    """(grad_out, means, variances (float32), windows, padding, seq_len, reference dict) of one GPU case; computed once, read-only.
    ``masked=False``: the same inputs without seq_len (every utterance is T frames long)."""
    bsz, t, dim, padding, windows, seq_len = VAR_CASES[name]
    seq_len = seq_len if masked else None
    rng = np.random.RandomState(2000 + 17 * sorted(VAR_CASES).index(name))
    windows = WINDOWS[windows]
    grad_out, means, variances = make_inputs(rng, name)
    want = grads_ref(grad_out, means, variances, windows, padding, seq_len)
    for array in (grad_out, means, variances) + tuple(want.values()):
        array.setflags(write=False)
    return grad_out, means, variances, windows, padding, None if seq_len is None else np.array(seq_len, np.int64), want
