"""Float64 reference of the gradient of MLPG with respect to its means (csrc/mlpg.hip, mg_mlpg_grad_f32), with dense matrices, the
cases the GPU tests run and the bounds they are held to.

One system (utterance b, dimension d) of length len with padding p has n = len + 2p unknowns; padded row s reads frame
f(s) = clamp(s - p, 0, len - 1); tau_w[s] = float32(1 / var) at that frame, widened (as the kernel forms it);
    P = sum_w W_w^T diag(tau_w) W_w,      x = P^-1 sum_w W_w^T (tau_w o mu_w),      output = rows [p, n - p) of x.
x is linear in mu, so for an upstream gradient g on the output rows
    P lambda = g~ (g on the output rows, 0 on the padding rows),   v_w = tau_w o (W_w lambda),   dL/dmu[b, f, w D + d] = sum_{s: f(s) = f} v_w[s].

Bounds (elementwise, `scale` = max |want| over the system the element belongs to):
* SOLVE_FLOOR = 1e-9 * scale.  Kernel and reference both solve P lambda = g~ in float64, by LDL^T and by LU.  A backward-stable
  banded solve has a forward error of about c * cond(P) * 2^-53 relative to max |lambda| with c a small multiple of the bandwidth
  (Higham, Accuracy and Stability of Numerical Algorithms, thm. 10.4 / 9.4: c ~ 3 (HB + 1) <= 15 here); two such solves and the
  window pass (at most 15 products per row, coefficients <= 2) stay under 64 * cond(P) * 2^-52, taken against max |want|.  The host test holds
  every GPU case to 64 * cond(P) * 2^-52 < 1e-9, which makes 1e-9 an honest floor.
* float32 output: one rounding of the float64 value, |want| * 2^-24, doubled for margin (2^-23), plus the floor.
"""
import functools

import numpy as np

DEFAULT_WINDOWS = ((0, 0, (1.0,)), (1, 1, (-0.5, 0.0, 0.5)), (1, 1, (1.0, -2.0, 1.0)))
WINDOWS_5PT = ((0, 0, (1.0,)), (2, 2, (-0.2, -0.1, 0.0, 0.1, 0.2)), (2, 2, (2 / 7., -1 / 7., -2 / 7., -1 / 7., 2 / 7.)))
WINDOWS = {'default': DEFAULT_WINDOWS, '5pt': WINDOWS_5PT}

SOLVE_FLOOR = 1e-9
COND_FACTOR = 64 * 2.0 ** -52
F32_ROUNDING = 2.0 ** -23

VAR_LAYOUTS = ('global', 'frame', 'item')

# (B, T, D, padding, windows, seq_len): the table of the issue
CASES = {
    'no_padding': (3, 26, 2, 0, 'default', (26, 17, 5)),
    'crosses_a_workgroup': (5, 60, 15, 100, 'default', (60, 41, 2, 33, 59)),
    'five_point': (4, 33, 5, 4, '5pt', (33, 20, 3, 9)),
    'ragged_to_nothing': (3, 9, 1, 3, 'default', (9, 1, 0)),
}


def window_matrix(window, n):
    """W[s, t] = c[l + t - s] for -l <= t - s <= u, cut off at the edges."""
    l, u, coeff = window
    mat = np.zeros((n, n), np.float64)
    for k in range(-l, u + 1):
        s = np.arange(max(0, -k), min(n, n - k))
        mat[s, s + k] = coeff[l + k]
    return mat


def _variance_at(variances, b, frames, column, shape):
    """float32 variances of one stream column at the given frames of utterance b, for the three layouts."""
    bsz, t, width = shape
    if variances.ndim == 1:
        return np.full(len(frames), variances[column], np.float32)
    if variances.ndim == 2:
        return np.full(len(frames), variances[b, column], np.float32)
    return variances[b, frames, column].astype(np.float32)


def grad_means_ref(grad_out, variances, windows, padding, seq_len=None):
    """grad_out (B, T, D), variances (W D,), (B, T, W D) or (B, W D) float32 -> (dL/dmeans (B, T, W D) float64, cond(P) (B, D); 0 for
    an empty item)."""
    grad_out = np.asarray(grad_out, np.float64)
    variances = np.asarray(variances, np.float32)
    bsz, t, dim = grad_out.shape
    n_win = len(windows)
    width = n_win * dim
    seq_len = [t] * bsz if seq_len is None else [min(max(int(v), 0), t) for v in seq_len]
    out = np.zeros((bsz, t, width), np.float64)
    cond = np.zeros((bsz, dim), np.float64)
    for b in range(bsz):
        length = seq_len[b]
        if length <= 0:
            continue
        n = length + 2 * padding
        frames = np.clip(np.arange(n) - padding, 0, length - 1)
        mats = [window_matrix(w, n) for w in windows]
        for d in range(dim):
            taus = [(np.float32(1.0) / _variance_at(variances, b, frames, w * dim + d, (bsz, t, width))).astype(np.float64)
                    for w in range(n_win)]
            p_mat = sum(m.T @ (tau[:, None] * m) for m, tau in zip(mats, taus))
            g_pad = np.zeros(n, np.float64)
            g_pad[padding:padding + length] = grad_out[b, :length, d]
            lam = np.linalg.solve(p_mat, g_pad)
            cond[b, d] = np.linalg.cond(p_mat)
            for w in range(n_win):
                np.add.at(out[b, :, w * dim + d], frames, taus[w] * (mats[w] @ lam))
    return out, cond


def system_scale(want, n_win):
    """max |want| over each system (b, d), broadcast back to want's shape (B, T, W D)."""
    bsz, t, width = want.shape
    dim = width // n_win
    per_system = np.abs(want).reshape(bsz, t, n_win, dim).max(axis=(1, 2))          # (B, D)
    return np.broadcast_to(per_system[:, None, None, :], (bsz, t, n_win, dim)).reshape(bsz, t, width)


def bound(want, n_win, f32):
    floor = SOLVE_FLOOR * system_scale(want, n_win)
    return F32_ROUNDING * np.abs(want) + floor if f32 else floor


def make_variances(rng, layout, bsz, t, width):
    """Standard deviations in [0.2, 0.6], as synthetic.acoustic_normalisers draws them; squared in float32."""
    shape = {'global': (width,), 'frame': (bsz, t, width), 'item': (bsz, width)}[layout]
    return (rng.uniform(0.2, 0.6, shape).astype(np.float32) ** 2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name, layout, masked=True):
    """(grad_out f32, variances f32, windows, padding, seq_len, want f64, cond) of one GPU case; computed once, read-only.
    ``masked=False``: the same inputs without seq_len (None: every utterance is T frames long)."""
    bsz, t, dim, padding, windows, seq_len = CASES[name]
    seq_len = seq_len if masked else None
    rng = np.random.RandomState(1000 + 17 * sorted(CASES).index(name) + VAR_LAYOUTS.index(layout))
    windows = WINDOWS[windows]
    grad_out = rng.standard_normal((bsz, t, dim)).astype(np.float32)
    variances = make_variances(rng, layout, bsz, t, len(windows) * dim)
    want, cond = grad_means_ref(grad_out, variances, windows, padding, seq_len)
    for array in (grad_out, variances, want, cond):
        array.setflags(write=False)
    return grad_out, variances, windows, padding, None if seq_len is None else np.array(seq_len, np.int64), want, cond
