"""Float64 reference of parameter generation under a global-variance prior (csrc/mlpg_gv.hip, mg_mlpg_gv_f32; Toda & Tokuda 2007),
with dense matrices, the cases the GPU tests run and the bounds they are held to.

One system (utterance b, static dimension d) of length len with padding p has N = len + 2p unknowns; P and rhs are MLPG's, with
1 / var and mean / var formed in float32 as the kernel forms them and widened.  O = [p, N - p) are the output rows, e their indicator,
n = len, W the number of windows, omega = 1 / (W n), v(x) the biased variance of x over O.  Minimised is
    F(x) = omega (1/2 x^T P x - x^T rhs) + (w / 2) (v(x) - mu_v)^2 / sigma_v^2.
A stationary point solves A(kappa) x = rhs with
    A(kappa) = P + gamma (E - e e^T / n),    gamma = 2 kappa / (n omega) = 2 W kappa,    kappa = w (v(x) - mu_v) / sigma_v^2,
and where A is positive definite v(x(kappa)) does not increase with kappa, so h(kappa) = w (v(x(kappa)) - mu_v) / sigma_v^2 - kappa
falls strictly (h' <= -1) and has one root.  Here: bisection of the bracket the kernel starts from down to 2^-50 of its larger end,
every evaluation a dense np.linalg.solve(A, rhs), feasibility by eigvalsh(A) > 0.

Bounds of the GPU tests (the issue's): the float64 output within X_FLOOR = 1e-9 of max |x_ref| of its system (a missing centring term,
a wrong sign of the rank-one coefficient or omega off by W each leave >= 1e-3; the reference's own residual is <= 1e-11), the float32
output within one rounding 2^-24 |x_ref| on top of it, the gradient of F at the output within 1e-9 of the gradient at MLPG's
solution, kappa within 2^-36 relative.
"""
import functools

import numpy as np

from mlpg_grad_ref64 import DEFAULT_WINDOWS, WINDOWS_5PT, make_variances, window_matrix

WINDOWS_STATIC_DELTA = DEFAULT_WINDOWS[:2]
WINDOWS = {'default': DEFAULT_WINDOWS, 'static_delta': WINDOWS_STATIC_DELTA, '5pt': WINDOWS_5PT}
VAR_LAYOUTS = ('global', 'frame', 'item')
GV_LAYOUTS = ('shared', 'item')             # gv_mean / gv_variance (D,) or (B, D)
FACTORS = (2.0, 0.5)                        # mu_v as a multiple of v(x0); sigma_v = 0.1 mu_v

X_FLOOR = 1e-9
F32_ROUNDING = 2.0 ** -24
GRAD_RATIO = 1e-9
KAPPA_REL = 2.0 ** -36
H_RULE = 1e-6                               # a search that ends with |h| > H_RULE (1 + |kappa|) falls back to MLPG's solution

# the shape of the issue: the fifth item has one frame (n < 2), the sixth all-zero means (v = 0 whatever kappa: the degenerate fallback)
BSZ, T, DIM, PADDING = 6, 24, 3, 3
SEQ_LEN = (24, 11, 5, 2, 1, 24)
DEGENERATE = 5


def variance_over(x, padding, length):
    rows = np.asarray(x, np.float64)[padding:padding + length]
    return float(np.mean((rows - rows.mean()) ** 2))


def build_system(means, variances, windows, padding, length, b, d):
    """(P, rhs) of system (b, d): float32 1 / var and mean / var, float64 after that."""
    means, variances = np.asarray(means, np.float32), np.asarray(variances, np.float32)
    n_win = len(windows)
    dim = means.shape[2] // n_win
    n_rows = length + 2 * padding
    frames = np.clip(np.arange(n_rows) - padding, 0, length - 1)
    p_mat, rhs = np.zeros((n_rows, n_rows)), np.zeros(n_rows)
    for w, window in enumerate(windows):
        column = w * dim + d
        if variances.ndim == 1:
            var = np.full(n_rows, variances[column], np.float32)
        elif variances.ndim == 2:
            var = np.full(n_rows, variances[b, column], np.float32)
        else:
            var = variances[b, frames, column]
        mu = means[b, frames, column]
        tau = (np.float32(1.0) / var).astype(np.float64)
        mu_tau = (mu / var).astype(np.float32).astype(np.float64)
        mat = window_matrix(window, n_rows)
        p_mat += mat.T @ (tau[:, None] * mat)
        rhs += mat.T @ mu_tau
    return p_mat, rhs


class System:
    """One system under the prior (mu_v, sigma_v^2, weight w)."""

    def __init__(self, p_mat, rhs, padding, length, n_win, mu_v, sigma2_v, weight=1.0):
        self.p_mat, self.rhs, self.padding, self.length, self.n_win = p_mat, rhs, padding, length, n_win
        self.mu_v, self.sigma2_v, self.weight = float(mu_v), float(sigma2_v), float(weight)
        self.omega = 1.0 / (n_win * length)
        self.e = np.zeros(len(rhs))
        self.e[padding:padding + length] = 1.0
        self.centre = np.diag(self.e) - np.outer(self.e, self.e) / length
        self.x0 = np.linalg.solve(p_mat, rhs)

    def variance(self, x):
        return variance_over(x, self.padding, self.length)

    def kappa_of(self, x):
        return self.weight * (self.variance(x) - self.mu_v) / self.sigma2_v

    def objective(self, x):
        return (self.omega * (0.5 * x @ self.p_mat @ x - x @ self.rhs)
                + 0.5 * self.weight * (self.variance(x) - self.mu_v) ** 2 / self.sigma2_v)

    def gradient(self, x):
        return self.omega * (self.p_mat @ x - self.rhs) + self.kappa_of(x) * (2.0 / self.length) * (self.centre @ x)

    def matrix(self, kappa):
        return self.p_mat + (2.0 * kappa / (self.length * self.omega)) * self.centre

    def evaluate(self, kappa):
        """(x(kappa), h(kappa)), or (None, None) where A(kappa) is not positive definite."""
        a_mat = self.matrix(kappa)
        if not (np.linalg.eigvalsh(a_mat) > 0).all():
            return None, None
        x = np.linalg.solve(a_mat, self.rhs)
        return x, self.kappa_of(x) - kappa

    def bracket(self):
        v0 = self.variance(self.x0)
        if v0 >= self.mu_v:
            return 0.0, self.weight * (v0 - self.mu_v) / self.sigma2_v
        diag = np.diag(self.p_mat)[self.padding:self.padding + self.length].min()
        return -self.omega * self.length * diag / (2.0 * (1.0 - 1.0 / self.length)), 0.0

    def solve(self, rel_width=2.0 ** -50, max_iter=400):
        """(x, kappa, |h|, evaluations, flag): the root of h by bisection, or MLPG's solution and flag 1."""
        if self.length < 2 or self.weight == 0 or not self.sigma2_v > 0:
            return self.x0, 0.0, 0.0, 0, 1
        lo, hi = self.bracket()
        best, used = None, 0
        for kappa in (lo, hi):
            x, h = self.evaluate(kappa)
            used += 1
            if x is not None and (best is None or abs(h) < abs(best[2])):
                best = (x, kappa, h)
        while used < max_iter and hi - lo > rel_width * max(abs(lo), abs(hi)):
            kappa = 0.5 * (lo + hi)
            x, h = self.evaluate(kappa)
            used += 1
            if x is None or h > 0:
                lo = kappa
            else:
                hi = kappa
            if x is not None and (best is None or abs(h) < abs(best[2])):
                best = (x, kappa, h)
        if best is None or not abs(best[2]) <= H_RULE * (1.0 + abs(best[1])):
            return self.x0, 0.0 if best is None else best[1], 0.0 if best is None else abs(best[2]), used, 1
        return best[0], best[1], abs(best[2]), used, 0

    def complete(self, x_out):
        """All N rows from the output rows: the padding rows minimise F given the output rows (the prior does not see them)."""
        out = self.e > 0
        x = np.zeros(len(self.rhs))
        x[out] = x_out
        if (~out).any():
            x[~out] = np.linalg.solve(self.p_mat[np.ix_(~out, ~out)], self.rhs[~out] - self.p_mat[np.ix_(~out, out)] @ x_out)
        return x

    def descend(self, steps=500):
        """Steepest descent with a diagonal-Hessian preconditioner and 1.2 / 0.5 step adaptation from the variance-scaled start (the
        generation loop of HTS): what the exact root has to be at least as good as."""
        out = self.e > 0
        x = self.x0.copy()
        v0 = self.variance(x)
        if v0 > 0:
            mean = x[out].mean()
            x[out] = np.sqrt(self.mu_v / v0) * (x[out] - mean) + mean
        step, value = 1.0, self.objective(x)
        for _ in range(steps):
            centred = (x - x[out].mean()) * self.e
            hess = self.omega * np.diag(self.p_mat) + (2.0 * self.weight / (self.length * self.sigma2_v)) * (
                abs(self.variance(x) - self.mu_v) * (1.0 - 1.0 / self.length) * self.e + 2.0 * centred ** 2 / self.length)
            trial = x - step * self.gradient(x) / hess
            trial_value = self.objective(trial)
            if trial_value < value:
                x, value, step = trial, trial_value, step * 1.2
            else:
                step *= 0.5
        return x, value


def mlpg_gv_ref(means, variances, gv_mean, gv_variance, windows, padding, seq_len=None, gv_weight=1.0):
    """-> (trajectory (B, T, D) float64, zero past seq_len; info (B, D, 4) = (kappa, |h|, evaluations, flag); systems {(b, d): System})."""
    means = np.asarray(means, np.float32)
    bsz, t, width = means.shape
    n_win = len(windows)
    dim = width // n_win
    gv_mean = np.broadcast_to(np.asarray(gv_mean, np.float32), (bsz, dim)).astype(np.float64)
    gv_variance = np.broadcast_to(np.asarray(gv_variance, np.float32), (bsz, dim)).astype(np.float64)
    seq_len = [t] * bsz if seq_len is None else [min(max(int(v), 0), t) for v in seq_len]
    out, info, systems = np.zeros((bsz, t, dim)), np.zeros((bsz, dim, 4)), {}
    info[:, :, 3] = 1.0
    for b in range(bsz):
        length = seq_len[b]
        if length <= 0:
            continue
        for d in range(dim):
            p_mat, rhs = build_system(means, variances, windows, padding, length, b, d)
            system = System(p_mat, rhs, padding, length, n_win, gv_mean[b, d], gv_variance[b, d], gv_weight)
            x, kappa, h_abs, used, flag = system.solve()
            out[b, :length, d] = x[padding:padding + length]
            info[b, d] = kappa, h_abs, used, flag
            systems[b, d] = system
    return out, info, systems


def make_inputs(windows, layout, seed=0):
    """(means f32 (B, T, W D), variances f32) of the issue's shape; the sixth item all zero."""
    rng = np.random.RandomState(4200 + seed)
    width = len(WINDOWS[windows]) * DIM
    means = rng.standard_normal((BSZ, T, width)).astype(np.float32)
    means[DEGENERATE] = 0.0
    return means, make_variances(rng, layout, BSZ, T, width)


def plain_variances(means, variances, windows, padding, seq_len):
    """v(x0) (B, D) of MLPG's own solution; 0 for an empty item."""
    bsz, _, width = means.shape
    dim = width // len(windows)
    v0 = np.zeros((bsz, dim))
    for b in range(bsz):
        if seq_len[b] > 0:
            for d in range(dim):
                p_mat, rhs = build_system(means, variances, windows, padding, seq_len[b], b, d)
                v0[b, d] = variance_over(np.linalg.solve(p_mat, rhs), padding, seq_len[b])
    return v0


def make_prior(v0, gv_layout, factor):
    """gv_mean, gv_variance f32: mu_v = factor x v(x0) - of the system itself (B, D), the items without a variance of their own taking
    the shared value - or of the mean over the first four items (D,); sigma_v = 0.1 mu_v."""
    shared = factor * v0[:4].mean(axis=0)
    if gv_layout == 'shared':
        mu = shared
    else:
        mu = np.where(v0 > 1e-20, factor * v0, shared[None, :])
    mu = mu.astype(np.float32)
    return mu, ((np.float32(0.1) * mu) ** 2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(windows='default', layout='global', gv_layout='shared', factor=2.0):
    """(means, variances, gv_mean, gv_variance, windows, padding, seq_len, want (B, T, D) f64, info (B, D, 4), systems) of one GPU case;
    computed once, read-only."""
    means, variances = make_inputs(windows, layout)
    wins = WINDOWS[windows]
    v0 = plain_variances(means, variances, wins, PADDING, SEQ_LEN)
    gv_mean, gv_variance = make_prior(v0, gv_layout, factor)
    want, info, systems = mlpg_gv_ref(means, variances, gv_mean, gv_variance, wins, PADDING, SEQ_LEN)
    for array in (means, variances, gv_mean, gv_variance, want, info):
        array.setflags(write=False)
    return means, variances, gv_mean, gv_variance, wins, PADDING, np.array(SEQ_LEN, np.int64), want, info, systems


# every variance layout and both prior layouts under the default windows, the other two window sets under global variances
CASE_KEYS = ([('default', layout, gv_layout, factor) for layout in VAR_LAYOUTS for gv_layout in GV_LAYOUTS for factor in FACTORS]
             + [(windows, 'global', gv_layout, factor) for windows in ('static_delta', '5pt') for gv_layout in GV_LAYOUTS
                for factor in FACTORS])
