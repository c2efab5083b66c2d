"""Float64 reference of the masked mixture-density negative log likelihood behind mg_masked_mdn_f32 and of the selection behind
mg_mdn_select_f32 (include/morgana_hip.h), with a DERIVED fp32 rounding bound for the per-frame loss, the total loss, every gradient
element and the selected variance.

Plain numpy, no GPU and no torch.  What is computed (a row of W = K (1 + 2 D) columns = K logits a, K D means mu, K D log standard
deviations s, component-major; target y of D values; restated independently of the kernel's order):

    s'_kd   = max(s_kd, floor)                                        (no floor: s' = s)
    z_kd    = (y_d - mu_kd) exp(-s'_kd)
    S_k     = sum_d (0.5 z_kd^2 + s'_kd)
    q_k     = log_softmax(a)_k - S_k - D c,   c = 0.9189385332046727 = log sqrt(2 pi)
    l[b,t]  = -logsumexp_k(q_k) / D
    L       = mean_b( sum_{t < n_b} l[b,t] / n_b ),   n_b = seq_len[b] clamped to [0, T]  (T without seq_len)
    r_k     = exp(q_k - logsumexp q),   p_k = softmax(a)_k,   C = grad_scale / (D n_b B)
    g_a_k   = C (p_k - r_k),   g_mu_kd = -C r_k z_kd exp(-s'_kd),   g_s_kd = C r_k (1 - z_kd^2)   (0 where s_kd < floor)
for t < n_b, 0 for pad frames, which are not read at all.

The bound is a property of fp32 arithmetic, not of any kernel.  U = 2^-24 is the unit roundoff; every elementary operation returns
its exact result times (1 + d), |d| <= U; expf and logf are charged 2 ulp (EXP_ULPS, LOG_ULPS; 1 ulp = 2U relative; HIP's and
glibc's are documented at 1).  Products of error terms are dropped (first order) EXCEPT where an error sits in the argument of an
exponential and need not be small (see q below).  Sums: a term that passes through k additions picks up at most k U relative to
its own magnitude, so any summation order of n terms is covered by  DEPTH(n) U sum |terms|  with DEPTH(n) = n - 1 for n <= 64 (every
order, a serial loop included) and ceil(n / 8) + 8 above (a sum blocked over W >= 8 accumulators and a binary tree over them, at
most 8 levels: a CPU's vector sum, numpy's pairwise sum, a wave striding the row with a cross-lane tree; tests/ce_ref64.py).

  * z:  y - mu rounds once (U), exp(-s') has eps_e = 2 EXP_ULPS U (its argument is exact), the product (or a division by exp(s'))
    rounds once:  eps_z = 2U + eps_e  relative.
  * the term 0.5 z^2 + s':  z^2 carries 2 eps_z + U, the halving is exact, the addition rounds once:
        A_kd = 0.5 z^2 (2 eps_z + 2U) + U |s'|                                        (absolute)
    The terms have BOTH signs (s' may be negative), so the sum over d is bounded relative to the sum of magnitudes
    0.5 z^2 + |s'| - which also covers an evaluation that sums the squares and the log-stds separately:
        dS_k = sum_d A_kd + DEPTH(D) U sum_d (0.5 z^2 + |s'|)
  * log_softmax(a)_k as in tests/ce_ref64.py: d_k = a_k - max a, e_k = expf(d_k), sa = sum e,
        rho_a  = U sum_k e_k |d_k| / sa + eps_e + DEPTH(K) U                            (relative error of sa)
        dlsm_k = U max(|d_k|, |max a + log sa|) + rho_a + 2 LOG_ULPS U |log sa| + U |lsm_k|
    (the first term: d_k - log sa, or a_k - (max a + log sa)).
  * q_k = (lsm_k - S_k) - D c, in either association: D c is a rounded constant times an exact integer (2U D c), two subtractions
    whose intermediate is at most |lsm_k| + |S_k| + D c, and the result:
        dq_k = dlsm_k + dS_k + 2U D c + U (|lsm_k| + |S_k| + D c) + U |q_k|
    dq_k is absolute and NOT small when a target lies far from a mean (0.5 z^2 = 5e5 at a thousand standard deviations resolves to
    about 0.1 in fp32), and it sits in an exponent.  logsumexp is monotone in every q_k, so the exact statement is used:
        |logsumexp(q +- dq) - logsumexp(q)| <= log sum_k r_k exp(dq_k) =: P       (>= sum_k r_k dq_k, its first-order form)
  * logsumexp of the computed q:  M = max q (exact), dq'_k = q_k - M (U |dq'_k| absolute, relative in exp), sq = sum exp(dq'),
        rho_q  = U sum_k r_k |dq'_k| + eps_e + DEPTH(K) U + K ETA                       (ETA = 2^-149: a term that underflows)
        dlse   = P + rho_q + 2 LOG_ULPS U |log sq| + U |lse|
        bound_l = dlse / D + U |l|                                                      (the division by the exact D)
  * total loss: sum_t l / n_b and the mean over b, in ANY order: (T + B) U relative to sum |l| on top of the frames' own bounds, one
    more U for each of the two divisions:   bound_L = mean_b( sum_t (bound_l + (T + B + 2) U |l|) / n_b ).
  * responsibilities, r_k = exp(dq'_k) / sq or exp(q_k - lse): the rounding of this evaluation is, as for the softmax of ce_ref64,
        rnd_r_k = 2 |dq'_k| U + eps_e + rho_q + 3U + (1 + 2 LOG_ULPS) U |log sq|
    and the error of its inputs is dq_k + P in the exponent:   rel_r_k = expm1(dq_k + P + rnd_r_k);
    likewise rnd_p_k = 2 |d_k| U + eps_e + rho_a + 3U + (1 + 2 LOG_ULPS) U |log sa| for p_k.
  * the coefficient C, at most four operations on exact integers and grad_scale: eps_c = 4U.  Underflow: r_k, p_k, the gradient and
    any partial product on the way (C r_k, say, where r_k is tiny and z exp(-s') large) may fall below the normal range, where a
    result is rounded on the subnormal grid, ETA absolute, and is then multiplied by the remaining factors - in whatever
    association, by at most the product of (1 + |factor|) over them.  Then
        bound g_a  = |C| ( p rnd_p + r rel_r + (eps_c + 2U) |p - r| ) + 2 ETA (1 + |C|)
        bound g_mu = |g_mu| (eps_c + rel_r + eps_z + eps_e + 3U) + ETA (1 + |C|) (1 + |z|) (1 + exp(-s'))
        bound g_s  = |C| r ( z^2 (2 eps_z + U) + U |1 - z^2| + |1 - z^2| (eps_c + rel_r + 2U) ) + ETA (1 + |C|) (1 + |1 - z^2|)
    A floored s has gradient exactly 0.
  * selected variance exp(2 s') (2 s' is exact), or exp(s')^2:   bound_v = v (2 eps_e + 2U) + ETA.
A -inf logit is exact (p_k = r_k = 0 in every evaluation) and is left out of every weighted term."""
import numpy as np

F64 = np.float64
U = 2.0 ** -24
ETA = 2.0 ** -149
EXP_ULPS = 2.0
LOG_ULPS = 2.0
HALF_LOG_2PI = 0.9189385332046727
MAX_COMPONENTS = 64      # MG_MDN_MAX_COMPONENTS
MAX_ROW = 16384          # MG_MDN_MAX_ROW
REG_MAX = 1024           # longest K * D of the kernel's register path (csrc/mdn.hip: MDN_REG_MAX)
SMALL_D = 16             # widest D of its one-lane-per-component sum (MDN_SMALL_D)


def depth(n):
    """Additions a term of a sum of n terms passes through (see the module docstring)."""
    return n - 1 if n <= 64 else int(np.ceil(n / 8.0)) + 8


def width(k, d):
    return k * (1 + 2 * d)


def valid_frames(seq_len, b, t):
    if seq_len is None:
        return np.full(b, t, dtype=np.int64)
    return np.clip(np.asarray(seq_len, dtype=np.int64), 0, t)


def split(pred, k, d):
    """(B, T, K (1 + 2 D)) -> logits (B, T, K), means (B, T, K, D), log standard deviations (B, T, K, D)."""
    b, t, w = pred.shape
    assert w == width(k, d), (w, k, d)
    return pred[:, :, :k], pred[:, :, k:k + k * d].reshape(b, t, k, d), pred[:, :, k + k * d:].reshape(b, t, k, d)


def _logsumexp(v):
    """log sum exp over axis 2 (kept), the maximum subtracted; -inf entries add nothing."""
    top = v.max(axis=2, keepdims=True)
    return top + np.log(np.exp(v - top).sum(axis=2, keepdims=True))


def mdn(pred, target, seq_len=None, n_components=1, min_log_std=None, grad_scale=1.0):
    """Float64 values and fp32 bounds.  pred (B, T, K (1 + 2 D)), target (B, T, D).  Returns a dict: ``frame_loss`` / ``frame_bound``
    (B, T) (0 on pad frames), ``loss`` / ``loss_bound`` (scalars), ``grad`` / ``grad_bound`` (B, T, W) (0 on pad frames),
    ``component`` (B, T) (0 on pad frames), ``mean`` (B, T, D) (0 on pad frames), ``variance`` / ``variance_bound`` (B, T, D)
    (1 and 0 on pad frames), ``mask`` (B, T) bool."""
    x = np.asarray(pred, dtype=F64)
    y = np.asarray(target, dtype=F64)
    b, t, _ = x.shape
    k, d = int(n_components), y.shape[2]
    assert y.shape[:2] == (b, t)
    n = valid_frames(seq_len, b, t)
    mask = np.arange(t)[None, :] < n[:, None]
    x = np.where(mask[:, :, None], x, 0.0)                # pad frames are not read
    y = np.where(mask[:, :, None], y, 0.0)
    a, mu, s_raw = split(x, k, d)
    floored = s_raw < min_log_std if min_log_std is not None else np.zeros(s_raw.shape, dtype=bool)
    s = np.where(floored, min_log_std, s_raw) if min_log_std is not None else s_raw
    eps_e = 2 * EXP_ULPS * U
    eps_z = 2 * U + eps_e
    eps_c = 4 * U
    dc = d * HALF_LOG_2PI
    with np.errstate(all='ignore'):
        es = np.exp(-s)
        z = (y[:, :, None, :] - mu) * es
        half = 0.5 * z * z
        big_s = (half + s).sum(axis=3)
        ds_ = (half * (2 * eps_z + 2 * U) + U * np.abs(s)).sum(axis=3) + depth(d) * U * (half + np.abs(s)).sum(axis=3)
        # log_softmax of the logits
        amax = a.max(axis=2, keepdims=True)
        da = a - amax
        live = np.isfinite(da)
        ea = np.exp(da)
        sa = ea.sum(axis=2, keepdims=True)
        log_sa = np.log(sa)
        lsm = da - log_sa
        p = ea / sa
        absda = np.where(live, np.abs(da), 0.0)
        abslsm = np.where(live, np.abs(lsm), 0.0)
        rho_a = U * (ea * absda).sum(axis=2, keepdims=True) / sa + eps_e + depth(k) * U
        dlsm = U * np.maximum(absda, np.abs(amax + log_sa)) + rho_a + 2 * LOG_ULPS * U * np.abs(log_sa) + U * abslsm
        # the components' joint log densities and their logsumexp
        q = lsm - big_s - dc
        dq = np.where(live, dlsm + ds_ + 2 * U * dc + U * (abslsm + np.abs(big_s) + dc) + U * np.abs(np.where(live, q, 0.0)), 0.0)
        qmax = q.max(axis=2, keepdims=True)
        dqs = q - qmax
        eq = np.exp(dqs)
        sq = eq.sum(axis=2, keepdims=True)
        log_sq = np.log(sq)
        lse = (qmax + log_sq)[:, :, 0]
        r = eq / sq
        log_r = dqs - log_sq                                # kept next to r: exp(-1e9) is 0 in float64 too, its bound must stay 0
        prop = _logsumexp(log_r + dq)                       # P = log sum_k r_k exp(dq_k)
        absdqs = np.where(np.isfinite(dqs), np.abs(dqs), 0.0)
        rho_q = U * (r * absdqs).sum(axis=2, keepdims=True) + eps_e + depth(k) * U + k * ETA
        dlse = (prop + rho_q + 2 * LOG_ULPS * U * np.abs(log_sq))[:, :, 0] + U * np.abs(lse)
        l = np.where(mask, -lse / d, 0.0)
        frame_bound = np.where(mask, dlse / d + U * np.abs(l), 0.0)
        nf = n.astype(F64)
        loss = np.mean(l.sum(axis=1) / nf)
        loss_bound = np.mean((frame_bound + (t + b + 2) * U * np.abs(l)).sum(axis=1) / nf)
        # gradient
        coef = (grad_scale / (d * nf * b))[:, None, None]
        log_terms = (1 + 2 * LOG_ULPS) * U
        rnd_r = 2 * absdqs * U + eps_e + rho_q + 3 * U + log_terms * np.abs(log_sq)
        rnd_p = 2 * absda * U + eps_e + rho_a + 3 * U + log_terms * np.abs(log_sa)
        arg = dq + prop + rnd_r                             # r_k rel_r_k = exp(log r_k + log expm1(arg)), without overflow
        r_err = np.exp(log_r + np.where(arg > 30.0, arg, np.log(np.expm1(np.minimum(arg, 30.0)))))
        g_a = coef * (p - r)
        b_a = np.abs(coef) * (p * rnd_p + r_err + (eps_c + 2 * U) * np.abs(p - r)) + 2 * ETA * (1 + np.abs(coef))
        c4, r4, r_err4 = coef[:, :, :, None], r[:, :, :, None], r_err[:, :, :, None]
        g_mu = -c4 * r4 * z * es
        b_mu = np.abs(c4 * z * es) * (r4 * (eps_c + eps_z + eps_e + 3 * U) + r_err4) + ETA * (1 + np.abs(c4)) * (1 + np.abs(z)) * (1 + es)
        one_z2 = 1.0 - z * z
        g_s = np.where(floored, 0.0, c4 * r4 * one_z2)
        b_s = np.abs(c4) * (r4 * (z * z * (2 * eps_z + U) + U * np.abs(one_z2) + np.abs(one_z2) * (eps_c + 2 * U)) + r_err4 * np.abs(one_z2))
        b_s = np.where(floored, 0.0, b_s + ETA * (1 + np.abs(c4)) * (1 + np.abs(one_z2)))
        valid3 = mask[:, :, None]
        grad = np.where(valid3, np.concatenate((g_a, g_mu.reshape(b, t, k * d), g_s.reshape(b, t, k * d)), axis=2), 0.0)
        grad_bound = np.where(valid3, np.concatenate((b_a, b_mu.reshape(b, t, k * d), b_s.reshape(b, t, k * d)), axis=2), 0.0)
        # selection
        component = np.where(mask, np.argmax(a, axis=2), 0).astype(np.int64)
        pick = component[:, :, None, None]
        mean = np.where(valid3, np.take_along_axis(mu, pick, axis=2)[:, :, 0, :], 0.0)
        variance = np.where(valid3, np.exp(2.0 * np.take_along_axis(s, pick, axis=2)[:, :, 0, :]), 1.0)
        variance_bound = np.where(valid3, variance * (2 * eps_e + 2 * U) + ETA, 0.0)
    return {'frame_loss': l, 'frame_bound': frame_bound, 'loss': loss, 'loss_bound': loss_bound, 'grad': grad, 'grad_bound': grad_bound,
            'component': component, 'mean': mean, 'variance': variance, 'variance_bound': variance_bound, 'mask': mask,
            'floored': floored, 'responsibility': r}


# ------------------------------------------------------------------------------------------------ the inputs the tests share
SWEEP_B, SWEEP_T = 3, 37                                  # 37: no multiple of the kernel's frames per workgroup (16, 4)
SWEEP_SEQ_LEN = (37, 20, 1)
LOGIT_GAP = 1e-3
# (K, D): the regimes of csrc/mdn.hip - K * D = 64 | 65, 128 | 129, 256 | 257, 512 | 513 (pairs per lane 1 | 2 | 4 | 8 | 16),
# 1024 | 1025 (registers | re-read), D = 16 | 17 (one lane per component | lanes stride d), both caps (K = 64, K * D = 16384)
SWEEP = ((1, 1), (2, 3), (8, 3), (16, 3), (64, 1), (64, 3), (3, 65), (4, 180), (5, 205), (16, 1024),
         (13, 5), (64, 2), (43, 3), (64, 4), (1, 257), (64, 8), (27, 19), (64, 16), (1, 1024), (4, 16), (4, 17), (60, 17), (1, 1025))


def range_cases(seed=20261020):
    """The range inputs, K = 8, D = 3, B = 3, T = 37, seq_len = (37, 20, 1), from the sweep's input:
    ``far``: every target 2000 standard deviations from every mean (s = 0, means ~ N(0, 1), y = 2000): each q_k is about -6e6;
    ``dominant``: one component's logit 80 nats above the others;  ``s_minus10`` / ``s_plus10``: every log-std -10 (means within a
    few e^-10 of the target) / +10;  ``minus_inf``: one -inf logit per frame."""
    k, d = 8, 3
    pred, target, seq_len = sweep_case(k, d)
    rng = np.random.RandomState(seed)
    b, t = SWEEP_B, SWEEP_T
    cases = {}
    far = pred.copy()
    far[:, :, k:k + k * d] = rng.standard_normal((b, t, k * d))
    far[:, :, k + k * d:] = 0.0
    cases['far'] = (far, np.full_like(target, 2000.0), seq_len)
    dominant = pred.copy()
    dominant[:, :, :k] = rng.standard_normal((b, t, k))
    np.put_along_axis(dominant[:, :, :k], rng.randint(0, k, size=(b, t, 1)), np.float32(80.0), axis=2)
    dominant[:, :, :k] += (dominant[:, :, :k] == 80.0) * np.float32(3.0)
    cases['dominant'] = (dominant, target, seq_len)
    tight = pred.copy()
    tight[:, :, k + k * d:] = -10.0
    tight[:, :, k:k + k * d] = (target[:, :, None, :] + np.exp(-10.0) * rng.standard_normal((b, t, k, d))).reshape(b, t, k * d)
    cases['s_minus10'] = (tight, target, seq_len)
    loose = pred.copy()
    loose[:, :, k + k * d:] = 10.0
    cases['s_plus10'] = (loose, target, seq_len)
    minus_inf = pred.copy()
    np.put_along_axis(minus_inf[:, :, :k], rng.randint(0, k, size=(b, t, 1)), -np.inf, axis=2)
    cases['minus_inf'] = (minus_inf, target, seq_len)
    return k, d, cases


def sweep_case(k, d, seed=20261019):
    """The sweep's input at K components of width D: B = 3, T = 37, seq_len = (37, 20, 1).  Logits ~ 2 N(0, 1) with a top-two gap of at
    least LOGIT_GAP in every frame (the selected component is unambiguous in fp32); targets ~ 1.5 N(0, 1); means = target + noise and
    log-stds = -0.5 + noise, the noise scaled by min(1, 2 / sqrt(D)) so that several components keep a share of every frame at every
    D (unscaled, sum_d separates them by about sqrt(D) nats and all but one responsibility underflow)."""
    rng = np.random.RandomState(seed + 100003 * k + d)
    b, t = SWEEP_B, SWEEP_T
    scale = min(1.0, 2.0 / np.sqrt(d))
    logits = (2.0 * rng.standard_normal((b, t, k))).astype(np.float32)
    target = (1.5 * rng.standard_normal((b, t, d))).astype(np.float32)
    means = (target[:, :, None, :] + scale * rng.standard_normal((b, t, k, d))).astype(np.float32)
    log_std = (-0.5 + 0.5 * scale * rng.standard_normal((b, t, k, d))).astype(np.float32)
    if k > 1:
        order = np.sort(logits, axis=2)
        close = (order[:, :, -1] - order[:, :, -2]) < 4 * LOGIT_GAP
        top = np.argmax(logits, axis=2)
        bump = np.zeros_like(logits)
        np.put_along_axis(bump, top[:, :, None], np.where(close, np.float32(0.0625), np.float32(0.0))[:, :, None], axis=2)
        logits = logits + bump
        order = np.sort(logits.astype(F64), axis=2)
        assert np.all(order[:, :, -1] - order[:, :, -2] >= LOGIT_GAP), 'sweep_case: two logits within the gap'
    pred = np.concatenate((logits, means.reshape(b, t, k * d), log_std.reshape(b, t, k * d)), axis=2).astype(np.float32)
    assert pred.shape[2] == width(k, d)
    return pred, target, np.array(SWEEP_SEQ_LEN, dtype=np.int64)
