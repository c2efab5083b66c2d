"""Float64 reference of the masked categorical cross entropy behind mg_masked_ce_f32 (include/morgana_hip.h), with a DERIVED fp32
rounding bound for the per-frame loss, the total loss and every gradient element.

Plain numpy, no GPU and no torch.  What is computed (morgana/losses.py:29-46 around :59-61, restated independently):

    l[b,t]      = logsumexp_c x[b,t,:] - x[b,t,y[b,t]]              (0 where y == -100, NaN where y is otherwise outside [0, C))
    L           = mean_b( sum_{t < n_b} l[b,t] / n_b ),              n_b = seq_len[b] clamped to [0, T]  (T without seq_len)
    g[b,t,c]    = grad_scale (softmax(x[b,t,:])[c] - [c == y]) / (n_b B)   for t < n_b, 0 for pad frames and for frames whose
                  target is -100 or out of range

The bound is a property of fp32 arithmetic, not of any kernel.  U = 2^-24 is the unit roundoff; every elementary operation returns
its exact result times (1 + d), |d| <= U; products of error terms are dropped (first order).  The evaluation it covers is the
max-subtracted one: M = max_c x_c (exact), d_c = x_c - M, e_c = expf(d_c), s = sum_c e_c, then either l = (M + logf(s)) - x_y (one
pass over registers) or l = -((x_y - M) - logf(s)) (log_softmax, then the pick); the gradient from p_c = e_c / s or from
p_c = expf((x_c - M) - logf(s)).  Both orders are covered: each term below is the larger of the two.

  * d_c carries |d_c| U absolute, which expf turns into a RELATIVE error |d_c| U of e_c; expf itself is good to EXP_ULPS units in
    the last place, i.e. EXP_ULPS * 2U relative (HIP's expf and glibc's are documented at 1 ulp; 2 is charged).  The terms enter s
    weighted by e_c / s, so the relative error of s from its terms is  U sum_c e_c |d_c| / s + 2 EXP_ULPS U  (the first part is
    evaluated exactly from the data in float64: it is the softmax-weighted mean distance from the maximum).
  * the sum itself: all terms are positive, so a term that passes through k additions picks up at most k U relative.  The sum is
    taken to be BLOCKED over W >= 8 accumulators: ceil(C / W) - 1 serial additions inside an accumulator, then a binary tree
    over the accumulators, log2 W levels.  W = 8 or 16 is a CPU's vector sum (torch's CPU kernel), W = 64 a wave striding the row
    with a cross-lane tree, W = 256 a workgroup (two tree stages, 6 + 2 levels).  DEPTH(C) = ceil(C / 8) + 8 additions covers all
    of them: the tree part never exceeds 8 levels (log2 C of them for a row of up to a wave), the serial part is longest at W = 8.
  * rho_s = U sum e|d| / s + 2 EXP_ULPS U + DEPTH(C) U is the relative error of s, hence the absolute error of log s; logf adds
    LOG_ULPS * 2U |log s| (1 ulp documented, 2 charged); the first of the two remaining operations rounds M + log s (U |lse|) or
    x_y - M (U |d_y|), the second one rounds l itself (U |l|):

        bound_l = rho_s + 2 LOG_ULPS U |log s| + U max(|lse|, |d_y|) + U |l|

  * total loss: sum_t l / n_b and the mean over b, in ANY order: (T + B) U relative to sum |l| on top of the frames' own bounds, one
    more U for each of the two divisions:   bound_L = mean_b( sum_t (bound_l + (T + B + 2) U |l|) / n_b ).
  * gradient: p_c = e_c / s has relative error |d_c| U + 2 EXP_ULPS U (its own e_c) + rho_s (the sum) + 3U (a reciprocal and a
    product, or a division).  p_c = expf(lp_c), lp_c = d_c - log s, has the absolute error of lp_c as its relative error:
    U |d_c| (d_c) + U |lp_c| (the subtraction; |lp_c| <= |d_c| + |log s|) + rho_s + 2 LOG_ULPS U |log s| (log s), and 2 EXP_ULPS U of
    expf.  The sum of the two lists' maxima is charged.  p_c - [c == y] adds U |p_c - [c == y]|, the coefficient
    grad_scale / (n_b B) - a product or quotient of up to three factors - is good to 3U and its product adds U:

        bound_g = |coef| ( p_c (2 |d_c| U + 2 EXP_ULPS U + rho_s + 3U + (1 + 2 LOG_ULPS) U |log s|) + 5U |p_c - [c == y]| )
                  + ETA        (ETA = 2^-149: a gradient that underflows is rounded on the subnormal grid, absolutely)

A -inf logit is exact (e_c = 0 in both evaluations) and is left out of the weighted distance."""
import numpy as np

F64 = np.float64
U = 2.0 ** -24
ETA = 2.0 ** -149
EXP_ULPS = 2.0
LOG_ULPS = 2.0
IGNORE = -100


def depth(c):
    """Additions a term of the blocked sum of C terms passes through (see the module docstring)."""
    return int(np.ceil(c / 8.0)) + 8


def valid_frames(seq_len, b, t):
    if seq_len is None:
        return np.full(b, t, dtype=np.int64)
    return np.clip(np.asarray(seq_len, dtype=np.int64), 0, t)


def ce(pred, target, seq_len=None, grad_scale=1.0):
    """Float64 values and fp32 bounds.  pred (B, T, C), target (B, T) integers.  Returns a dict: ``frame_loss`` / ``frame_bound``
    (B, T) (0 on pad frames), ``loss`` / ``loss_bound`` (scalars), ``grad`` / ``grad_bound`` (B, T, C), ``argmax`` (B, T) (0 on pad
    frames), ``mask`` (B, T) bool."""
    x = np.asarray(pred, dtype=F64)
    y = np.asarray(target, dtype=np.int64)
    b, t, c = x.shape
    assert y.shape == (b, t)
    n = valid_frames(seq_len, b, t)
    mask = np.arange(t)[None, :] < n[:, None]
    with np.errstate(all='ignore'):
        m = x.max(axis=2)
        d = x - m[:, :, None]
        e = np.exp(d)
        s = e.sum(axis=2)
        log_s = np.log(s)
        lse = m + log_s
        ignore = y == IGNORE
        bad = ((y < 0) | (y >= c)) & ~ignore
        y_safe = np.where(ignore | bad, 0, y)
        x_y = np.take_along_axis(x, y_safe[:, :, None], axis=2)[:, :, 0]
        l = lse - x_y
        l = np.where(ignore, 0.0, np.where(bad, np.nan, l))
        l = np.where(mask, l, 0.0)
        dist = np.where(np.isfinite(d), e * np.abs(d), 0.0).sum(axis=2) / s
        rho_s = U * dist + 2 * EXP_ULPS * U + depth(c) * U
        d_y = np.take_along_axis(d, y_safe[:, :, None], axis=2)[:, :, 0]
        frame_bound = rho_s + 2 * LOG_ULPS * U * np.abs(log_s) + U * np.maximum(np.abs(lse), np.abs(d_y)) + U * np.abs(l)
        frame_bound = np.where(mask & ~ignore, frame_bound, 0.0)
        nf = n.astype(F64)
        loss = np.mean(np.where(mask, l, 0.0).sum(axis=1) / nf)
        loss_bound = np.mean((frame_bound + (t + b + 2) * U * np.abs(l)).sum(axis=1) / nf)
        p = e / s[:, :, None]
        onehot = np.arange(c)[None, None, :] == y_safe[:, :, None]
        coef = (grad_scale / (nf * b))[:, None, None]
        live = (mask & ~ignore & ~bad)[:, :, None]
        grad = np.where(live, coef * (p - onehot), 0.0)
        absd = np.where(np.isfinite(d), np.abs(d), 0.0)
        rel = 2 * absd * U + 2 * EXP_ULPS * U + rho_s[:, :, None] + 3 * U + (1 + 2 * LOG_ULPS) * U * np.abs(log_s)[:, :, None]
        grad_bound = np.where(live, np.abs(coef) * (p * rel + 5 * U * np.abs(p - onehot)) + ETA, 0.0)
    argmax = np.where(mask, np.argmax(x, axis=2), 0).astype(np.int64)
    return {'frame_loss': l, 'frame_bound': frame_bound, 'loss': loss, 'loss_bound': loss_bound, 'grad': grad, 'grad_bound': grad_bound,
            'argmax': argmax, 'mask': mask}


# ------------------------------------------------------------------------------------------------ the inputs the tests share
REG_MAX = 1024           # widest row of the kernel's one-wave-per-row path (csrc/ce.hip: CE_REG_MAX)
MAX_CLASSES = 65536      # MG_CE_MAX_CLASSES
SWEEP_CLASSES = (1, 2, 63, 64, 65, 255, REG_MAX, REG_MAX + 1, MAX_CLASSES - 1)
SWEEP_SEQ_LEN = (5, 3)


def sweep_case(c, seed=20261017):
    """The class-count sweep's input at C classes: B=2, T=5, seq_len=[5, 3]; logits ~ 3 N(0, 1), one exact tie for the maximum in
    frame (0, 1) when C > 2 (argmax must name the lower index)."""
    rng = np.random.RandomState(seed + c)
    pred = (rng.standard_normal((2, 5, c)) * 3.0).astype(np.float32)
    if c > 2:
        pred[0, 1, c - 1] = pred[0, 1, c // 2] = np.float32(np.abs(pred[0, 1]).max() + 1.0)
    target = rng.randint(0, c, size=(2, 5)).astype(np.int64)
    return pred, target, np.array(SWEEP_SEQ_LEN, dtype=np.int64)


def range_cases(seed=20261018):
    """The three range inputs (B=2, T=5, C=37, seq_len=[5, 3]): logits scaled to +-80, one logit of 1e4, a -inf non-target logit."""
    rng = np.random.RandomState(seed)
    base = rng.standard_normal((2, 5, 37)).astype(np.float32)
    target = rng.randint(0, 37, size=(2, 5)).astype(np.int64)
    seq_len = np.array(SWEEP_SEQ_LEN, dtype=np.int64)
    wide = (base / np.abs(base).max() * 80.0).astype(np.float32)
    spike = base.copy()
    spike[0, 2, 5] = 1e4
    spike[1, 1, int(target[1, 1])] = 1e4
    minus_inf = base.copy()
    for (i, j) in ((0, 0), (0, 4), (1, 2)):
        minus_inf[i, j, (int(target[i, j]) + 3) % 37] = -np.inf
    return {'pm80': (wide, target, seq_len), 'spike_1e4': (spike, target, seq_len), 'minus_inf': (minus_inf, target, seq_len)}
