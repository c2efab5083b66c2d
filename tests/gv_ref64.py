"""Two-pass restatement of the global-variance loss behind ``losses.gv`` (mg_gv_f32 / mg_gv_bwd_f32 of include/morgana_hip.h) in
long double, with DERIVED bounds for what the kernel may differ from it.  Plain numpy, no GPU and no torch.  The reference project has
no global-variance loss, so there is no golden file: this module is the reference.

For x (B, T, D), n_b = seq_len[b] clamped to [0, T] (T without seq_len), over the valid frames t < n_b:

    m[b,d] = mean_t x[b,t,d]            v[b,d] = mean_t (x[b,t,d] - m[b,d])^2           (biased; the mean first, then the squares)
    f(v)   = log(v + eps) | v           delta = f(v_pred) - f(v_tgt)                    L = (1 / (B D)) sum_{b,d} delta^2
    c[b,d] = (2 / (B D)) delta f'(v_pred) (2 / n_b)                                     grad[b,t,d] = g c (x_pred[b,t,d] - m_pred[b,d])

grad is exactly 0 on pad frames (which are never read) and NaN on every frame of an utterance with n_b == 0, whose loss is NaN.

What the kernel may differ by.  u = 2^-53 (float64), U = 2^-24 (float32).  Per (b, d, operand) let R = max - min of the valid
frames.  The kernel forms every value from float64 terms that lie in the hull of the samples: deviations x - k from a sample k and
differences of means of samples, each at most R, and their squares, at most R^2.  There are at most n of them, M2 = n v is at most
n R^2, and a term passes through at most n + 32 roundings on its way (the running sums of a chunk of 32, the Chan merges, the LDS
tree, the chunk merge), each relative to a partial sum that n R^2 (or n R) bounds.  With gamma = 4 (n + 32) u - the 4 covers the
difference s2 - s1^2 / n of a shifted chunk (two terms of up to 32 R^2) and the three products of a merge -

    |v_k - v| <= e_v = gamma R^2        |m_k - m| <= e_m = gamma R + u |m|              (the anchor x[b,0,d] is added back once)
    log:    e_f = e_v / (v + eps) + u + 4 u |f|      (the sum v + eps, a library log good to a few ulp)
            e_f' = (e_v + u (v + eps)) / (v + eps)^2 + u f'
    linear: e_f = e_v,  e_f' = 0
    e_delta = e_f(pred) + e_f(tgt) + u |delta|
    e_term  = 2 |delta| e_delta + e_delta^2 + u delta^2
    loss:   |loss_k - L| <= U |L|  +  [ mean(e_term) + (B D + 2) u L ]                  one float32 rounding + the float64 term
    e_c     = (4 / (B D n)) (e_delta f' + |delta| e_f') + 4 u |c|
    grad:   |grad_k - grad| <= U |grad|  +  [ |g| (|c| e_m + |x - m| e_c) + 3 u |grad| ]     one float32 rounding + the float64 term:
            the error of m_pred through x - m, and that of c through the product

A constant column has R = 0: v == 0 exactly.  n_b == 1 likewise, and m == x: the gradient is exactly 0.
"""
import numpy as np

LD = np.longdouble
F64 = np.float64
U = 2.0 ** -24
u = 2.0 ** -53


def valid_frames(seq_len, b, t):
    if seq_len is None:
        return np.full(b, t, dtype=np.int64)
    return np.clip(np.asarray(seq_len, dtype=np.int64), 0, t)


def _moments(x, n):
    """x (B, T, D) float32 -> (m, v, R) as (B, D) long doubles over the first n[b] frames; NaN where n[b] == 0."""
    b, _, d = x.shape
    m, v, r = (np.full((b, d), np.nan, dtype=LD) for _ in range(3))
    for i in range(b):
        if n[i] > 0:
            seg = x[i, :n[i]].astype(LD)
            m[i] = seg.sum(axis=0) / LD(n[i])
            v[i] = ((seg - m[i]) ** 2).sum(axis=0) / LD(n[i])
            r[i] = seg.max(axis=0) - seg.min(axis=0)
    return m, v, r


def _f(v, log, eps):
    with np.errstate(all='ignore'):
        return (np.log(v + LD(eps)), 1 / (v + LD(eps))) if log else (v, np.ones_like(v))


def gv(pred, tgt, seq_len=None, log=True, eps=1e-6, grad_scale=1.0):
    """Long-double values (returned as float64) and the derived bounds.  pred, tgt (B, T, D) float32.  Returns a dict: ``loss``,
    ``grad`` (B, T, D), ``mask`` (B, T) bool, ``m_pred`` / ``v_pred`` / ``v_tgt`` / ``c`` (B, D), ``loss_rounding`` and
    ``loss_float64`` (their sum is ``loss_bound``), ``grad_rounding`` and ``grad_float64`` (B, T, D; their sum is ``grad_bound``)."""
    pred, tgt = np.asarray(pred, dtype=np.float32), np.asarray(tgt, dtype=np.float32)
    b, t, d = pred.shape
    n = valid_frames(seq_len, b, t)
    nf = n.astype(LD)[:, None]
    mask = np.arange(t)[None, :] < n[:, None]
    mp, vp, rp = _moments(pred, n)
    _, vt, rt = _moments(tgt, n)
    fp, slope = _f(vp, log, eps)
    ft, _ = _f(vt, log, eps)
    with np.errstate(all='ignore'):
        delta = fp - ft
        loss = (delta ** 2).sum() / LD(b * d)
        c = (LD(2) / LD(b * d)) * delta * slope * (LD(2) / nf)
        dev = np.where(mask[:, :, None], pred.astype(LD) - mp[:, None, :], LD(0))
        grad = LD(grad_scale) * c[:, None, :] * dev
        grad = np.where(mask[:, :, None], grad, LD(0))
        grad[n == 0] = np.nan

        # the bounds of the module docstring
        gamma = 4 * (nf + 32) * u
        ev_p, ev_t = gamma * rp ** 2, gamma * rt ** 2
        e_m = gamma * rp + u * np.abs(mp)
        if log:
            ef_p = ev_p / (vp + eps) + u + 4 * u * np.abs(fp)
            ef_t = ev_t / (vt + eps) + u + 4 * u * np.abs(ft)
            e_slope = (ev_p + u * (vp + eps)) / (vp + eps) ** 2 + u * slope
        else:
            ef_p, ef_t, e_slope = ev_p, ev_t, np.zeros_like(vp)
        e_delta = ef_p + ef_t + u * np.abs(delta)
        e_term = 2 * np.abs(delta) * e_delta + e_delta ** 2 + u * delta ** 2
        loss_float64 = e_term.sum() / (b * d) + (b * d + 2) * u * loss
        e_c = (4 / (b * d * nf)) * (e_delta * slope + np.abs(delta) * e_slope) + 4 * u * np.abs(c)
        grad_float64 = abs(grad_scale) * (np.abs(c) * e_m)[:, None, :] + abs(grad_scale) * np.abs(dev) * e_c[:, None, :] + 3 * u * np.abs(grad)
        grad_float64 = np.where(mask[:, :, None], grad_float64, 0)
    out = {'loss': F64(loss), 'grad': grad.astype(F64), 'mask': mask, 'm_pred': mp.astype(F64), 'v_pred': vp.astype(F64),
           'v_tgt': vt.astype(F64), 'c': c.astype(F64),
           'loss_rounding': U * abs(F64(loss)), 'loss_float64': F64(loss_float64),
           'grad_rounding': U * np.abs(grad).astype(F64), 'grad_float64': grad_float64.astype(F64)}
    out['loss_bound'] = out['loss_rounding'] + out['loss_float64']
    out['grad_bound'] = out['grad_rounding'] + out['grad_float64']
    return out


def variance_bound(x, seq_len=None):
    """(v (B, D) float64, bound (B, D)) for ``losses.global_variance``: one float32 rounding of v plus e_v."""
    x = np.asarray(x, dtype=np.float32)
    n = valid_frames(seq_len, x.shape[0], x.shape[1])
    _, v, r = _moments(x, n)
    e_v = 4 * (n.astype(LD)[:, None] + 32) * u * r ** 2
    return v.astype(F64), (U * np.abs(v) + e_v).astype(F64)


def report(name, ref, loss=None, grad=None):
    """Prints both terms of both bounds (and, given the kernel's results, where they fall)."""
    with np.errstate(all='ignore'):
        line = '%s: loss %.9g  bound = rounding %.3e + float64 %.3e' % (name, ref['loss'], ref['loss_rounding'], ref['loss_float64'])
        if loss is not None:
            line += '  |err| %.3e' % abs(float(loss) - ref['loss'])
        line += ';  gradient bound (worst element) = rounding %.3e + float64 %.3e' % (np.nanmax(ref['grad_rounding']),
                                                                                      np.nanmax(ref['grad_float64']))
        if grad is not None:
            err = np.abs(np.asarray(grad, dtype=F64) - ref['grad'])
            line += '  worst |err| / bound %.3f' % float(np.nanmax(np.where(ref['grad_bound'] > 0, err / ref['grad_bound'], 0)))
    print(line)


# ------------------------------------------------------------------------------------------------------- the inputs both test files use
SEQ_LENS = ('head', 'tail', None)


def seq_len_case(kind, chunk):
    """(B,) lengths for B = 3, T = chunk + 3: one frame / a whole chunk / one past it, or every frame / one short of a chunk / two."""
    return {'head': [1, chunk, chunk + 1], 'tail': [chunk + 3, chunk - 1, 2], None: None}[kind]


def case(chunk, d, seed=0):
    """(pred, tgt) float32 (3, chunk + 3, d): an over-smoothed prediction (0.6 of the natural spread) of a natural trajectory."""
    rng = np.random.RandomState(1000 * d + seed)
    t = chunk + 3
    tgt = (rng.standard_normal((3, t, d)) * rng.uniform(0.5, 2.0, (1, 1, d)) + rng.uniform(-1, 1, (1, 1, d))).astype(np.float32)
    pred = (0.6 * tgt + 0.2 * rng.standard_normal((3, t, d)) + 0.1).astype(np.float32)
    return pred, tgt


def offset_case(chunk, seed=5):
    """D = 5: column 0 at 16384 with standard deviation 2^-6 (a sum of raw squares loses it), column 1 lf0-like at 5 +- 0.25, the rest
    standard normal."""
    rng = np.random.RandomState(seed)
    t = chunk + 3
    tgt = rng.standard_normal((3, t, 5))
    pred = 0.7 * tgt + 0.1 * rng.standard_normal((3, t, 5))
    for x, s in ((tgt, 1.0), (pred, 0.8)):
        x[:, :, 0] = 16384.0 + s * 2.0 ** -6 * rng.standard_normal((3, t))
        x[:, :, 1] = 5.0 + s * 0.25 * rng.standard_normal((3, t))
    return pred.astype(np.float32), tgt.astype(np.float32)


def other_order(pred, tgt, seq_len=None, log=True, eps=1e-6, grad_scale=1.0):
    """The same two-pass definition on the float32 inputs, accumulated in float64 in ANOTHER order than the kernel's or the
    restatement's (frames in descending order, one after the other), results rounded to float32 as the kernel rounds them."""
    pred, tgt = np.asarray(pred, dtype=np.float32), np.asarray(tgt, dtype=np.float32)
    b, t, d = pred.shape
    n = valid_frames(seq_len, b, t)
    total, grad = F64(0), np.zeros((b, t, d), dtype=np.float32)
    for i in range(b):
        if n[i] == 0:
            total, grad[i] = F64(np.nan), np.nan
            continue
        stats = []
        for x in (pred, tgt):
            m, v = np.zeros(d), np.zeros(d)
            for k in range(n[i] - 1, -1, -1):
                m = m + x[i, k].astype(F64)
            m = m / n[i]
            for k in range(n[i] - 1, -1, -1):
                v = v + (x[i, k].astype(F64) - m) ** 2
            stats.append((m, v / n[i]))
        (mp, vp), (_, vt) = stats
        delta = np.log(vp + eps) - np.log(vt + eps) if log else vp - vt
        slope = 1 / (vp + eps) if log else np.ones(d)
        for k in range(d):
            total = total + delta[k] ** 2
        c = (2.0 / (b * d)) * delta * slope * (2.0 / n[i])
        grad[i, :n[i]] = (grad_scale * c * (pred[i, :n[i]].astype(F64) - mp)).astype(np.float32)
    return np.float32(total / (b * d)), grad


def raw_squares_loss(pred, tgt, seq_len=None, log=True, eps=1e-6):
    """The loss with v = E[x^2] - E[x]^2 in float64: what the kernel must NOT compute."""
    pred, tgt = np.asarray(pred, dtype=F64), np.asarray(tgt, dtype=F64)
    b, t, d = pred.shape
    n = valid_frames(seq_len, b, t)
    total = 0.0
    for i in range(b):
        vs = []
        for x in (pred, tgt):
            seg = x[i, :n[i]]
            vs.append((seg ** 2).sum(axis=0) / n[i] - (seg.sum(axis=0) / n[i]) ** 2)
        delta = np.log(vs[0] + eps) - np.log(vs[1] + eps) if log else vs[0] - vs[1]
        total += (delta ** 2).sum()
    return total / (b * d)


if __name__ == '__main__':
    for dim in (1, 5, 60, 67):
        for kind in SEQ_LENS:
            for log_variance in (True, False):
                p, y = case(256, dim)
                report('D=%d seq_len=%s log=%s' % (dim, kind, log_variance), gv(p, y, seq_len_case(kind, 256), log=log_variance))
    report('offset', gv(*offset_case(256)))
