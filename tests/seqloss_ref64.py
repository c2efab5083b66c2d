"""Float64 restatement of the reduction behind ``losses.sequence_loss`` (mg_seq_mean_f32 / mg_seq_mean_bwd_f32 of
include/morgana_hip.h; morgana/losses.py:29-46 restated independently), with DERIVED bounds for what may differ from it.

Plain numpy, no GPU and no torch.  For a feature loss x (B, T, D) and n_b = seq_len[b] clamped to [0, T] (T without seq_len):

    L64        = (1 / (B D)) sum_b ( sum_{t < T, d} x[b,t,d] m[b,t] ) / n_b,     m[b,t] = (t < n_b)
    A64        = the same expression on |x|: the scale every summation error is relative to
    g64[b,t,d] = grad_scale / (n_b B D) for t < n_b, 0 on the pad frames of an utterance with n_b > 0, NaN on every frame of an
                 utterance with n_b == 0

Every frame enters the sum multiplied by its mask value, so a NaN or Inf in a pad frame makes L64 NaN; n_b == 0 gives 0 / 0 = NaN.
U = 2^-24 is fp32's unit roundoff, 2^-53 float64's.

  * The kernel against the restatement.  The kernel adds float64 terms: an element passes through fewer than T D additions, each good
    to 2^-53 relative to the partial sum it forms, which |x| bounds - at most T D 2^-53 A64, charged as T D 2^-52 A64 to cover the
    division by n_b, the mean and the restatement's own float64 sum - and then rounds ONCE to fp32: U |L64|.

        |loss - L64| <= U |L64| + T D 2^-52 A64            |grad - g64| <= U |g64|   (a float64 quotient rounded once)

  * The reference's fp32 evaluation (the golden file) against the restatement.  It sums T terms per (b, d) in fp32, divides, and
    takes the mean of B D values: a summand passes through at most T + B D additions and three more operations (the mask product, the
    division by n_b, the division of the mean), each U relative to a partial sum that |x| bounds.

        |golden - L64| <= (T + B D + 3) U A64              |golden - g64| <= 2 U |g64|   (two fp32 roundings: 1 / n_b, then / (B D))
"""
import numpy as np

F64 = np.float64
U = 2.0 ** -24


def valid_frames(seq_len, b, t):
    if seq_len is None:
        return np.full(b, t, dtype=np.int64)
    return np.clip(np.asarray(seq_len, dtype=np.int64), 0, t)


def seq_mean(x, seq_len=None, grad_scale=1.0):
    """Float64 values and the derived bounds.  x (B, T, D).  Returns a dict: ``loss`` (L64), ``abs_loss`` (A64), ``grad`` (g64,
    (B, T, D)), ``mask`` (B, T) bool, ``kernel_loss_bound`` / ``kernel_grad_bound`` and ``golden_loss_bound`` / ``golden_grad_bound``
    (the gradient bounds elementwise)."""
    x = np.asarray(x, dtype=F64)
    b, t, d = x.shape
    n = valid_frames(seq_len, b, t)
    mask = np.arange(t)[None, :] < n[:, None]
    m = mask.astype(F64)[:, :, None]
    nf = n.astype(F64)
    with np.errstate(all='ignore'):
        loss = ((x * m).sum(axis=(1, 2)) / nf).sum() / (b * d)
        abs_loss = ((np.abs(x) * m).sum(axis=(1, 2)) / nf).sum() / (b * d)
        coef = F64(grad_scale) / (nf * b * d)
    grad = np.where(mask[:, :, None], coef[:, None, None], 0.0) * np.ones((1, 1, d))
    grad[n == 0] = np.nan
    return {'loss': loss, 'abs_loss': abs_loss, 'grad': grad, 'mask': mask,
            'kernel_loss_bound': U * abs(loss) + t * d * 2.0 ** -52 * abs_loss, 'kernel_grad_bound': U * np.abs(grad),
            'golden_loss_bound': (t + b * d + 3) * U * abs_loss, 'golden_grad_bound': 2 * U * np.abs(grad)}


GOLDEN = 'g20_sequence_loss.npz'
GOLDEN_CASES = ('huber', 'l1_d1', 'l1_full', 'l1_long', 'l1_ragged', 'nll', 'signed')


def golden_case(g, name):
    """(pred, target, seq_len or None, feature_loss, loss, grad_feature, grad_pred) of one case of the loaded golden file."""
    return (g[name + '__pred'], g[name + '__target'], g.get(name + '__seq_len'), g[name + '__feature_loss'], float(g[name + '__loss']),
            g[name + '__grad_feature'], g[name + '__grad_pred'])
