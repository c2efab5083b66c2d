"""Mirror of ``morgana.losses`` for the hot path.  Reference: morgana/losses.py:9-51 (``sequence_loss`` / ``mse``), :54-56 (``bce``),
:59-61 (``ce``) and :64-67 (``KLD_standard_normal``)."""
import functools

import torch

from . import functional as F_hip
from . import ops


def sequence_loss(loss_fn):
    r"""Sequence loss wrapper of the reference (losses.py:9-46): turns ``loss_fn(predictions, targets)``, which returns the loss of
    every frame and feature, into ``wrapped(predictions, targets, seq_len=None)``: the per-utterance mean over the valid frames, then
    the mean over (batch, feature).  The extension point for a model's own loss::

        @losses.sequence_loss
        def l1(predictions, targets):
            return F.l1_loss(predictions, targets, reduction='none')

    ``loss_fn`` runs as the torch ops it is written in, and autograd flows through them.  Its result - a (B, T, D') float32 device
    tensor; D' need not be the predictions' width - is reduced by one HIP pass in float64 and a one-workgroup finish, read in place
    whatever its strides, and the backward writes d loss / d feature loss in one launch (csrc/seqmean.hip through
    ``functional.SeqMeanFn``; the reference runs a host-built mask, mul, two sums, div and mean, then their autograd mirrors).  Every
    frame is read and multiplied by its mask value, so a NaN in a pad frame gives NaN, and ``seq_len[b] == 0`` gives NaN, both as in
    the reference.  ``seq_len``: (B,) integers or None (every frame valid).  No double backward through the reduction."""

    @functools.wraps(loss_fn)
    def wrapped_loss(predictions, targets, seq_len=None):
        feature_loss = loss_fn(predictions, targets)
        name = getattr(loss_fn, '__name__', 'loss_fn')
        if not isinstance(feature_loss, torch.Tensor):
            raise TypeError('sequence_loss: %s must return a torch.Tensor, got %s' % (name, type(feature_loss)))
        if feature_loss.dim() != 3:
            raise ValueError('sequence_loss: %s must return a (B, T, D) feature loss, got shape %s' % (name, tuple(feature_loss.shape)))
        if feature_loss.dtype != torch.float32:
            raise TypeError('sequence_loss: %s must return a torch.float32 feature loss, got %s' % (name, feature_loss.dtype))
        if seq_len is not None:
            if not isinstance(seq_len, torch.Tensor) or seq_len.is_floating_point() or seq_len.is_complex() or seq_len.dtype == torch.bool:
                raise TypeError('sequence_loss: seq_len must be a tensor of integers, got %s'
                                % (seq_len.dtype if isinstance(seq_len, torch.Tensor) else type(seq_len)))
            if tuple(seq_len.shape) != (feature_loss.shape[0],):
                raise ValueError('sequence_loss: seq_len must be (B,) = (%d,), got %s' % (feature_loss.shape[0], tuple(seq_len.shape)))
            if seq_len.dtype != torch.int64:
                seq_len = seq_len.long()
        return F_hip.SeqMeanFn.apply(feature_loss, seq_len)

    return wrapped_loss


def mse(predictions, targets, seq_len=None):
    """Masked mean-squared error: per-utterance mean over valid frames, then mean over (batch, feature).

    Argument order is the reference wrapper's ``(predictions, targets, seq_len)`` (losses.py:30).  One HIP pass
    computes the loss and d loss / d predictions (the reference runs mse_loss, a host-built mask, mul, two sums, div
    and mean, then their autograd mirrors).  ``seq_len[b] == 0`` gives NaN, as in the reference.
    """
    if seq_len is not None and seq_len.dtype != torch.int64:
        seq_len = seq_len.long()
    if targets.shape[1] != predictions.shape[1]:
        raise RuntimeError('The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension 1'
                           % (predictions.shape[1], targets.shape[1]))
    return F_hip.MaskedMSEFn.apply(predictions, targets, seq_len)


def bce(predictions, targets, seq_len=None):
    """Masked binary cross entropy with the same per-utterance averaging as ``mse`` (reference: losses.py:54-56; the voicing
    stream of models/RNN_SPSS.py:137).  Logs are clamped at -100, as ``F.binary_cross_entropy`` does."""
    if seq_len is not None and seq_len.dtype != torch.int64:
        seq_len = seq_len.long()
    if targets.shape[1] != predictions.shape[1]:
        raise RuntimeError('The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension 1'
                           % (predictions.shape[1], targets.shape[1]))
    return F_hip.MaskedMSEFn.apply(predictions, targets, seq_len, 'bce')


def _class_targets(predictions, targets):
    """Class indices as the kernel reads them: (B, T) int64 (``(B, T, 1)`` is squeezed, int32 / int16 / int8 / uint8 are widened)."""
    if not isinstance(targets, torch.Tensor):
        raise TypeError('ce: targets must be a torch.Tensor of class indices, got %s' % type(targets))
    if targets.is_floating_point() or targets.is_complex() or targets.dtype == torch.bool:
        raise TypeError('ce: targets must hold integer class indices, got %s' % targets.dtype)
    if targets.dim() == 3 and targets.shape[2] == 1:
        targets = targets[:, :, 0]
    if targets.dim() != 2 or targets.shape[0] != predictions.shape[0]:
        raise ValueError('ce: targets must be (B, T) or (B, T, 1) class indices for predictions %s, got %s'
                         % (tuple(predictions.shape), tuple(targets.shape)))
    if targets.shape[1] != predictions.shape[1]:
        raise RuntimeError('The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension 1'
                           % (predictions.shape[1], targets.shape[1]))
    return targets if targets.dtype == torch.int64 else targets.long()


def ce(predictions, targets, seq_len=None, want_argmax=False):
    """Masked categorical cross entropy with the same per-utterance averaging as ``mse`` (reference: losses.py:59-61,
    ``F.cross_entropy(predictions.transpose(1, 2), targets, reduction='none')`` under the wrapper of :29-46).

    predictions (B, T, C) float32 logits - a column slice of a wider tensor is read in place; targets (B, T) or (B, T, 1) integer
    class indices.  A target of -100 (``F.cross_entropy``'s ``ignore_index``) scores 0 and still counts as a valid frame; any other
    target outside [0, C) in a valid frame makes the loss NaN (the reference asserts on the device).  One HIP pass computes the loss
    and d loss / d predictions (csrc/ce.hip; the reference runs a transpose, log_softmax, nll_loss, a host-built mask, mul, two sums,
    div and mean, then their autograd mirrors).  ``want_argmax``: returns (loss, predicted class (B, T) int64 from the same pass; 0 in
    pad frames)."""
    if seq_len is not None and seq_len.dtype != torch.int64:
        seq_len = seq_len.long()
    if not isinstance(predictions, torch.Tensor) or predictions.dim() != 3:
        raise ValueError('ce: predictions must be a (B, T, C) tensor')
    loss, argmax = F_hip.MaskedCEFn.apply(predictions, _class_targets(predictions, targets), seq_len, want_argmax)
    return (loss, argmax) if want_argmax else loss


def mdn_width(n_components, dim):
    """Prediction columns of a mixture-density stream: K logits, K D means, K D log standard deviations."""
    return int(n_components) * (1 + 2 * int(dim))


def _mdn_predictions(what, predictions, n_components, dim):
    if not isinstance(predictions, torch.Tensor) or predictions.dim() != 3:
        raise ValueError('%s: predictions must be a (B, T, K (1 + 2 D)) tensor' % what)
    if predictions.dtype != torch.float32:
        raise TypeError('%s: predictions must be torch.float32, got %s' % (what, predictions.dtype))
    if int(n_components) < 1 or predictions.shape[2] != mdn_width(n_components, dim):
        raise ValueError('%s: predictions %s are not n_components * (1 + 2 D) = %d * (1 + 2 * %d) = %d columns wide'
                         % (what, tuple(predictions.shape), n_components, dim, mdn_width(n_components, dim)))


def mdn(predictions, targets, seq_len=None, n_components=1, min_log_std=None):
    r"""Masked negative log likelihood of a mixture density network's output (Zen & Senior 2014) with the per-utterance averaging of
    ``mse``, in nats per target dimension.  The reference has no such loss.

    predictions (B, T, K (1 + 2 D)) float32, K = ``n_components``: ``[K logits a | K D means mu, component-major | K D log standard
    deviations s]`` - a column slice of a wider tensor is read in place; targets (B, T, D) float32.  Per frame

        z_kd = (y_d - mu_kd) exp(-s_kd),   q_k = log_softmax(a)_k - sum_d (0.5 z_kd^2 + s_kd) - D log sqrt(2 pi),
        l = -logsumexp_k(q_k) / D

    and the loss is ``mean_b( sum_{t < n_b} l[b,t] / n_b )``; ``seq_len[b] == 0`` gives NaN.  ``min_log_std`` puts a floor under s
    (``torch.clamp``'s rule: a floored s gets gradient 0).  Pad frames are not read: a NaN there does not reach the loss.  A -inf
    logit removes its component.  One HIP pass computes the loss and d loss / d predictions (csrc/mdn.hip); composed of torch ops it
    is about 15 launches over (B, T, K, D) temporaries plus their autograd mirrors.  No gradient for the targets, no double backward."""
    if not isinstance(targets, torch.Tensor) or targets.dim() != 3:
        raise ValueError('mdn: targets must be a (B, T, D) tensor')
    _mdn_predictions('mdn', predictions, n_components, targets.shape[2])
    if targets.shape[1] != predictions.shape[1]:
        raise RuntimeError('The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension 1'
                           % (predictions.shape[1], targets.shape[1]))
    if seq_len is not None and seq_len.dtype != torch.int64:
        seq_len = seq_len.long()
    if targets.dtype != torch.float32:
        targets = targets.float()
    return F_hip.MaskedMDNFn.apply(predictions, targets.detach(), seq_len, int(n_components),
                                   None if min_log_std is None else float(min_log_std))


def mdn_select(predictions, n_components, dim, seq_len=None, min_log_std=None):
    """Generation from a mixture-density stream (the layout of ``mdn``, D = ``dim``): per frame the most probable component (the
    lowest index among the largest logits), its means and its variances ``exp(2 max(s, min_log_std))`` - what MLPG takes as per-frame
    means and variances.  Returns (component (B, T) int64, mean (B, T, D), variance (B, T, D)), detached; pad frames hold 0, 0 and 1.
    One launch (csrc/mdn.hip).  ``mdn_sample`` draws a component from the mixture weights instead of taking the largest."""
    _mdn_predictions('mdn_select', predictions, n_components, dim)
    if seq_len is not None and seq_len.dtype != torch.int64:
        seq_len = seq_len.long()
    return ops.mdn_select(predictions.detach(), seq_len, int(n_components), int(dim), min_log_std=min_log_std)


def mdn_sample(predictions, n_components, dim, seq_len=None, min_log_std=None, temperature=1., noise_scale=0.):
    """Sampled generation from a mixture-density stream (the layout of ``mdn``, D = ``dim``): per frame ONE component drawn with
    probability ``softmax(logits / temperature)``, its means and its variances ``exp(2 max(s, min_log_std))`` - what MLPG takes as
    per-frame means and variances, a different rendition on every call where ``mdn_select`` always gives the mode.  Returns
    (component (B, T) int64, mean (B, T, D), variance (B, T, D)), detached; pad frames hold 0, 0 and 1.

    ``temperature`` (a finite Python number > 0): below 1 the draw leans towards the most probable component, above 1 towards the
    uniform one; 0 is refused - that limit is ``mdn_select``.  ``noise_scale`` (>= 0): 0 returns the drawn component's mean as it is;
    otherwise the mean is ``mu + noise_scale * exp(max(s, min_log_std)) * g`` with g ~ N(0, 1) per element (1: a draw from the mixture
    itself).  A -inf logit is never drawn.  One launch (csrc/mdn.hip); the draws are Philox words of (torch's seed, ops.MDN_COMPONENT_SITE
    / ops.MDN_NOISE_SITE, ONE draw of the device's step counter, frame [, element]), so ``torch.manual_seed`` makes a run repeatable
    and a captured graph draws anew on every replay.  No gradient flows through the draw."""
    temperature, noise_scale = ops.mdn_sample_arguments('mdn_sample', temperature, noise_scale)
    _mdn_predictions('mdn_sample', predictions, n_components, dim)
    if seq_len is not None and seq_len.dtype != torch.int64:
        seq_len = seq_len.long()
    predictions = predictions.detach()
    ops.mdn_sample_shape(predictions, n_components, dim)      # the caps, before the step counter moves
    return ops.mdn_sample(predictions, seq_len, int(n_components), int(dim), ops.dropout_seed(), ops.dropout_draw(predictions.device),
                          min_log_std=min_log_std, temperature=temperature, noise_scale=noise_scale)


_HALF_LOG_2PI = 0.9189385332046727


def gaussian_nll(predictions, targets, min_log_std=None):
    """The per-frame, per-dimension term of ``gaussian``: predictions (..., 2 D) = ``[means | log standard deviations]`` against
    targets (..., D) -> ``0.5 ((y - mu) exp(-s'))^2 + s' + 0.5 log(2 pi)`` with ``s' = max(s, min_log_std)``, shaped like the targets.
    Plain torch ops on whatever device and dtype the inputs have; autograd flows through them (a floored s gets gradient 0)."""
    dim = targets.shape[-1]
    if predictions.shape[-1] != 2 * dim:
        raise ValueError('gaussian: predictions %s are not 2 D = 2 * %d columns wide ([means | log standard deviations])'
                         % (tuple(predictions.shape), dim))
    mean, log_std = predictions[..., :dim], predictions[..., dim:]
    if min_log_std is not None:
        log_std = torch.clamp(log_std, min=float(min_log_std))
    z = (targets - mean) * torch.exp(-log_std)
    return 0.5 * (z * z) + log_std + _HALF_LOG_2PI


def gaussian(predictions, targets, seq_len=None, min_log_std=None):
    r"""Masked negative log likelihood of a diagonal Gaussian whose mean AND standard deviation the model predicts per frame (the
    single-Gaussian trajectory model of Hashimoto et al. 2016), with the per-utterance averaging of ``mse``, in nats per dimension:
    the value of ``mdn`` at ``n_components=1``.  The reference has no such loss.

    predictions (B, T, 2 D) float32 ``[means | log standard deviations s]`` - a column slice of a wider tensor is read in place;
    targets (B, T, D) float32.  Per element ``0.5 ((y - mu) exp(-s'))^2 + s' + 0.5 log(2 pi)``, ``s' = max(s, min_log_std)``
    (``torch.clamp``'s rule: a floored s gets gradient 0); the loss is ``mean_{b,d}( sum_{t < n_b} l[b,t,d] / n_b )``.  Built on
    ``sequence_loss``: the per-element term runs as torch ops (``gaussian_nll``), the reduction and its backward on csrc/seqmean.hip -
    and with ``sequence_loss``'s rule for pad frames (every frame is read: a NaN there gives NaN), not ``mdn``'s.  A fused one-pass
    kernel for it is not provided."""
    if not isinstance(predictions, torch.Tensor) or predictions.dim() != 3:
        raise ValueError('gaussian: predictions must be a (B, T, 2 D) tensor')
    if not isinstance(targets, torch.Tensor) or targets.dim() != 3:
        raise ValueError('gaussian: targets must be a (B, T, D) tensor')
    if predictions.dtype != torch.float32:
        raise TypeError('gaussian: predictions must be torch.float32, got %s' % predictions.dtype)
    if predictions.shape[2] != 2 * targets.shape[2]:
        raise ValueError('gaussian: predictions %s are not 2 D = 2 * %d columns wide ([means | log standard deviations])'
                         % (tuple(predictions.shape), targets.shape[2]))
    if targets.shape[1] != predictions.shape[1]:
        raise RuntimeError('The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension 1'
                           % (predictions.shape[1], targets.shape[1]))
    if targets.dtype != torch.float32:
        targets = targets.float()

    def gaussian_feature_loss(p, y):
        return gaussian_nll(p, y, min_log_std)

    return sequence_loss(gaussian_feature_loss)(predictions, targets.detach(), seq_len)


def _gv_seq_len(what, x, seq_len):
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError('%s: a (B, T, D) tensor is wanted, got %s' % (what, tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)))
    if seq_len is not None and seq_len.dtype != torch.int64:
        seq_len = seq_len.long()
    return seq_len


def gv(predictions, targets, seq_len=None, log=True, eps=1e-6):
    r"""Global-variance loss (Toda & Tokuda 2007): the squared gap between the per-utterance variance of a generated trajectory and
    that of the natural one - the usual companion of trajectory training against over-smoothing.  The reference has no such loss.

    predictions and targets (B, T, D) float32 on the device, both read in place whatever their strides (a column slice, a
    transposed view, an expanded operand).  With n_b = ``seq_len[b]`` clamped to [0, T] (T without ``seq_len``):

        m[b,d] = mean_{t < n_b} x[b,t,d],   v[b,d] = mean_{t < n_b} (x[b,t,d] - m[b,d])^2    (biased),
        loss = mean_{b,d} ( f(v_pred[b,d]) - f(v_tgt[b,d]) )^2,    f(v) = log(v + eps) if ``log`` else v.

    Returns a 0-d float32 device tensor, differentiable in ``predictions``; the targets get no gradient.  One utterance of one frame
    has v = 0: the loss is finite and its gradient 0.  ``seq_len[b] == 0`` gives NaN, as for ``mse``.  Pad frames are NOT read, so a
    NaN there changes nothing: this is ``mdn``'s rule, not ``sequence_loss``'s, which multiplies every frame by its mask value.
    Targets of another dtype are refused as ``mse`` refuses them.  The variances are accumulated in float64 from shifted chunks
    merged by Chan's update - no sum of raw squares, so a column far from 0 (a spectral coefficient at 16384 +- 2^-6) keeps its
    variance - in an order that depends on (b, t, d) alone: the same bits on every call and for every layout of the same values.
    Two launches forward, one backward (csrc/gv.hip through ``functional.GVFn``); composed of torch ops it is about a dozen
    launches plus their autograd mirrors.  No CPU fallback, no double backward."""
    seq_len = _gv_seq_len('gv', predictions, seq_len)
    if not isinstance(targets, torch.Tensor) or targets.shape != predictions.shape:
        raise ValueError('gv: targets must be a tensor shaped like the predictions %s, got %s'
                         % (tuple(predictions.shape), tuple(targets.shape) if isinstance(targets, torch.Tensor) else type(targets)))
    return F_hip.GVFn.apply(predictions, targets.detach(), seq_len, bool(log), float(eps))


def global_variance(x, seq_len=None):
    """Per-utterance variance of every column over the valid frames (biased, as ``gv`` defines it): x (B, T, D) float32 on the device
    -> (B, D) float32, detached, from ``gv``'s kernel.  What one plots against the natural features' to see over-smoothing; a
    constant column gives exactly 0, an utterance without a valid frame NaN."""
    seq_len = _gv_seq_len('global_variance', x, seq_len)
    return ops.gv(x.detach(), None, seq_len, want_variances=True)[2]


def multi_stream(predictions, targets, kinds, seq_len=None, want_prob=False, widths=None, want_argmax=False):
    """Mean over streams of ``mse`` / ``bce(sigmoid(.))`` / ``ce`` on column slices of one prediction tensor - the loss of the
    reference's LSTM acoustic model (models/RNN_SPSS.py:120-139: three ``losses.mse`` + one ``losses.bce``, ``/ 4.``) in one
    pass instead of torch.split + four masked losses and their autograd mirrors.

    predictions (B, T, sum of widths); targets[k] (B, T, width_k) in column order; kinds[k] in {'mse', 'sigmoid_bce', 'ce'}.
    Returns (loss, sigmoid(predictions) of the BCE stream if ``want_prob`` else None).

    A 'ce' stream's target holds integer class indices, (B, T) or (B, T, 1), and its width is its number of classes: ``widths[k]``,
    or what the other streams leave of the prediction when there is one 'ce' stream.  Such a table takes the one-pass launch over
    its mse / sigmoid_bce streams plus one categorical launch per 'ce' stream, all writing ONE gradient tensor, the losses summed on
    the device (no host read).  ``want_argmax`` then makes the result (loss, prob, {k: predicted class (B, T) int64 of stream k})."""
    if seq_len is not None and seq_len.dtype != torch.int64:
        seq_len = seq_len.long()
    if 'ce' not in kinds:
        targets = [y if y.dtype == torch.float32 else y.float() for y in targets]
        loss, prob = F_hip.StreamLossFn.apply(predictions, seq_len, tuple(kinds), want_prob, *targets)
        return (loss, prob, {}) if want_argmax else (loss, prob)
    kinds = tuple(kinds)
    if widths is None:
        if kinds.count('ce') != 1:
            raise ValueError("multi_stream: more than one 'ce' stream needs widths (the number of classes of each)")
        rest = sum(int(y.shape[-1]) for y, kind in zip(targets, kinds) if kind != 'ce')
        widths = [predictions.shape[-1] - rest if kind == 'ce' else int(y.shape[-1]) for y, kind in zip(targets, kinds)]
    targets = [_class_targets(predictions, y) if kind == 'ce' else (y if y.dtype == torch.float32 else y.float())
               for y, kind in zip(targets, kinds)]
    out = F_hip.StreamLossCEFn.apply(predictions, seq_len, kinds, tuple(int(w) for w in widths), want_prob, want_argmax, *targets)
    if not want_argmax:
        return out[0], out[1]
    return out[0], out[1], dict(zip([k for k, kind in enumerate(kinds) if kind == 'ce'], out[2:]))


def KLD_standard_normal(mean, log_variance):
    r"""KL divergence of N(``mean``, exp(``log_variance``)) from N(0, I): ``-0.5 sum_z (1 + log_variance - mean^2 - exp(log_variance))``
    averaged over the leading dims (reference losses.py:64-67).  One HIP reduction with a fixed order and its backward
    (csrc/vae.hip); column views of one encoder output are read in place."""
    return F_hip.KLDFn.apply(mean, log_variance)
