"""``morgana/viz/synthesis.py`` against this package: ``MLPG`` with the reference's signature and return conventions, solved on the
device (``csrc/mlpg.hip``) instead of on the host with ``bandmat``.

The reference calls this from ``predict`` of its shipped models (``models/f0_test_model.py:86-89``, ``models/RNN_SPSS.py:107-118``)
on every training step - a device -> host copy, B x D banded float64 solves in a Python loop, a host -> device copy - to feed the
LF0 / MCD metrics of ``loss``.  Here the delta streams never leave the device and nothing synchronises.

``mlpg_trajectory`` is the same solve as a differentiable layer (device tensors only), for losses taken on the trajectory itself.
"""
import numpy as np
import torch

from .. import _lib, functional, ops

DEFAULT_WINDOWS = (                                  # synthesis.py:122-127
    (0, 0, np.array([1.0])),
    (1, 1, np.array([-0.5, 0.0, 0.5])),
    (1, 1, np.array([1.0, -2.0, 1.0])),
)


def _device_of(*values):
    for v in values:                                 # synthesis.py:101-112: the first tensor's device
        if isinstance(v, torch.Tensor):
            return v.device
    return None


def MLPG(means, variances, windows=None, padding_size=0, seq_len=None):
    r"""Performs maximum-likelihood parameter generation (synthesis.py:79-178).

    means : (batch_size, seq_len, feat_dim) or (seq_len, feat_dim); variances : the same shape, or (feat_dim,) global;
    windows : list of (l, u, coefficients), default static / delta / delta-delta; padding_size : frames repeated at either end
    as burn-in; seq_len : (batch_size,) lengths (frames past them come back as zeros).

    Returns the most probable trajectory, (batch_size, seq_len, feat_dim // len(windows)) or without the batch axis for a
    single sequence: a float32 tensor on the inputs' device if any input was a tensor (as the reference), else a float64 array.
    Tensors must live on the MI355X; numpy inputs are uploaded to the current device (float32, the dtype the model emits).
    There is no host implementation: without the HIP library this raises.
    """
    device = _device_of(means, variances, seq_len)
    as_tensor = device is not None
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.MorganaHipError('MLPG runs only on an MI355X device (no CPU fallback)')
        device = torch.device('cuda', torch.cuda.current_device())

    def put(x, dtype):
        if isinstance(x, torch.Tensor):
            return x.detach().to(device=device, dtype=dtype)
        return torch.as_tensor(np.ascontiguousarray(x)).to(device=device, dtype=dtype)

    means = put(means, torch.float32)
    variances = put(variances, torch.float32)
    if windows is None:
        windows = DEFAULT_WINDOWS
    using_batches = means.dim() != 2                  # :129-133
    if not using_batches:
        means = means[None]
        if variances.dim() == 2:
            variances = variances[None]               # :143-144
    if seq_len is not None:
        seq_len = put(seq_len, torch.int64).reshape(-1)
    out = ops.mlpg(means, variances, windows, padding_size=padding_size, seq_len=seq_len,
                   out_dtype=torch.float32 if as_tensor else torch.float64)
    if not using_batches:
        out = out.squeeze(0)                          # :173-174
    return out if as_tensor else out.cpu().numpy()    # :176-178


def MLPG_GV(means, variances, gv_mean, gv_variance, windows=None, padding_size=0, seq_len=None, gv_weight=1., max_iter=48):
    r"""``MLPG`` under a global-variance prior (Toda & Tokuda 2007; ``csrc/mlpg_gv.hip`` - the reference generates with ``MLPG`` only).

    means, variances, windows, padding_size, seq_len and the return conventions are ``MLPG``'s.  gv_mean, gv_variance :
    (feat_dim // len(windows),) mean and variance of the per-utterance variance of the static feature
    (``data.fit_global_variance``), or (batch_size, feat_dim // len(windows)) with one row per utterance (per-speaker statistics);
    gv_weight : the weight of the prior against the per-frame likelihood of ``MLPG`` (0: ``MLPG`` itself); max_iter : the most
    evaluations of the root search, a banded solve each.  An utterance of fewer than two frames, and any system whose search does
    not converge, comes back as ``MLPG`` gives it (``ops.mlpg_gv(..., want_info=True)`` tells which).
    """
    device = _device_of(means, variances, seq_len, gv_mean, gv_variance)
    as_tensor = device is not None
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.MorganaHipError('MLPG_GV runs only on an MI355X device (no CPU fallback)')
        device = torch.device('cuda', torch.cuda.current_device())

    def put(x, dtype):
        if isinstance(x, torch.Tensor):
            return x.detach().to(device=device, dtype=dtype)
        return torch.from_numpy(np.array(x)).to(device=device, dtype=dtype)      # a copy: a read-only array is welcome

    means = put(means, torch.float32)
    variances = put(variances, torch.float32)
    if windows is None:
        windows = DEFAULT_WINDOWS
    using_batches = means.dim() != 2
    if not using_batches:
        means = means[None]
        if variances.dim() == 2:
            variances = variances[None]
    if seq_len is not None:
        seq_len = put(seq_len, torch.int64).reshape(-1)
    if not isinstance(gv_variance, torch.Tensor) and not (np.asarray(gv_variance, np.float64) > 0).all():
        raise ValueError('gv_variance must be positive everywhere')
    out = ops.mlpg_gv(means, variances, put(gv_mean, torch.float32), put(gv_variance, torch.float32), windows,
                      padding_size=padding_size, seq_len=seq_len, gv_weight=gv_weight, max_iter=max_iter,
                      out_dtype=torch.float32 if as_tensor else torch.float64)
    if not using_batches:
        out = out.squeeze(0)
    return out if as_tensor else out.cpu().numpy()


def mlpg_trajectory(means, variances, windows=None, padding_size=0, seq_len=None, variance_grad=False):
    r"""``MLPG`` as a differentiable layer (trajectory / minimum-generation-error training; the reference's host MLPG has no gradient).

    means : (batch_size, seq_len, feat_dim) float32 device tensor; variances : (feat_dim,) global, the same shape as ``means`` or
    (batch_size, feat_dim) per item, float32 on the same device - constants: one that requires grad is a ValueError; windows,
    padding_size, seq_len as for ``MLPG``.  Device tensors only, always batched.
    variance_grad : True makes the variances a trained input as well (a stream that predicts its variance): they must be per frame,
    the same shape as ``means`` - expand a global or per-item table, autograd sums the expansion - and the backward returns both
    gradients from one pair of side-by-side solves (``functional.MLPGVarFn``).  The forward is the same launch either way.

    Returns the most probable trajectory (batch_size, seq_len, feat_dim // len(windows)), float32, zero past ``seq_len``, with a
    gradient for ``means``: one more banded solve with the forward's matrix and a window pass (``csrc/mlpg.hip``).
    """
    for name, value in (('means', means), ('variances', variances)):
        if not isinstance(value, torch.Tensor):
            raise TypeError('mlpg_trajectory takes device tensors; %s is %s (MLPG takes arrays)' % (name, type(value)))
    if variances.requires_grad and not variance_grad:
        raise ValueError('mlpg_trajectory has no gradient for its variances (they are normaliser constants): detach them, or pass '
                         'variance_grad=True with per-frame variances to train them')
    if variance_grad and variances.shape != means.shape:
        raise ValueError('mlpg_trajectory(variance_grad=True) takes per-frame variances shaped like the means %s, got %s: expand them to '
                         '(B, T, W*D) so that autograd sums the expansion' % (tuple(means.shape), tuple(variances.shape)))
    if windows is None:
        windows = DEFAULT_WINDOWS
    if seq_len is not None:
        if not isinstance(seq_len, torch.Tensor):
            raise TypeError('mlpg_trajectory takes device tensors; seq_len is %s' % type(seq_len))
        seq_len = seq_len.reshape(-1).to(device=means.device, dtype=torch.int64)
    if variance_grad:
        return functional.MLPGVarFn.apply(means, variances, windows, padding_size, seq_len)
    return functional.MLPGFn.apply(means, variances, windows, padding_size, seq_len)
