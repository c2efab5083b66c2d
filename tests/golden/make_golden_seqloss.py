#!/usr/bin/env python
"""Generate tests/golden/g20_sequence_loss.npz by RUNNING THE REFERENCE'S ``losses.sequence_loss`` and its autograd in fp32 on the CPU
(build container only).

Usage (from the repo root, in the container that has the reference checkout ``make_golden.py`` imports):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_seqloss.py

Nothing of the reference's source is written anywhere: the .npz holds inputs, sequence lengths and the numbers the reference
computed.  The loss functions that are wrapped are the ones named below, written here.

Contents: ``cases`` (the case names) and per case ``<case>__pred`` (B, T, P) float32, ``<case>__target`` (B, T, D) float32,
``<case>__seq_len`` (B,) int64 (absent when the case passes ``seq_len=None``), ``<case>__feature_loss`` (B, T, D) float32 (what the
wrapped function returned), ``<case>__loss`` () float32, ``<case>__grad_feature`` (B, T, D) float32 = d loss / d feature_loss and
``<case>__grad_pred`` (B, T, P) float32 = d loss / d predictions.

  l1_ragged  F.l1_loss,                                  B=3, T=7, D=5, seq_len=[7, 4, 1]
  l1_full    the same inputs, seq_len=None
  l1_d1      F.l1_loss, D=1
  l1_long    F.l1_loss,                                  B=2, T=70, D=33, seq_len=[70, 13]
  huber      F.smooth_l1_loss,                           B=3, T=7, D=5, seq_len=[7, 4, 1]
  nll        0.5 (logvar + (y - mu)^2 exp(-logvar)) on predictions of 10 columns (mu | logvar), feature loss of 5
  signed     p - y (the summands cancel),                B=3, T=7, D=5, seq_len=[7, 4, 1]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import import_reference  # noqa: E402


def main():
    import torch
    import torch.nn.functional as F
    _, losses, _, _, _, _ = import_reference()
    torch.set_num_threads(1)
    rng = np.random.RandomState(20261019)
    seq_len = np.array([7, 4, 1], dtype=np.int64)

    def inputs(b, t, p, d):
        return (rng.standard_normal((b, t, p)) * 1.5).astype(np.float32), (rng.standard_normal((b, t, d)) * 1.5).astype(np.float32)

    def l1(predictions, targets):
        return F.l1_loss(predictions, targets, reduction='none')

    def huber(predictions, targets):
        return F.smooth_l1_loss(predictions, targets, reduction='none')

    def nll(predictions, targets):
        mu, logvar = predictions[:, :, :5], predictions[:, :, 5:]
        return 0.5 * (logvar + (targets - mu) ** 2 * torch.exp(-logvar))

    def signed(predictions, targets):
        return predictions - targets

    pred5, target5 = inputs(3, 7, 5, 5)
    cases = {'l1_ragged': (l1, pred5, target5, seq_len), 'l1_full': (l1, pred5, target5, None),
             'l1_d1': (l1,) + inputs(3, 7, 1, 1) + (seq_len,),
             'l1_long': (l1,) + inputs(2, 70, 33, 33) + (np.array([70, 13], dtype=np.int64),),
             'huber': (huber,) + inputs(3, 7, 5, 5) + (seq_len,),
             'nll': (nll,) + inputs(3, 7, 10, 5) + (seq_len,),
             'signed': (signed,) + inputs(3, 7, 5, 5) + (seq_len,)}
    out = {'cases': np.array(sorted(cases))}
    for name, (loss_fn, pred, target, n) in cases.items():
        kept = {}

        def keeping(predictions, targets, loss_fn=loss_fn, kept=kept):
            kept['feature_loss'] = loss_fn(predictions, targets)
            kept['feature_loss'].retain_grad()
            return kept['feature_loss']

        x = torch.from_numpy(pred.copy()).requires_grad_(True)
        loss = losses.sequence_loss(keeping)(x, torch.from_numpy(target.copy()), None if n is None else torch.from_numpy(n.copy()))
        loss.backward()
        out[name + '__pred'], out[name + '__target'] = pred, target
        if n is not None:
            out[name + '__seq_len'] = n
        out[name + '__feature_loss'] = kept['feature_loss'].detach().numpy().astype(np.float32)
        out[name + '__loss'] = loss.detach().numpy().astype(np.float32)
        out[name + '__grad_feature'] = kept['feature_loss'].grad.numpy().astype(np.float32)
        out[name + '__grad_pred'] = x.grad.numpy().astype(np.float32)
        for key in ('loss', 'grad_feature', 'grad_pred'):
            assert np.isfinite(out[name + '__' + key]).all(), (name, key)
    path = os.path.join(HERE, 'g20_sequence_loss.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes, %d arrays)' % (path, os.path.getsize(path), len(out)))


if __name__ == '__main__':
    main()
