#!/usr/bin/env python
"""Generate tests/golden/g18_ce.npz by RUNNING THE REFERENCE'S ``losses.ce`` and its autograd in fp32 on the CPU (build container only).

Usage (from the repo root, in the container that has the reference checkout ``make_golden.py`` imports):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ce.py

Nothing of the reference's source is written anywhere: the .npz holds inputs, targets, sequence lengths and the numbers the
reference computed.

Contents: ``cases`` (the case names) and per case ``<case>__pred`` (B, T, C) float32, ``<case>__target`` (B, T) int64,
``<case>__seq_len`` (B,) int64 (absent when the case passes ``seq_len=None``), ``<case>__loss`` () float32 and ``<case>__grad``
(B, T, C) float32 = d loss / d predictions.

  ragged     B=3, T=7, C=5, seq_len=[7, 4, 1]
  full       the same inputs, seq_len=None
  c2         C=2
  c65        C=65 (one class more than a wave has lanes)
  ignore     ragged with targets of -100 (F.cross_entropy's default ignore_index) in valid frames
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
    _, losses, _, _, _, _ = import_reference()
    torch.set_num_threads(1)
    rng = np.random.RandomState(20261017)
    b, t = 3, 7
    seq_len = np.array([7, 4, 1], dtype=np.int64)

    def inputs(c):
        return (rng.standard_normal((b, t, c)) * 2.0).astype(np.float32), rng.randint(0, c, size=(b, t)).astype(np.int64)

    pred5, target5 = inputs(5)
    ignore = target5.copy()
    ignore[0, 2] = ignore[1, 0] = ignore[1, 3] = -100        # valid frames of utterances 0 and 1
    ignore[2, 5] = -100                                      # and one pad frame
    cases = {'ragged': (pred5, target5, seq_len), 'full': (pred5, target5, None), 'c2': inputs(2) + (seq_len,),
             'c65': inputs(65) + (seq_len,), 'ignore': (pred5, ignore, seq_len)}
    out = {'cases': np.array(sorted(cases))}
    for name, (pred, target, n) in cases.items():
        x = torch.from_numpy(pred.copy()).requires_grad_(True)
        loss = losses.ce(x, torch.from_numpy(target.copy()), None if n is None else torch.from_numpy(n.copy()))
        loss.backward()
        out[name + '__pred'], out[name + '__target'] = pred, target
        if n is not None:
            out[name + '__seq_len'] = n
        out[name + '__loss'] = loss.detach().numpy().astype(np.float32)
        out[name + '__grad'] = x.grad.numpy().astype(np.float32)
        assert np.isfinite(out[name + '__loss']) and np.isfinite(out[name + '__grad']).all(), name
    path = os.path.join(HERE, 'g18_ce.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes, %d arrays)' % (path, os.path.getsize(path), len(out)))


if __name__ == '__main__':
    main()
