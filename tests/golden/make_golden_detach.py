#!/usr/bin/env python
"""Generate tests/golden/g19_detach.npz by RUNNING THE REFERENCE'S ``utils.detach_batched_seqs``, ``batched_masked_select``,
``both_voiced_mask``, ``listify``, ``map_nested`` and ``get_epoch_from_checkpoint_path`` on the CPU (build container only).

Usage (from the repo root, in the container that has the reference checkout ``make_golden.py`` imports):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_detach.py

Nothing of the reference's source is written anywhere: the .npz holds what the reference returned for the inputs that
tests/detach_ref.py builds (B=4, T=7, seq_len=[7, 4, 1, 0]; widths 1, 3, 5; float32, bool, int64).

Contents
  detach__<case>__unwrapped          1 when the call returned the single feature's value itself, 0 for a list of features
  detach__<case>__<k>__whole         feature k came back as one array (items with ndim <= 1, or seq_len=None)
  detach__<case>__<k>__<b>           item b of feature k (shape as returned: np.squeeze of a length-1 item is 0-d or (D,))
  select__<feature>                  batched_masked_select(feature, seq_len)
  voiced__<case>__<dtype>            both_voiced_mask(*features, dtype=...)
  epochs                             get_epoch_from_checkpoint_path of detach_ref.CHECKPOINT_PATHS
  listify_json, map_nested_json      detach_ref.encode of the results for detach_ref.LISTIFY_INPUTS / nested_input() under double()
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

from make_golden import import_reference  # noqa: E402
import detach_ref  # noqa: E402


def main():
    import torch
    utils = import_reference()[0]
    torch.set_num_threads(1)
    x = detach_ref.detach_inputs()
    out = {}
    for case, (names, kind, squeeze) in detach_ref.DETACH_CASES.items():
        seq_len = {'tensor': torch.from_numpy(detach_ref.SEQ_LEN.copy()), 'numpy': detach_ref.SEQ_LEN.copy(), 'none': None}[kind]
        feats = [torch.from_numpy(x[n].copy()).requires_grad_(x[n].dtype == np.float32) for n in names]
        got = utils.detach_batched_seqs(*feats, seq_len=seq_len, squeeze=squeeze)
        out['detach__%s__unwrapped' % case] = np.array(int(len(names) == 1))
        for k, value in enumerate([got] if len(names) == 1 else got):
            if isinstance(value, np.ndarray):
                out['detach__%s__%d__whole' % (case, k)] = value
            else:
                assert len(value) == detach_ref.B
                for b, item in enumerate(value):
                    out['detach__%s__%d__%d' % (case, k, b)] = np.asarray(item)
    seq_len = torch.from_numpy(detach_ref.SEQ_LEN.copy())
    for name in detach_ref.SELECT_CASES:
        out['select__' + name] = utils.batched_masked_select(torch.from_numpy(x[name].copy()), seq_len).numpy()
    torch_dtypes = {'uint8': torch.ByteTensor, 'bool': torch.bool, 'float32': torch.float32}
    for case, names in detach_ref.VOICED_CASES.items():
        for dtype in detach_ref.VOICED_DTYPES:
            got = utils.both_voiced_mask(*[torch.from_numpy(x[n].copy()) for n in names], dtype=torch_dtypes[dtype])
            out['voiced__%s__%s' % (case, dtype)] = got.numpy()
    out['epochs'] = np.array([utils.get_epoch_from_checkpoint_path(p) for p in detach_ref.CHECKPOINT_PATHS], dtype=np.int64)
    out['listify_json'] = np.array(json.dumps([detach_ref.encode(utils.listify(v)) for v in detach_ref.LISTIFY_INPUTS]))
    out['map_nested_json'] = np.array(json.dumps(detach_ref.encode(utils.map_nested(detach_ref.double, detach_ref.nested_input()))))
    path = os.path.join(HERE, 'g19_detach.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes, %d arrays)' % (path, os.path.getsize(path), len(out)))


if __name__ == '__main__':
    main()
