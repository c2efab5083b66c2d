#!/usr/bin/env python
"""Generate tests/golden/g17_speaker_normalisers.npz by RUNNING THE REFERENCE'S speaker-dependent normalisers (build container only).

Usage (from the repo root, in the container that has the reference checkout ``make_golden.py`` imports):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_speakers.py

The reference is imported with the stand-ins of ``make_golden.import_reference`` (its ``get_file_ids`` is one of them, so
``speaker_ids`` is set on the classes directly; ``load_json`` is pointed at the json module so that ``load_params`` reads the files
this script writes to a temporary directory).  Nothing of the reference's source is written anywhere: the .npz holds parameters,
inputs, speaker lists and the outputs the reference computed.

Contents (kind in {mvn, minmax}, group in {static, deltas}):
  speakers                      the speaker list (three names), batch_speakers the batch's names (one repeated), single_speaker one name
  <kind>__<group>__p0 / __p1    (S, D) parameter tables in ``speakers`` order (mean / std_dev, mmin / mmax); one std_dev == 0 column
                                and one mmax == mmin column
  x__<group>                    (B, T, D) float32 input;  x_single__<group>  (T, D)
  <kind>__<group>__torch_norm / torch_denorm      reference on torch tensors, batched (B names)
  <kind>__<group>__numpy_norm / numpy_denorm      reference on NumPy arrays, batched (the reference's functions over its own (B, D)
                                                  parameters; its classes' NumPy path takes one speaker at a time)
  <kind>__<group>__single_norm / single_denorm    reference on one (T, D) NumPy array with one name
  <kind>__<group>__fetch_single / fetch_batch     fetch_params(...)[first parameter]: (D,) and (B, D)
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import import_reference  # noqa: E402

SPEAKERS = ['p1', 'p2', 'p3']
BATCH = ['p2', 'p1', 'p3', 'p2']
SINGLE = 'p3'
KINDS = {'mvn': ('mean', 'std_dev', '{name}_mvn.json'), 'minmax': ('mmin', 'mmax', '{name}_minmax.json')}


def main():
    import torch
    _, _, data, _, _, _ = import_reference()
    sys.modules['tts_data_tools.file_io'].load_json = lambda path: json.load(open(path))
    classes = {'mvn': data.SpeakerDependentMeanVarianceNormaliser, 'minmax': data.SpeakerDependentMinMaxNormaliser}
    functions = {'mvn': (data.normalise_mvn, data.denormalise_mvn), 'minmax': (data.normalise_minmax, data.denormalise_minmax)}
    rng = np.random.RandomState(20261016)
    dims = {'static': 3, 'deltas': 9}
    out = {'speakers': np.array(SPEAKERS), 'batch_speakers': np.array(BATCH), 'single_speaker': np.array(SINGLE)}
    inputs = {}
    for group, d in dims.items():
        inputs[group] = (rng.standard_normal((len(BATCH), 7, d)) * 2.0 + 1.0).astype(np.float32)
        out['x__' + group] = inputs[group]
        out['x_single__' + group] = inputs[group][2, :5].copy()
    with tempfile.TemporaryDirectory() as root:
        tables = {}
        for kind, (n0, n1, pattern) in KINDS.items():
            for group, d in dims.items():
                p0 = rng.standard_normal((len(SPEAKERS), d)).astype(np.float32)
                p1 = rng.uniform(0.2, 1.5, (len(SPEAKERS), d)).astype(np.float32)
                if kind == 'minmax':
                    p1 = p0 + p1
                    p1[1, 1] = p0[1, 1]                      # mmax == mmin for one speaker's column
                else:
                    p1[1, 1] = 0.0                           # std_dev == 0
                tables[kind, group] = (p0, p1)
                out['%s__%s__p0' % (kind, group)], out['%s__%s__p1' % (kind, group)] = p0, p1
                for row, speaker in enumerate(SPEAKERS):
                    os.makedirs(os.path.join(root, 'norm', speaker), exist_ok=True)
                    name = 'feat' + ('_deltas' if group == 'deltas' else '')
                    with open(os.path.join(root, 'norm', speaker, pattern.format(name=name)), 'w') as f:
                        json.dump({n0: p0[row].tolist(), n1: p1[row].tolist()}, f)
        for kind, (n0, n1, _) in KINDS.items():
            normaliser = classes[kind]('feat', 'unused_speaker_id_list', use_deltas=True)
            normaliser.speaker_ids = list(SPEAKERS)
            normaliser.load_params('norm', data_root=root)
            norm_fn, denorm_fn = functions[kind]
            for group in dims:
                deltas = group == 'deltas'
                key = '%s__%s__' % (kind, group)
                x = inputs[group]
                out[key + 'torch_norm'] = normaliser.normalise(torch.from_numpy(x.copy()), list(BATCH), deltas=deltas).numpy()
                out[key + 'torch_denorm'] = normaliser.denormalise(torch.from_numpy(x.copy()), list(BATCH), deltas=deltas).numpy()
                batch_params = normaliser.fetch_params(list(BATCH), torch.Tensor, deltas=deltas)
                as_numpy = {n: v.numpy().copy() for n, v in batch_params.items()}
                out[key + 'numpy_norm'] = norm_fn(x.copy(), as_numpy[n0].copy(), as_numpy[n1].copy())
                out[key + 'numpy_denorm'] = denorm_fn(x.copy(), as_numpy[n0].copy(), as_numpy[n1].copy())
                single = out['x_single__' + group]
                out[key + 'single_norm'] = normaliser.normalise(single.copy(), SINGLE, deltas=deltas)
                out[key + 'single_denorm'] = normaliser.denormalise(single.copy(), SINGLE, deltas=deltas)
                out[key + 'fetch_single'] = normaliser.fetch_params(SINGLE, np.ndarray, deltas=deltas)[n0]
                out[key + 'fetch_batch'] = as_numpy[n0]
                assert out[key + 'fetch_single'].shape == (dims[group],) and out[key + 'fetch_batch'].shape == (len(BATCH), dims[group])
                try:
                    normaliser.fetch_params('nobody', np.ndarray, deltas=deltas)
                    raise AssertionError('the reference accepted an unknown speaker')
                except KeyError:
                    pass
    path = os.path.join(HERE, 'g17_speaker_normalisers.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes, %d arrays)' % (path, os.path.getsize(path), len(out)))


if __name__ == '__main__':
    main()
