"""Speaker-dependent normalisers, host side (no GPU): the NumPy path against what the reference's classes computed
(tests/golden/g17_speaker_normalisers.npz, written by tests/golden/make_golden_speakers.py), the parameter plumbing, ``FilesDataset``
with a ``speaker_id`` data source, the argument checks of the new C entry points, and that a model built WITHOUT ``speaker_id_list`` is
what it was."""
import json
import os

import numpy as np
import pytest
import torch

from morgana_amd import _lib, data, models, ops, synthetic

KINDS = {'mvn': (data.SpeakerDependentMeanVarianceNormaliser, 'mean', 'std_dev', '{name}_mvn.json'),
         'minmax': (data.SpeakerDependentMinMaxNormaliser, 'mmin', 'mmax', '{name}_minmax.json')}
TOL = dict(rtol=1e-6, atol=1e-7)          # the shared normalisers' tolerance (tests/test_gpu_parity.py): same arithmetic per element


def _names(g, key):
    return [str(s) for s in np.atleast_1d(g[key])]


def _normaliser(g, kind, device='cpu', use_deltas=True):
    cls, n0, n1, _ = KINDS[kind]
    speakers = _names(g, 'speakers')
    groups = {}
    for group in ('static', 'deltas'):
        p0, p1 = g['%s__%s__p0' % (kind, group)], g['%s__%s__p1' % (kind, group)]
        groups[group] = {spk: {n0: p0[row], n1: p1[row]} for row, spk in enumerate(speakers)}
    normaliser = cls('feat', 'speakers.scp', use_deltas=use_deltas)
    return normaliser.set_params(groups['static'], groups['deltas'], device=device)


@pytest.mark.parametrize('kind', ['mvn', 'minmax'])
@pytest.mark.parametrize('group', ['static', 'deltas'])
def test_numpy_path_equals_the_reference(golden, kind, group):
    g = golden('g17_speaker_normalisers.npz')
    normaliser, deltas, key = _normaliser(g, kind), group == 'deltas', '%s__%s__' % (kind, group)
    batch, single = _names(g, 'batch_speakers'), _names(g, 'single_speaker')[0]
    assert len(set(batch)) < len(batch) and len(_names(g, 'speakers')) >= 3            # a speaker is repeated in the batch
    x, x1 = g['x__' + group], g['x_single__' + group]
    np.testing.assert_allclose(normaliser.normalise(x, batch, deltas=deltas), g[key + 'numpy_norm'], **TOL)
    np.testing.assert_allclose(normaliser.denormalise(x, batch, deltas=deltas), g[key + 'numpy_denorm'], **TOL)
    np.testing.assert_allclose(normaliser.normalise(x, batch, deltas=deltas), g[key + 'torch_norm'], **TOL)
    np.testing.assert_allclose(normaliser.denormalise(x, batch, deltas=deltas), g[key + 'torch_denorm'], **TOL)
    np.testing.assert_allclose(normaliser.normalise(x1, single, deltas=deltas), g[key + 'single_norm'], **TOL)
    np.testing.assert_allclose(normaliser.denormalise(x1, single, deltas=deltas), g[key + 'single_denorm'], **TOL)
    np.testing.assert_allclose(normaliser.normalise(x1, [single], deltas=deltas), g[key + 'single_norm'], **TOL)
    # an integer index (rows of speaker_ids) names the same speakers
    rows = np.array(normaliser.speaker_rows(batch))
    assert np.array_equal(normaliser.normalise(x, rows, deltas=deltas), normaliser.normalise(x, batch, deltas=deltas))


@pytest.mark.parametrize('kind', ['mvn', 'minmax'])
def test_fetch_params_shapes_and_unknown_speaker(golden, kind):
    g = golden('g17_speaker_normalisers.npz')
    normaliser = _normaliser(g, kind)
    n0, n1 = KINDS[kind][1:3]
    batch, single = _names(g, 'batch_speakers'), _names(g, 'single_speaker')[0]
    for group, deltas in (('static', False), ('deltas', True)):
        key = '%s__%s__' % (kind, group)
        one = normaliser.fetch_params(single, deltas=deltas)
        many = normaliser.fetch_params(batch, np.ndarray, deltas=deltas)
        assert set(one) == {n0, n1} and one[n0].shape == g[key + 'fetch_single'].shape and one[n0].ndim == 1
        assert many[n0].shape == g[key + 'fetch_batch'].shape == (len(batch), one[n0].shape[0])
        assert np.array_equal(one[n0], g[key + 'fetch_single']) and np.array_equal(many[n0], g[key + 'fetch_batch'])
        as_torch = normaliser.fetch_params(batch, torch.Tensor, deltas=deltas)
        assert isinstance(as_torch[n1], torch.Tensor) and tuple(as_torch[n1].shape) == many[n1].shape
    with pytest.raises(KeyError):
        normaliser.fetch_params('nobody')
    with pytest.raises(KeyError):
        normaliser.normalise(g['x__static'], ['p1', 'nobody', 'p2', 'p3'])
    assert sorted(normaliser.params) == sorted(normaliser.params_torch) == sorted(_names(g, 'speakers'))
    assert set(normaliser.delta_params[single]) == {n0, n1} and isinstance(normaliser.delta_params_torch[single][n0], torch.Tensor)
    assert normaliser.speaker_ids == _names(g, 'speakers')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        normaliser.normalise(torch.zeros(4, 7, 3), batch)


def _write_tree(g, root, kind):
    _, n0, n1, pattern = KINDS[kind]
    speakers = _names(g, 'speakers')
    for group in ('static', 'deltas'):
        p0, p1 = g['%s__%s__p0' % (kind, group)], g['%s__%s__p1' % (kind, group)]
        for row, spk in enumerate(speakers):
            os.makedirs(os.path.join(root, 'norm', spk), exist_ok=True)
            name = 'feat' + ('_deltas' if group == 'deltas' else '')
            with open(os.path.join(root, 'norm', spk, pattern.format(name=name)), 'w') as f:
                json.dump({n0: p0[row].tolist(), n1: p1[row].tolist()}, f)
    with open(os.path.join(root, 'speakers.scp'), 'w') as f:
        f.write('\n'.join(speakers) + '\n\n')
    return speakers


@pytest.mark.parametrize('kind', ['mvn', 'minmax'])
def test_load_params_reads_one_directory_per_speaker(golden, tmp_path, kind):
    g = golden('g17_speaker_normalisers.npz')
    speakers = _write_tree(g, str(tmp_path), kind)
    cls, n0, n1, _ = KINDS[kind]
    normaliser = cls('feat', 'speakers.scp', use_deltas=True)
    assert normaliser.speaker_ids is None and normaliser.params == {}
    normaliser.load_params('norm', data_root=str(tmp_path))
    assert normaliser.speaker_ids == speakers
    for row, spk in enumerate(speakers):
        assert np.array_equal(normaliser.params[spk][n1], g['%s__static__p1' % kind][row])
        assert np.array_equal(normaliser.delta_params[spk][n0], g['%s__deltas__p0' % kind][row])
    np.testing.assert_allclose(normaliser.normalise(g['x__deltas'], _names(g, 'batch_speakers'), deltas=True),
                               g['%s__deltas__numpy_norm' % kind], **TOL)
    # the builder's container: as in the reference it hands load_params the joined directory only, so the speaker list is an
    # absolute path (or relative to the working directory)
    both = data.Normalisers({'feat': cls('feat', str(tmp_path / 'speakers.scp'))}, 'norm', data_root=str(tmp_path))
    assert both['feat'].speaker_ids == speakers and both['feat'].delta_params is None
    p0, p1 = both['feat'].tables('cpu')
    assert tuple(p0.shape) == g['%s__static__p0' % kind].shape and np.array_equal(p1.numpy(), g['%s__static__p1' % kind])


def test_files_dataset_with_speaker_ids(golden, tmp_path):
    g = golden('g17_speaker_normalisers.npz')
    root = str(tmp_path)
    _write_tree(g, root, 'mvn')
    single = _names(g, 'single_speaker')[0]
    for name, value in (('feat', g['x_single__static']), ('feat_deltas', g['x_single__deltas'])):
        os.makedirs(os.path.join(root, 'train', name))
        np.save(os.path.join(root, 'train', name, 'utt1.npy'), value)
    os.makedirs(os.path.join(root, 'train', 'speaker_id'))
    with open(os.path.join(root, 'train', 'speaker_id', 'utt1.txt'), 'w') as f:
        f.write(single + '\n')
    with open(os.path.join(root, 'ids.scp'), 'w') as f:
        f.write('utt1\n')
    normalisers = data.Normalisers({'feat': data.SpeakerDependentMeanVarianceNormaliser(
        'feat', os.path.join(root, 'speakers.scp'), use_deltas=True)}, 'norm', data_root=root)
    sources = {'feat': data.NumpyBinarySource('feat', use_deltas=True), 'speaker_id': data.StringSource('speaker_id')}
    with pytest.raises(KeyError, match='speaker-dependent'):
        data.FilesDataset({'feat': sources['feat']}, 'train', 'ids.scp', normalisers, data_root=root)
    dataset = data.FilesDataset(sources, 'train', 'ids.scp', normalisers, data_root=root)
    item = dataset[0]
    assert item['speaker_id'] == single and item['name'] == 'utt1' and 'normalised_speaker_id' not in item
    assert item['normalised_feat'].dtype == np.float32 and item['normalised_feat_deltas'].dtype == np.float32
    np.testing.assert_allclose(item['normalised_feat'], g['mvn__static__single_norm'], **TOL)
    np.testing.assert_allclose(item['normalised_feat_deltas'], g['mvn__deltas__single_norm'], **TOL)
    assert 'normalised_feat' not in dataset.raw(0) and dataset.raw(0)['speaker_id'] == single
    batch = data.to_device(data.collate_fn([item, item]), 'cpu', normalisers=normalisers)
    assert batch['speaker_id'] == [single, single]
    index = batch['speaker_index']
    assert index.dtype == torch.int32 and index.tolist() == [normalisers['feat'].speaker_ids.index(single)] * 2


def test_one_speaker_order_per_normaliser_dict(golden):
    g = golden('g17_speaker_normalisers.npz')
    a, b = _normaliser(g, 'mvn'), _normaliser(g, 'minmax')
    assert data._speaker_order({'a': a, 'b': b, 'c': data.MinMaxNormaliser('c')}) == _names(g, 'speakers')
    assert data._speaker_order({'c': data.MinMaxNormaliser('c')}) is None
    b.speaker_ids = list(reversed(b.speaker_ids))
    utterance = {'name': 'u', 'speaker_id': 'p1', 'a': g['x_single__static'], 'b': g['x_single__static']}
    with pytest.raises(ValueError, match='order'):
        data.collate_to_device([utterance], {'a': a, 'b': b}, 'cpu')
    with pytest.raises(KeyError, match='speaker_id'):
        data.collate_to_device([{'name': 'u', 'a': g['x_single__static']}], {'a': a}, 'cpu')


def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    ok = 4096                                            # any non-null address: every call below is refused before a launch
    cases = {
        'mg_normalise_items_f32': [
            lambda: lib.mg_normalise_items_f32(None, ok, ok, ok, ok, 4, 7, 3, 2, ops.NORM_MVN, 0, None),
            lambda: lib.mg_normalise_items_f32(ok, ok, ok, ok, None, 4, 7, 3, 2, ops.NORM_MVN, 0, None),
            lambda: lib.mg_normalise_items_f32(ok, ok, ok, ok, ok, 4, 7, 3, 0, ops.NORM_MVN, 0, None),          # S <= 0
            lambda: lib.mg_normalise_items_f32(ok, ok, ok, ok, ok, 4, 7, 3, -1, ops.NORM_MVN, 0, None),
            lambda: lib.mg_normalise_items_f32(ok, ok, ok, ok, ok, 4, 7, 0, 2, ops.NORM_MVN, 0, None),          # D <= 0
            lambda: lib.mg_normalise_items_f32(ok, ok, ok, ok, ok, 4, 7, 3, 2, 4, 0, None),                     # unknown kind
            lambda: lib.mg_normalise_items_f32(ok, ok, ok, ok, ok, 4, 7, 3, 2, -1, 1, None),
            lambda: lib.mg_normalise_items_f32(ok, ok, ok, ok, ok, 0, 7, 3, 2, ops.NORM_MVN, 0, None),          # B <= 0
        ],
        'mg_pad_normalise_items_f32': [
            lambda: lib.mg_pad_normalise_items_f32(None, ok, 4, 7, 3, ok, ok, ok, 2, ops.NORM_MVN, ok, ok, None),
            lambda: lib.mg_pad_normalise_items_f32(ok, ok, 4, 7, 3, ok, ok, ok, 2, ops.NORM_MVN, ok, None, None),
            lambda: lib.mg_pad_normalise_items_f32(ok, ok, 4, 7, 3, ok, ok, None, 2, ops.NORM_MVN, ok, ok, None),
            lambda: lib.mg_pad_normalise_items_f32(ok, ok, 4, 7, 3, ok, ok, ok, 0, ops.NORM_MVN, ok, ok, None),     # S <= 0
            lambda: lib.mg_pad_normalise_items_f32(ok, ok, 4, 7, 0, ok, ok, ok, 2, ops.NORM_MVN, ok, ok, None),     # D <= 0
            lambda: lib.mg_pad_normalise_items_f32(ok, ok, 4, 7, 3, ok, ok, ok, 2, ops.DENORM_MVN, ok, ok, None),   # not a forward kind
            lambda: lib.mg_pad_normalise_items_f32(ok, ok, 4, 7, 3, ok, ok, ok, 2, 9, ok, ok, None),
        ],
        'mg_item_rows_f32': [
            lambda: lib.mg_item_rows_f32(None, 2, 3, ok, 4, ok, None),
            lambda: lib.mg_item_rows_f32(ok, 0, 3, ok, 4, ok, None),
            lambda: lib.mg_item_rows_f32(ok, 2, 0, ok, 4, ok, None),
        ],
    }
    for name, calls in cases.items():
        for i, call in enumerate(calls):
            assert call() == -1 and name in _lib.last_error(), (name, i, _lib.last_error())
    with pytest.raises(ValueError):
        _lib.check(-1, 'mg_normalise_items_f32')
    # nothing to do: no launch, no error
    assert lib.mg_normalise_items_f32(ok, ok, ok, ok, ok, 4, 0, 3, 2, ops.NORM_MVN, 0, None) == 0
    assert lib.mg_pad_normalise_items_f32(ok, ok, 4, 0, 3, ok, ok, ok, 2, ops.NORM_MVN, ok, ok, None) == 0
    # the tensor-level wrappers: no CPU fallback
    x, table, rows = torch.zeros(4, 7, 3), torch.zeros(2, 3), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(_lib.MorganaHipError):
        ops.normalise_items(x, table, table, rows, ops.NORM_MVN)
    with pytest.raises(_lib.MorganaHipError):
        ops.item_rows(table, rows)


def test_models_without_a_speaker_list_are_unchanged():
    model = models.GRUF0Model()
    assert model.speaker_id_list is None
    assert {k: type(v) for k, v in model.normaliser_sources().items()} == {
        'dur': data.MeanVarianceNormaliser, 'lab': data.MinMaxNormaliser, 'counters': data.MinMaxNormaliser,
        'lf0': data.MeanVarianceNormaliser}
    assert sorted(model.state_dict()) == sorted(synthetic.gru_f0_state())
    with_speakers = models.GRUF0Model(speaker_id_list='speakers.scp')
    assert sorted(with_speakers.state_dict()) == sorted(model.state_dict())
    sources = with_speakers.normaliser_sources()
    assert type(sources['lf0']) is data.SpeakerDependentMeanVarianceNormaliser and sources['lf0'].use_deltas
    assert sources['lf0'].speaker_id_list == 'speakers.scp' and type(sources['lab']) is data.MinMaxNormaliser
    acoustic = models.LSTMAcousticModel(num_layers=1, speaker_id_list='speakers.scp').normaliser_sources()
    assert all(type(acoustic[n]) is data.SpeakerDependentMeanVarianceNormaliser for n in ('lf0', 'mcep', 'bap'))
    assert type(models.VAEF0Model(speaker_id_list='s').normaliser_sources()['lf0']) is data.SpeakerDependentMeanVarianceNormaliser
    # synthetic per-speaker parameters: one order on every normaliser, delta tables as wide as the stream
    normalisers = synthetic.speaker_acoustic_normalisers(with_speakers, n_speakers=5)
    assert normalisers['lf0'].speaker_ids == synthetic.speaker_names(5)
    assert tuple(normalisers['lf0'].tables('cpu', deltas=True)[1].shape) == (5, 3)
    names, rows = synthetic.speaker_batch_ids(16, n_speakers=5)
    assert rows.dtype == np.int32 and normalisers['lf0'].speaker_rows(names) == rows.tolist()
