"""Corpus statistics without a GPU: the float64 reference judged by exact arithmetic, the chunk-and-Chan scheme restated in NumPy,
the argument checks of mg_column_stats_f32 (the library loads without a device), save_params -> load_params, the arithmetic of
ColumnStats.result / params on a hand-written state, and the absence of a CPU path."""
import json
import os

import numpy as np
import pytest
import torch

import colstats_ref64 as ref
from morgana_amd import _lib, data, ops


def test_the_reference_judges_itself_and_the_naive_forms_fail():
    column = ref.adversarial_column(2113)
    assert np.all(column >= 2.0 ** 20) and len(np.unique(column)) == 8
    mean, var = ref.exact(column)
    got = ref.two_pass([column.reshape(-1, 1)])
    assert abs(got['var'][0, 0] - float(var)) <= 1e-13 * float(var)
    assert abs(got['mean'][0, 0] - float(mean)) <= 2.0 ** -52 * float(mean)
    assert got['count'][0, 0] == 2113 and got['mmin'][0, 0] == column.min() and got['mmax'][0, 0] == column.max()
    for sequential in (True, False):                      # 1.8e-2 and 1.6e-5 relative: the case bites
        miss = abs(ref.naive(column, sequential) - float(var)) / float(var)
        print('naive sum of squares, %s: %.3g relative' % ('sequential' if sequential else 'np.sum', miss))
        assert miss > ref.CAP_VAR


def test_two_pass_handles_ragged_items_and_groups():
    rng = np.random.RandomState(3)
    items = [rng.randn(n, 2).astype(np.float32) for n in (0, 1, 5, 3)]
    got = ref.two_pass(items, item_row=[0, 2, 7, 2], groups=3)
    np.testing.assert_array_equal(got['count'], [[0, 0], [0, 0], [4, 4]])
    rows = np.concatenate([items[1], items[3]]).astype(np.float64)
    np.testing.assert_allclose(got['mean'][2], rows.mean(axis=0), rtol=1e-15)
    np.testing.assert_allclose(got['var'][2], rows.var(axis=0), rtol=1e-14)
    assert np.isnan(got['mean'][:2]).all()
    for col in range(2):
        mean, var = ref.exact(rows[:, col])
        assert abs(got['var'][2, col] - float(var)) <= 1e-13 * float(var)


def test_chunk_and_chan_restatement_stays_under_the_cap():
    column = ref.adversarial_column(2113)
    mean, var = ref.exact(column)
    n, got_mean, m2 = ref.chunk_chan(column)
    miss = abs(m2 / n - float(var)) / float(var)
    print('chunk + Chan on the 2^20 + k/8 column: %.3g relative' % miss)
    assert n == 2113 and miss <= ref.CAP_VAR
    bound_mean, bound_var = ref.bounds([column.reshape(-1, 1)], np.array([[2113.0]]))
    assert abs(m2 / n - float(var)) <= bound_var[0, 0] <= ref.CAP_VAR * float(var)
    assert abs(got_mean - float(mean)) <= bound_mean[0, 0] <= ref.CAP_MEAN * float(column.max())
    for value in (np.float32(0.1), np.float32(2.0 ** 20 + 0.125), np.float32(-3e-30)):
        n, got_mean, m2 = ref.chunk_chan(np.full(2113, value, dtype=np.float32))
        assert m2 == 0.0 and got_mean == float(value) and n == 2113


def test_chan_skips_empty_partials():
    assert ref.chan((0.0, 0.0, 0.0), (3.0, 1.5, 2.0)) == (3.0, 1.5, 2.0)
    assert ref.chan((3.0, 1.5, 2.0), (0.0, float('nan'), float('nan'))) == (3.0, 1.5, 2.0)


def test_column_stats_validates_its_arguments_without_a_gpu():
    lib = _lib.load()
    fake = 1 << 20                                        # never dereferenced: every call below returns before a launch
    need = lib.mg_column_stats_workspace_bytes(4, 100, 3)
    assert need > 0 and need % 8 == 0
    assert lib.mg_column_stats_workspace_bytes(0, 100, 3) == 0 and lib.mg_column_stats_workspace_bytes(4, 100, 0) == 0
    assert lib.mg_column_stats_workspace_bytes(4, 100, 3) <= lib.mg_column_stats_workspace_bytes(4, 100000, 3)

    def call(x=fake, ld=3, d=3, b=4, t=100, offsets=None, seq_len=fake, item_row=None, s=1, state=fake, ws=fake, ws_bytes=need):
        return lib.mg_column_stats_f32(x, ld, d, b, t, offsets, seq_len, item_row, s, state, ws, ws_bytes, None)

    for rc in (call(offsets=fake, seq_len=fake), call(offsets=None, seq_len=None)):
        assert rc == -1 and 'mg_column_stats_f32' in _lib.last_error() and 'exactly one' in _lib.last_error()
    for d in (0, -3, _lib.MG_COLSTATS_MAX_D + 1):
        assert call(d=d, ld=max(d, 1)) == -1 and 'mg_column_stats_f32: D=' in _lib.last_error()
    for s in (0, -1):
        assert call(s=s) == -1 and 'mg_column_stats_f32: S=' in _lib.last_error()
    assert call(s=2, item_row=None) == -1 and 'item_row' in _lib.last_error()
    assert call(state=None) == -1 and 'mg_column_stats_f32: state' in _lib.last_error()
    assert call(ld=2) == -1 and 'ld=2' in _lib.last_error()
    assert call(x=None) == -1 and call(ws=None) == -1
    assert call(x=fake + 2) == -1 and 'aligned' in _lib.last_error()
    assert call(ws_bytes=need - 1) == -3 and 'mg_column_stats_f32: workspace' in _lib.last_error()
    assert call(offsets=fake, seq_len=None, ws_bytes=lib.mg_column_stats_workspace_bytes(4, 1, 3) - 1) == -3
    assert call(b=0) == 0 and call(b=0, x=None, ws=None, ws_bytes=0) == 0
    assert call(t=0) == 0                                 # an empty padded batch: nothing to launch
    assert call(b=-1) == -1


def _random_params(rng, kind, width):
    lo = rng.randn(width).astype(np.float32)
    return dict(zip(data._KINDS[kind]['params'], (lo, lo + np.abs(rng.randn(width)).astype(np.float32) + np.float32(0.1))))


@pytest.mark.parametrize('cls, kind', [(data.MeanVarianceNormaliser, 'mvn'), (data.MinMaxNormaliser, 'minmax')])
def test_save_params_round_trip(tmp_path, cls, kind):
    rng = np.random.RandomState(5)
    own, deltas = _random_params(rng, kind, 3), _random_params(rng, kind, 9)
    own[data._KINDS[kind]['params'][0]][0] = np.float32(1.0) / np.float32(3.0)       # not a short decimal
    cls('lf0', use_deltas=True).set_params(own, deltas).save_params('norm', data_root=str(tmp_path))
    assert sorted(os.listdir(tmp_path / 'norm')) == ['lf0_deltas_%s.json' % kind, 'lf0_%s.json' % kind]
    with open(tmp_path / 'norm' / ('lf0_%s.json' % kind)) as f:
        stored = json.load(f)
    assert sorted(stored) == sorted(data._KINDS[kind]['params'])
    assert all(isinstance(v, list) and all(isinstance(e, float) for e in v) for v in stored.values())
    loaded = cls('lf0', use_deltas=True)
    loaded.load_params('norm', data_root=str(tmp_path))
    for name in data._KINDS[kind]['params']:
        assert loaded.params[name].dtype == np.float32
        np.testing.assert_array_equal(loaded.params[name].view(np.uint32), own[name].view(np.uint32))
        np.testing.assert_array_equal(loaded.delta_params[name].view(np.uint32), deltas[name].view(np.uint32))
    with pytest.raises(RuntimeError, match='no parameters to save'):
        cls('vuv').save_params('norm', data_root=str(tmp_path))


@pytest.mark.parametrize('cls, kind', [(data.SpeakerDependentMeanVarianceNormaliser, 'mvn'),
                                       (data.SpeakerDependentMinMaxNormaliser, 'minmax')])
def test_save_params_round_trip_per_speaker(tmp_path, cls, kind):
    rng = np.random.RandomState(6)
    (tmp_path / 'speakers.txt').write_text('anna\nbert\n')
    own = {spk: _random_params(rng, kind, 4) for spk in ('anna', 'bert')}
    deltas = {spk: _random_params(rng, kind, 12) for spk in ('anna', 'bert')}
    cls('mcep', 'speakers.txt', use_deltas=True).set_params(own, deltas).save_params('norm', data_root=str(tmp_path))
    for spk in ('anna', 'bert'):
        assert sorted(os.listdir(tmp_path / 'norm' / spk)) == ['mcep_deltas_%s.json' % kind, 'mcep_%s.json' % kind]
    loaded = cls('mcep', 'speakers.txt', use_deltas=True)
    loaded.load_params('norm', data_root=str(tmp_path))
    assert loaded.speaker_ids == ['anna', 'bert']
    for spk in ('anna', 'bert'):
        for name in data._KINDS[kind]['params']:
            np.testing.assert_array_equal(loaded.params[spk][name].view(np.uint32), own[spk][name].view(np.uint32))
            np.testing.assert_array_equal(loaded.delta_params[spk][name].view(np.uint32), deltas[spk][name].view(np.uint32))


def test_column_stats_result_and_params_arithmetic():
    state = np.zeros((3, 5, 2))
    state[0] = [[4, 4], [1.5, -2.0], [8.0, -1e-20], [-1.0, -2.0], [3.0, -2.0]]       # second column: M2 a rounding below zero
    state[1] = [[1, 1], [0.1, 0.2], [0.0, 0.0], [0.1, 0.2], [0.1, 0.2]]              # one frame
    state[2, 1:] = 123.0                                                           # count == 0: the other fields are ignored
    stats = data.ColumnStats.from_state(state)
    assert (stats.groups, stats.dim) == (3, 2)
    pop, sample = stats.result(), stats.result(ddof=1)
    np.testing.assert_array_equal(pop['count'], [[4, 4], [1, 1], [0, 0]])
    np.testing.assert_array_equal(pop['var'][:2], [[2.0, 0.0], [0.0, 0.0]])
    np.testing.assert_array_equal(sample['var'][0], [8.0 / 3.0, 0.0])
    assert np.isnan(sample['var'][1]).all()               # one frame has no sample variance
    np.testing.assert_array_equal(pop['std_dev'][0], [np.sqrt(2.0), 0.0])
    for field in ('mean', 'var', 'std_dev', 'mmin', 'mmax'):
        assert np.isnan(pop[field][2]).all(), field
        assert pop[field].dtype == np.float64 and pop[field].shape == (3, 2)
    np.testing.assert_array_equal(pop['mmin'][0], [-1.0, -2.0])
    mvn, minmax = stats.params('mvn'), stats.params('minmax', group=1)
    assert sorted(mvn) == ['mean', 'std_dev'] and sorted(minmax) == ['mmax', 'mmin']
    assert mvn['std_dev'].dtype == np.float32 and mvn['std_dev'][0] == np.float32(np.sqrt(2.0))
    np.testing.assert_array_equal(minmax['mmin'], np.array([0.1, 0.2], dtype=np.float32))
    assert stats.params('mvn', ddof=1)['std_dev'][0] == np.float32(np.sqrt(8.0 / 3.0))
    nan_state = state.copy()
    nan_state[0, 2, 0] = np.nan                           # a NaN column stays NaN through the floor
    assert np.isnan(data.ColumnStats.from_state(nan_state).result()['var'][0, 0])


def test_there_is_no_cpu_fallback(tmp_path):
    utterances = [{'name': 'a', 'lf0': np.zeros((5, 1), dtype=np.float32)}]
    with pytest.raises(_lib.MorganaHipError, match='no CPU fallback'):
        data.fit_normalisers(utterances, {'lf0': data.MeanVarianceNormaliser('lf0')}, device='cpu', out_dir='norm', data_root=str(tmp_path))
    assert os.listdir(tmp_path) == []
    with pytest.raises(_lib.MorganaHipError):
        data.ColumnStats(3, device='cpu')
    with pytest.raises(_lib.MorganaHipError, match='no CPU fallback'):
        ops.column_stats(torch.zeros((1, 5, 3), dtype=torch.float64), torch.zeros((2, 4, 3)), seq_len=torch.tensor([4, 2]))
    with pytest.raises(_lib.MorganaHipError):
        data.ColumnStats.from_state(np.zeros((1, 5, 3))).update_padded(torch.zeros((2, 4, 3)), torch.tensor([4, 2]))
