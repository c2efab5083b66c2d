"""data.frame_counters on the host (NumPy), FrameCountersSource in FilesDataset and the CLI option, against tests/counters_ref.py
(python integers and Fractions, rounded to float32 from the exact rational).  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import counters_ref as ref
from morgana_amd import _lib, data, ops

KINDS = ('full', 'phone')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n_states', [1, 3, 5])
def test_host_form_equals_the_reference_bit_for_bit(kind, n_states):
    rng = np.random.RandomState(100 + n_states)
    for n_phones in (1, 4, 7, 12):
        dur = ref.random_durations(rng, n_phones, n_states)
        got = data.frame_counters(dur, kind)
        assert got.dtype == np.float32 and got.shape == (int(dur.sum()), ref.COLUMNS[kind])
        np.testing.assert_array_equal(_bits(got), _bits(ref.rows(dur, kind)))
    empty = data.frame_counters(np.zeros((5, n_states), dtype=np.int64), kind)      # an item whose durations are all zero
    assert empty.shape == (0, ref.COLUMNS[kind]) and empty.dtype == np.float32
    if n_states == 1:                                     # (P,), (P, 1) and other integer types are the same item
        dur = ref.random_durations(rng, 6, 1)
        want = data.frame_counters(dur, kind)
        np.testing.assert_array_equal(data.frame_counters(dur[:, 0], kind), want)
        np.testing.assert_array_equal(data.frame_counters(dur.astype(np.int32), kind), want)


@pytest.mark.parametrize('kind', KINDS)
def test_a_phone_of_2_to_the_24_minus_1_frames(kind):
    """The longest phone the exactness claim covers, between two short ones: first, last and a handful of frames in between."""
    long = 2 ** 24 - 1
    dur = np.array([[3], [long], [2]], dtype=np.int64)
    got = data.frame_counters(dur, kind)
    assert got.shape == (long + 5, ref.COLUMNS[kind])
    frames = [0, 2, 3, 4, 5, 3 + 12345, 3 + 2 ** 23 - 1, 3 + 2 ** 23, 3 + 2 ** 23 + 1, 3 + 11184810, long, long + 1, long + 2, long + 3, long + 4]
    np.testing.assert_array_equal(_bits(got[frames]), _bits(ref.rows(dur, kind, frames=frames)))


def test_hand_written_example_pins_the_column_order():
    """Two phones of two states: durations [[2, 1], [0, 3]].  Frames 0-1 state 0 of phone 0, frame 2 its state 1, frames 3-5 state 1 of
    phone 1 (whose state 0 is empty)."""
    dur = np.array([[2, 1], [0, 3]], dtype=np.int64)
    f = np.float32
    third, two_thirds = f(1.0 / 3.0), f(2.0 / 3.0)
    #        (i+1)/n_s   (n_s-i)/n_s  n_s  s+1  S-s  n_p  n_s/n_p     (n_p-j)/n_p  (j+1)/n_p
    want = np.array([
        [f(0.5),     f(1.0),     2,   1,   2,   3,   two_thirds, f(1.0),     third],          # t = 0: p 0, s 0, i 0, j 0
        [f(1.0),     f(0.5),     2,   1,   2,   3,   two_thirds, two_thirds, two_thirds],     # t = 1: p 0, s 0, i 1, j 1
        [f(1.0),     f(1.0),     1,   2,   1,   3,   third,      third,      f(1.0)],         # t = 2: p 0, s 1, i 0, j 2
        [third,      f(1.0),     3,   2,   1,   3,   f(1.0),     f(1.0),     third],          # t = 3: p 1, s 1, i 0, j 0
        [two_thirds, two_thirds, 3,   2,   1,   3,   f(1.0),     two_thirds, two_thirds],     # t = 4: p 1, s 1, i 1, j 1
        [f(1.0),     third,      3,   2,   1,   3,   f(1.0),     third,      f(1.0)],         # t = 5: p 1, s 1, i 2, j 2
    ], dtype=np.float32)
    np.testing.assert_array_equal(_bits(data.frame_counters(dur, 'full')), _bits(want))
    np.testing.assert_array_equal(_bits(ref.rows(dur, 'full')), _bits(want))
    np.testing.assert_array_equal(_bits(data.frame_counters(dur, 'phone')), _bits(want[:, [8, 7, 5]]))


def test_one_state_per_phone_makes_the_state_and_phone_columns_coincide():
    dur = ref.random_durations(np.random.RandomState(3), 9, 1)
    got = data.frame_counters(dur)
    for a, b in ((0, 8), (1, 7), (2, 5)):
        np.testing.assert_array_equal(_bits(got[:, a]), _bits(got[:, b]))
    for c in (3, 4, 6):
        assert np.all(got[:, c] == 1.0)


def test_refusals():
    with pytest.raises(ValueError, match='negative'):
        data.frame_counters(np.array([[3], [-1], [2]], dtype=np.int64))
    with pytest.raises(TypeError):
        data.frame_counters(np.array([[3.0], [1.0]]))
    with pytest.raises(ValueError):
        data.frame_counters(np.zeros((2, 3, 4), dtype=np.int64))
    with pytest.raises(ValueError, match='kind'):
        data.frame_counters(np.array([3, 1]), kind='minimal')
    with pytest.raises(ValueError):
        data.frame_counters(np.array([3, 1]), max_len=4)
    with pytest.raises(TypeError):
        data.frame_counters([3, 1])
    with pytest.raises(_lib.MorganaHipError):             # a CPU tensor: no CPU fallback of the device form
        data.frame_counters(torch.tensor([[3, 1]]))
    with pytest.raises(TypeError):
        data.frame_counters(torch.tensor([[3.0, 1.0]]))
    with pytest.raises(_lib.MorganaHipError):
        ops.frame_counters(torch.tensor([[3, 1]]), t=4)
    with pytest.raises(ValueError):
        data.CountersSpec(kind='minimal')
    with pytest.raises(ValueError):
        data.FrameCountersSource('dur', dur_name='dur')
    spec = data.FrameCountersSource().counter_spec
    assert (spec.source, spec.kind, spec.columns) == ('dur', 'full', 9) and data.CountersSpec('state_dur', 'phone').columns == 3
    assert data.FrameCountersSource.use_deltas is False and data.FrameCountersSource()('utt', '/nowhere') == {}


def test_entry_point_validates_its_arguments_without_a_gpu():
    lib = _lib.load()
    full, ok = _lib.MG_COUNTERS_FULL, 8                    # (fake addresses: nothing is launched before the checks fail)
    call = lambda **kw: lib.mg_frame_counters_f32(*[kw.get(k, v) for k, v in (
        ('dur', ok), ('b', 2), ('p', 5), ('s', 1), ('sb', 5), ('sp', 1), ('ss', 0), ('n_phones', None), ('seq_len', None), ('t', 10),
        ('kind', full), ('p0', None), ('p1', None), ('item_row', None), ('n_rows', 0), ('norm_kind', -1), ('raw', ok), ('norm', None),
        ('blocks', 0), ('stream', None))])
    for bad in (dict(kind=7), dict(p=0), dict(s=0), dict(t=-1), dict(b=-1), dict(p=ops.MAX_PHONES + 1), dict(p=ops.MAX_PHONES // 5 + 1, s=5),
                dict(sp=-1), dict(raw=None), dict(norm=ok), dict(norm=ok, p0=ok, p1=ok, norm_kind=_lib.MG_DENORM_MVN),
                dict(norm=ok, p0=ok, p1=ok, norm_kind=_lib.MG_NORM_MVN, item_row=ok, n_rows=0), dict(blocks=-1), dict(dur=None), dict(dur=4),
                dict(raw=6)):
        assert call(**bad) == _lib.MG_EINVAL, bad
    assert call(b=0) == _lib.MG_OK and call(t=0) == _lib.MG_OK
    assert ops.COUNTERS_KINDS == {'full': (0, 9), 'phone': (1, 3)}


# ---------------------------------------------------------------------------------------------------------------- FilesDataset
def _corpus(root, n_states):
    rng = np.random.RandomState(17)
    names = ['utt%d' % i for i in range(3)]
    durs = {}
    for name in names:
        state_dur = ref.random_durations(rng, 6, n_states, high=9)
        durs[name] = state_dur
        for folder, value in (('state_dur', state_dur), ('dur', state_dur.sum(axis=1, keepdims=True)),
                              ('counters', data.frame_counters(state_dur.sum(axis=1)))):
            os.makedirs(root / 'train' / folder, exist_ok=True)
            np.save(root / 'train' / folder / (name + '.npy'), value)
    (root / 'ids.scp').write_text('\n'.join(names) + '\n')
    return names, durs


@pytest.mark.parametrize('source,kind', [('dur', 'full'), ('state_dur', 'full'), ('state_dur', 'phone')])
def test_files_dataset_with_a_frame_counters_source(tmp_path, source, kind):
    names, durs = _corpus(tmp_path, 5)
    cols = ref.COLUMNS[kind]
    normaliser = data.MinMaxNormaliser('counters')
    rng = np.random.RandomState(1)
    normaliser.set_params({'mmin': rng.rand(cols).astype(np.float32), 'mmax': (rng.rand(cols) + 2).astype(np.float32)})
    sources = {source: data.NumpyBinarySource(source), 'counters': data.FrameCountersSource('counters', dur_name=source, kind=kind)}
    dataset = data.FilesDataset(sources, 'train', 'ids.scp', {'counters': normaliser}, data_root=str(tmp_path))
    assert list(dataset.counter_specs()) == ['counters'] and dataset.counter_specs()['counters'].source == source
    for i, name in enumerate(names):
        assert sorted(dataset.raw(i)) == sorted(['name', source])                   # raw() has neither
        item = dataset[i]
        dur = durs[name] if source == 'state_dur' else durs[name].sum(axis=1)
        want = ref.rows(dur, kind)
        np.testing.assert_array_equal(_bits(item['counters']), _bits(want))
        twin = normaliser.normalise(want).astype(np.float32)
        assert item['normalised_counters'].dtype == np.float32
        np.testing.assert_array_equal(_bits(item['normalised_counters']), _bits(twin))
    # a corpus that also reads ``counters`` from files under the same name: read or computed, not both
    both = dict(sources, files=data.NumpyBinarySource('counters'))
    clash = data.FilesDataset(both, 'train', 'ids.scp', {'counters': normaliser}, data_root=str(tmp_path))
    with pytest.raises(ValueError, match='read from files or computed'):
        clash[0]
    # durations that no source provides
    alone = data.FilesDataset({'counters': data.FrameCountersSource()}, 'train', 'ids.scp', {}, data_root=str(tmp_path))
    with pytest.raises(KeyError):
        alone[0]


def test_loaders_take_counter_specs_and_refuse_on_the_host_what_they_can():
    utts = [{'name': 'a', 'dur': np.array([[2], [3]], dtype=np.int64)}]
    loader = data.DeviceBatches(utts, 2, {}, 'cuda:0', counter_specs={'counters': data.CountersSpec()})
    assert list(loader.counter_specs) == ['counters'] and data.DeviceBatches(utts, 2, {}, 'cuda:0').counter_specs == {}
    with pytest.raises(ValueError, match='read from files or computed'):
        data.collate_to_device([dict(utts[0], counters=np.zeros((5, 9), dtype=np.float32))], {}, 'cpu', counter_specs={'counters': data.CountersSpec()})
    with pytest.raises(KeyError):
        data.collate_to_device(utts, {}, 'cpu', counter_specs={'counters': data.CountersSpec('state_dur')})
    with pytest.raises(TypeError):
        data.collate_to_device([{'name': 'a', 'dur': np.ones((2, 1), dtype=np.float32)}], {}, 'cpu', counter_specs={'counters': data.CountersSpec()})


def test_cli_parse_spec():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))
    try:
        import fit_normalisers as cli
    finally:
        sys.path.pop(0)
    name, normaliser, deltas, source = cli.parse_spec('counters:minmax:counters=dur', None)
    assert (name, deltas) == ('counters', 'file') and isinstance(normaliser, data.MinMaxNormaliser) and not normaliser.use_deltas
    assert isinstance(source, data.CountersSpec) and (source.source, source.kind) == ('dur', 'full')
    source = cli.parse_spec('counters:minmax:counters=state_dur,full', None)[3]
    assert (source.source, source.kind) == ('state_dur', 'full')
    source = cli.parse_spec('pos:mvn:counters=state_dur,phone', 'speakers.txt')
    assert isinstance(source[1], data.SpeakerDependentMeanVarianceNormaliser) and (source[3].source, source[3].kind) == ('state_dur', 'phone')
    assert cli.parse_spec('mcep:mvn:deltas', None)[2:] == ('file', None)            # the other forms are what they were
    assert cli.parse_spec('lf0:mvn:deltas=compute:from=f0', None)[2:] == ('compute', 'f0')
    for bad in ('counters:minmax:counters=', 'counters:minmax:counters=counters', 'counters:minmax:counters=dur,', 'counters:minmax:counters=dur,half',
                'counters:minmax:counters', 'counters:minmax:counters=dur:deltas', 'counters:minmax:deltas=compute:counters=dur',
                'counters:minmax:counters=dur:from=f0', 'counters:minmax:counters=dur:counters=dur', 'counters:var:counters=dur'):
        with pytest.raises(SystemExit):
            cli.parse_spec(bad, None)
