"""K29 without a GPU: tests/f0_ref64.py against np.interp, the host form of data.continuous_lf0 against that reference, the file-backed
loader's host path, the refusals, the CLI's spec parser and the argument checks of mg_continuous_lf0_f32 through the C ABI."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import f0_ref64 as ref
from morgana_amd import _lib, data, ops

CHUNK = 256                      # mg_continuous_lf0_chunk_rows(): pinned in test_entry_point_validates_its_arguments_without_a_gpu
WIDTHS = (1, 3, 4)


@functools.lru_cache(maxsize=None)
def _case(width):
    return ref.case(width, CHUNK)


@functools.lru_cache(maxsize=None)
def _want(width, log_input=False):
    items = ref.log_case(_case(width)[0]) if log_input else _case(width)[0]
    return tuple(ref.reference(x, log_input=log_input) for x in items)


def test_the_case_holds_every_pattern():
    items, names = _case(1)
    assert sorted(set(len(x) for x in items)) == [0, 1, 2, 63, 64, 65, 2 * CHUNK + 1]
    seen = set(n for picked in names for n in picked)
    assert seen == set(name for pats in ref._pattern_flags(CHUNK).values() for name, _ in pats)
    assert ref.adjacent_pairs(items) == (True, True)
    gaps = dict(ref._pattern_flags(CHUNK)[2 * CHUNK + 1])['gaps of 64, 65 and chunk + 1']
    runs = np.diff(np.flatnonzero(np.diff(np.concatenate(([1], gaps.astype(int), [1]))) != 0))[::2]
    assert sorted(runs) == [64, 65, CHUNK + 1]
    edge = dict(ref._pattern_flags(CHUNK)[2 * CHUNK + 1])['a gap from the last frame of a chunk']
    assert edge[CHUNK - 2] and not edge[CHUNK - 1] and not edge[CHUNK]
    for width in (3, 4):
        wide, wide_names = _case(width)
        assert any(len(set(picked)) == width for picked in wide_names)              # the columns of an item differ in their voicing
        assert any(np.isnan(x).any() for x in wide) and any((x < 0).any() for x in wide)


def test_reference_against_np_interp():
    """The long-double reference is np.interp over np.log of the voiced frames, to 1e-12 (np.interp holds the edge values too)."""
    for width in WIDTHS:
        for x, (want, vuv, _, _) in zip(_case(width)[0], _want(width)):
            for c in range(x.shape[1]):
                voiced = np.flatnonzero(x[:, c] > 0)
                np.testing.assert_array_equal(vuv[:, c], (x[:, c] > 0).astype(np.float32))
                if voiced.size == 0:
                    assert np.all(want[:, c] == 0)
                    continue
                interp = np.interp(np.arange(len(x)), voiced, np.log(x[voiced, c].astype(np.float64)))
                assert np.max(np.abs(want[:, c].astype(np.float64) - interp)) <= 1e-12 * np.max(np.abs(interp))


@pytest.mark.parametrize('log_input', [False, True], ids=['raw', 'log'])
@pytest.mark.parametrize('width', WIDTHS)
def test_host_form_against_the_reference(width, log_input):
    items = ref.log_case(_case(width)[0]) if log_input else _case(width)[0]
    worst = 0.0
    for x, (want, vuv, scale, interpolated) in zip(items, _want(width, log_input)):
        lf0, flag = data.continuous_lf0(x, log_input=log_input)
        assert lf0.dtype == np.float32 and flag.dtype == np.float32 and lf0.shape == x.shape == flag.shape
        np.testing.assert_array_equal(flag, vuv)
        limit = ref.bound(want, scale, interpolated, log_input)
        worst = max(worst, ref.worst_ratio(lf0, want, limit))
        assert not ref.misses(lf0, want, limit)
    print('D=%d log_input=%s: largest |host - reference| / bound = %.3f' % (width, log_input, worst))


def test_host_form_arguments():
    x = np.array([[0.0], [100.0], [0.0], [200.0], [0.0]], dtype=np.float32)
    lf0, vuv = data.continuous_lf0(x)
    lo, hi = np.log(np.float64(100.0)), np.log(np.float64(200.0))
    np.testing.assert_array_equal(lf0[:, 0], np.array([lo, lo, lo + (hi - lo) * 0.5, hi, hi]).astype(np.float32))
    np.testing.assert_array_equal(vuv[:, 0], [0, 1, 0, 1, 0])
    # a threshold of one's own; fill; an item without a voiced frame; lengths 0 and 1
    lf0, vuv = data.continuous_lf0(x, voiced_above=150.0)
    np.testing.assert_array_equal(vuv[:, 0], [0, 0, 0, 1, 0])
    np.testing.assert_array_equal(lf0[:, 0], np.full(5, np.float32(hi)))
    lf0, vuv = data.continuous_lf0(np.zeros((4, 2), dtype=np.float32), fill=-7.25)
    assert np.all(lf0 == np.float32(-7.25)) and np.all(vuv == 0)
    lf0, vuv = data.continuous_lf0(np.zeros((0, 1), dtype=np.float32))
    assert lf0.shape == vuv.shape == (0, 1)
    # log_input: the HTS marker is unvoiced by default, the values pass through untouched
    y = np.array([[-1e10], [4.5], [-1e10], [5.5]], dtype=np.float32)
    lf0, vuv = data.continuous_lf0(y, log_input=True)
    np.testing.assert_array_equal(lf0[:, 0], np.float32([4.5, 4.5, 5.0, 5.5]))
    np.testing.assert_array_equal(vuv[:, 0], [0, 1, 0, 1])
    with pytest.raises(ValueError, match='seq_len'):
        data.continuous_lf0(x, seq_len=np.array([5]))
    with pytest.raises(ValueError, match='frames, features'):
        data.continuous_lf0(np.zeros(5, dtype=np.float32))
    with pytest.raises(ValueError, match='NaN'):
        data.continuous_lf0(x, voiced_above=float('nan'))


def test_refusals():
    x = torch.zeros(4, 1)
    with pytest.raises(_lib.MorganaHipError, match='no CPU fallback'):
        data.continuous_lf0(x)
    with pytest.raises(RuntimeError, match='no backward'):
        data.continuous_lf0(torch.zeros(4, 1, requires_grad=True))
    with pytest.raises(TypeError):
        data.continuous_lf0([[1.0]])
    with pytest.raises(_lib.MorganaHipError):
        ops.continuous_lf0(torch.zeros(4, 1), offsets=torch.tensor([0, 4]), t=4)
    utterance = {'name': 'a', 'f0': np.zeros((3, 1), dtype=np.float32), 'lf0': np.zeros((3, 1), dtype=np.float32)}
    with pytest.raises(ValueError, match="'lf0' is in the utterances and in f0_specs"):
        data.collate_to_device([utterance], {}, 'cpu', f0_specs={'lf0': data.F0Spec()})
    utterance = {'name': 'a', 'f0': np.zeros((3, 1), dtype=np.float32), 'vuv': np.zeros((3, 1), dtype=np.float32)}
    with pytest.raises(ValueError, match="'vuv' is in the utterances and in f0_specs"):
        data.collate_to_device([utterance], {}, 'cpu', f0_specs={'lf0': data.F0Spec()})
    with pytest.raises(KeyError, match='f0_specs read'):
        data.collate_to_device([{'name': 'a'}], {}, 'cpu', f0_specs={'lf0': data.F0Spec()})
    with pytest.raises(TypeError, match='float32'):
        data.collate_to_device([{'f0': np.zeros((3, 1))}], {}, 'cpu', f0_specs={'lf0': data.F0Spec()})
    with pytest.raises(ValueError, match='must differ'):
        data.ContinuousLF0Source('lf0', f0_name='lf0')
    with pytest.raises(ValueError):
        data.F0Spec(source='')


# ---------------------------------------------------------------------------------------------------------------- the file-backed loader
@pytest.fixture()
def corpus(tmp_path):
    rng = np.random.RandomState(5)
    ids = ['utt%02d' % i for i in range(4)]
    os.makedirs(tmp_path / 'train' / 'f0')
    tracks = {}
    for i, name in enumerate(ids):
        n = 40 + 13 * i
        track = (80.0 + 200.0 * rng.rand(n, 1)).astype(np.float32)
        track[rng.rand(n) < 0.4] = 0.0
        track[:i] = 0.0
        tracks[name] = track
        np.save(tmp_path / 'train' / 'f0' / (name + '.npy'), track)
    with open(tmp_path / 'ids.scp', 'w') as f:
        f.write('\n'.join(ids) + '\n')
    return tmp_path, ids, tracks


def test_files_dataset_computes_lf0_and_vuv_on_the_host(corpus):
    root, ids, tracks = corpus
    normaliser = data.MeanVarianceNormaliser('lf0', use_deltas=True)
    normaliser.set_params({'mean': [5.0], 'std_dev': [0.5]}, {'mean': [5.0, 0.0, 0.0], 'std_dev': [0.5, 0.1, 0.05]})
    source = data.ContinuousLF0Source('lf0', use_deltas=True)
    assert source.f0_spec.source == 'f0' and source.f0_spec.vuv == 'vuv' and source.delta_spec.edge == 'replicate'
    assert data.ContinuousLF0Source('lf0').delta_spec is None
    dataset = data.FilesDataset({'lf0': source}, 'train', 'ids.scp', {'lf0': normaliser}, data_root=str(root))
    assert list(dataset.f0_specs()) == ['lf0'] and isinstance(dataset.f0_specs()['lf0'], data.F0Spec)
    assert list(dataset.delta_specs()) == ['lf0']
    for i, name in enumerate(ids):
        raw = dataset.raw(i)
        assert sorted(raw) == ['f0', 'name'] and raw['name'] == name
        np.testing.assert_array_equal(raw['f0'], tracks[name])
        item = dataset[i]
        assert sorted(item) == ['f0', 'lf0', 'lf0_deltas', 'name', 'normalised_lf0', 'normalised_lf0_deltas', 'vuv']
        lf0, vuv = data.continuous_lf0(tracks[name])
        np.testing.assert_array_equal(item['lf0'], lf0)
        np.testing.assert_array_equal(item['vuv'], vuv)
        np.testing.assert_array_equal(item['lf0_deltas'], data.compute_deltas(lf0))
        np.testing.assert_array_equal(item['normalised_lf0'], normaliser.normalise(lf0).astype(np.float32))
        np.testing.assert_array_equal(item['normalised_lf0_deltas'], normaliser.normalise(item['lf0_deltas'], deltas=True).astype(np.float32))
    # a corpus that also holds lf0 files next to a source that computes them: one or the other
    os.makedirs(root / 'train' / 'lf0')
    for name in ids:
        np.save(root / 'train' / 'lf0' / (name + '.npy'), data.continuous_lf0(tracks[name])[0])
    both = data.FilesDataset({'lf0': source, 'files': data.NumpyBinarySource('lf0')}, 'train', 'ids.scp', {}, data_root=str(root))
    with pytest.raises(ValueError, match='read from files or computed'):
        both[0]
    # a float64 track on disk (WORLD) and a 1-D one are taken as float32 (frames, 1)
    np.save(root / 'train' / 'f0' / 'utt00.npy', tracks['utt00'][:, 0].astype(np.float64))
    np.testing.assert_array_equal(dataset.raw(0)['f0'], tracks['utt00'])


def test_loaders_take_f0_specs():
    """The device loaders accept ``f0_specs`` and default to what the data sources ask for (their kernels are tested on the GPU)."""
    loader = data.DeviceBatches([{'f0': np.zeros((3, 1), dtype=np.float32)}], 2, {}, 'cpu', f0_specs={'lf0': data.F0Spec()})
    assert list(loader.f0_specs) == ['lf0']
    assert data.DeviceBatches([], 2, {}, 'cpu').f0_specs == {}
    with pytest.raises(_lib.MorganaHipError):
        data.fit_normalisers([{'f0': np.zeros((3, 1), dtype=np.float32)}], {'lf0': data.MeanVarianceNormaliser('lf0')}, device='cpu',
                             f0_specs={'lf0': data.F0Spec()})


def test_cli_parse_spec():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))
    try:
        import fit_normalisers as cli
    finally:
        sys.path.pop(0)
    name, normaliser, deltas, source = cli.parse_spec('lf0:mvn:deltas=compute:from=f0', None)
    assert (name, deltas, source) == ('lf0', 'compute', 'f0') and isinstance(normaliser, data.MeanVarianceNormaliser) and normaliser.use_deltas
    name, normaliser, deltas, source = cli.parse_spec('lf0:minmax:from=pitch', None)
    assert (name, deltas, source) == ('lf0', 'file', 'pitch') and isinstance(normaliser, data.MinMaxNormaliser) and not normaliser.use_deltas
    assert cli.parse_spec('mcep:mvn:deltas', None)[2:] == ('file', None)
    assert cli.parse_spec('mcep:mvn', None)[2:] == ('file', None)
    assert isinstance(cli.parse_spec('lf0:mvn:deltas=compute:from=f0', 'speakers.txt')[1], data.SpeakerDependentMeanVarianceNormaliser)
    for bad in ('lf0:mvn:deltas:from=f0', 'lf0:mvn:from=', 'lf0:mvn:from=lf0', 'lf0:mvn:from=f0:from=f1', 'lf0:mvn:from', 'lf0:var:from=f0'):
        with pytest.raises(SystemExit):
            cli.parse_spec(bad, None)


# ---------------------------------------------------------------------------------------------------------------- the C entry point
def test_entry_point_validates_its_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.mg_continuous_lf0_chunk_rows() == CHUNK
    assert (_lib.MG_F0_VUV_PADDED, _lib.MG_F0_VUV_PACKED) == (0, 1)
    x, off, seq, out, p = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20       # never dereferenced: every call below is refused on the host
    names = ('x', 'D', 'B', 'offsets', 'seq_len', 'T_in', 'log_input', 'voiced_above', 'fill', 'p0', 'p1', 'item_row', 'S', 'kind',
             'out_rows', 'packed_rows', 'packed_out', 'padded_out', 'norm_out', 'vuv_out', 'vuv_form', 'stream')
    ok = (x, 1, 3, off, None, 0, 0, 0.0, 0.0, None, None, None, 0, -1, 10, 30, None, out, None, None, 0, None)
    assert len(names) == len(_lib.SIGNATURES['mg_continuous_lf0_f32'][1])

    def call(**changed):
        args = dict(zip(names, ok))
        args.update(changed)
        return lib.mg_continuous_lf0_f32(*[args[n] for n in names])

    def refused(message, **changed):
        return call(**changed) == _lib.MG_EINVAL and 'mg_continuous_lf0_f32' in _lib.last_error() and message in _lib.last_error()

    assert refused('exactly one of', offsets=None)
    assert refused('exactly one of', seq_len=seq)
    assert refused('D=0', D=0) and refused('D=-3', D=-3)
    assert refused('B=-1', B=-1)
    assert refused('T_in=-1', offsets=None, seq_len=seq, T_in=-1)
    assert refused('NaN', voiced_above=float('nan'))
    assert refused('no output', padded_out=None)
    assert refused('vuv form', vuv_out=out, vuv_form=2)
    assert refused('out_rows=-1', out_rows=-1) and refused('out_rows', out_rows=1 << 31)
    assert refused('out_rows=-1', padded_out=None, vuv_out=out, vuv_form=_lib.MG_F0_VUV_PADDED, out_rows=-1)
    assert refused('packed_rows=-1', packed_out=out, packed_rows=-1)
    assert refused('packed_rows=-1', padded_out=None, vuv_out=out, vuv_form=_lib.MG_F0_VUV_PACKED, packed_rows=-1)
    assert refused('normalised output', norm_out=out)
    assert refused('normalised output', norm_out=out, p0=p, p1=p, kind=_lib.MG_DENORM_MVN)
    assert refused('normalised output', norm_out=out, p0=p, kind=_lib.MG_NORM_MVN)
    assert refused('S=0', norm_out=out, p0=p, p1=p, kind=_lib.MG_NORM_MINMAX, item_row=p, S=0)
    assert refused('overflow', B=1 << 30, out_rows=(1 << 31) - 1, D=1 << 10)
    assert refused('overflow', offsets=None, seq_len=seq, B=1 << 30, T_in=(1 << 31) - 1, D=1 << 10, out_rows=0)
    assert refused('x must not be NULL', x=None)
    assert refused('aligned', x=x + 2) and refused('aligned', padded_out=out + 1) and refused('aligned', offsets=off + 4)
    assert refused('aligned', norm_out=out, p0=p + 2, p1=p, kind=_lib.MG_NORM_MVN)
    # nothing to do is not an error, and nothing is launched (no device is needed): no items
    assert call(B=0) == 0 and call(B=0, x=None) == 0
