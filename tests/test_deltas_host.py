"""Delta features without a GPU: the host form of data.compute_deltas against the exact rational reference of tests/deltas_ref64.py,
FilesDataset over data sources that compute their deltas, the argument checks of mg_deltas_f32 (the library loads without a device),
and the refusals of the loaders."""
import functools
import os

import numpy as np
import pytest
import torch

import deltas_ref64 as ref
from morgana_amd import _lib, data, ops
from morgana_amd.viz import synthesis

WINDOWS = {'default': ref.DEFAULT_WINDOWS, 'static': ref.STATIC_WINDOW, '5pt': ref.WINDOWS_5PT}


@functools.lru_cache(maxsize=None)
def _item(length, width=3):
    x = (np.random.RandomState(100 * length + width).randn(length, width) * 2.0 + 5.0).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _want(length, windows, edge, width=3):
    return ref.reference(_item(length, width), WINDOWS[windows], edge)


def test_the_reference_rounds_once_and_knows_its_windows():
    assert ref.round_f32(ref.Fraction(1, 3)) == np.float32(1.0) / np.float32(3.0)
    tie = ref.Fraction(2 ** 24 + 1)                       # half way between 2^24 and 2^24 + 2: the even mantissa wins
    assert ref.round_f32(tie) == np.float32(2 ** 24) and ref.round_f32(tie + 2) == np.float32(2 ** 24 + 4)
    # 1 + 2^-24 + 2^-60 lies above the tie: a float64 in between would round it down first
    assert ref.round_f32(1 + ref.Fraction(1, 2 ** 24) + ref.Fraction(1, 2 ** 60)) == np.nextafter(np.float32(1), np.float32(2))
    assert ref.round_f32(ref.Fraction(0)) == 0.0
    assert ref.exact_windows(ref.DEFAULT_WINDOWS) and ref.exact_windows(ref.STATIC_WINDOW) and not ref.exact_windows(ref.WINDOWS_5PT)
    assert ref.exponent_span(np.array([1.0, 1.5, 0.0, -3.0])) == 2 and ref.exponent_span(np.zeros(3)) == 0
    for (l, u, c), (rl, ru, rc) in zip(synthesis.DEFAULT_WINDOWS, ref.DEFAULT_WINDOWS):
        assert (l, u, tuple(c)) == (rl, ru, rc)
    exact, rounded, total = ref.reference(np.array([[1.0], [4.0], [9.0]], dtype=np.float32), ref.DEFAULT_WINDOWS, 'replicate')
    np.testing.assert_array_equal(rounded, [[1, 1.5, 3], [4, 4, 2], [9, 2.5, -5]])
    _, zero, _ = ref.reference(np.array([[1.0], [4.0], [9.0]], dtype=np.float32), ref.DEFAULT_WINDOWS, 'zero')
    np.testing.assert_array_equal(zero, [[1, 2, 2], [4, 4, 2], [9, -2, -14]])
    assert total[1, 2] == 1 + 8 + 9 and exact[1, 1] == 4


@pytest.mark.parametrize('edge', ['replicate', 'zero'])
@pytest.mark.parametrize('windows', ['default', 'static', '5pt'])
@pytest.mark.parametrize('length', [1, 2, 3, 40])
def test_host_compute_deltas_against_exact_arithmetic(length, windows, edge):
    x = _item(length)
    assert ref.exponent_span(x) < 29
    got = data.compute_deltas(x, None if windows == 'default' else WINDOWS[windows], edge=edge)
    assert got.dtype == np.float32 and got.shape == (length, len(WINDOWS[windows]) * 3)
    bad = ref.misses(got, _want(length, windows, edge), must_be_rounded=ref.exact_windows(WINDOWS[windows]))
    assert not bad, bad[:5]


def test_host_compute_deltas_edges_and_shapes():
    x = _item(3)
    np.testing.assert_array_equal(data.compute_deltas(x[:1]), np.concatenate([x[:1], np.zeros((1, 6), np.float32)], axis=1))
    zero = data.compute_deltas(x[:1], edge='zero')          # one frame, no neighbours: delta 0, delta-delta -2 x
    np.testing.assert_array_equal(zero, np.concatenate([x[:1], np.zeros((1, 3), np.float32), -2 * x[:1]], axis=1))
    assert data.compute_deltas(np.zeros((0, 4), np.float32)).shape == (0, 12)
    assert data.compute_deltas(x, edge='zero')[1].tolist() == data.compute_deltas(x)[1].tolist()      # the inner frame has no edge
    with pytest.raises(ValueError, match='edge'):
        data.compute_deltas(x, edge='reflect')
    with pytest.raises(ValueError, match='coefficients'):
        data.compute_deltas(x, windows=[(1, 1, (1.0, 2.0))])
    with pytest.raises(ValueError, match='frames, features'):
        data.compute_deltas(np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError, match='seq_len'):
        data.compute_deltas(x, seq_len=np.array([3]))


def test_device_path_refuses_cpu_tensors_and_gradients():
    with pytest.raises(_lib.MorganaHipError, match='no CPU fallback'):
        data.compute_deltas(torch.zeros(2, 5, 3), seq_len=torch.tensor([5, 4]))
    with pytest.raises(_lib.MorganaHipError):
        ops.deltas(torch.zeros(7, 3), ref.DEFAULT_WINDOWS, offsets=torch.tensor([0, 3, 7]), t=4)
    with pytest.raises(RuntimeError, match='no backward'):
        data.compute_deltas(torch.zeros(5, 3, requires_grad=True))
    with pytest.raises(_lib.MorganaHipError):
        data.fit_normalisers([{'lf0': np.zeros((5, 1), np.float32)}], {'lf0': data.MeanVarianceNormaliser('lf0', use_deltas=True)},
                             device='cpu', delta_specs={'lf0': data.DeltaSpec()})


def test_mg_deltas_validates_its_arguments_without_a_gpu():
    import ctypes
    lib = _lib.load()
    fake = 1 << 20                                        # never dereferenced: every call below returns before a launch
    assert lib.mg_deltas_chunk_rows(1) == 256 and lib.mg_deltas_chunk_rows(60) == 34 and lib.mg_deltas_chunk_rows(5000) == 1
    assert lib.mg_deltas_chunk_rows(5) == 51 and lib.mg_deltas_chunk_rows(4) == 512
    assert lib.mg_deltas_chunk_rows(0) == 0
    win_l, win_u, win_c = ops._window_arrays(ref.DEFAULT_WINDOWS)

    def call(x=fake, d=3, b=4, offsets=fake, seq_len=None, t_in=0, n_win=3, l=win_l, u=win_u, c=win_c, edge=0, p0=None, p1=None,
             item_row=None, s=0, kind=-1, form=0, rows=10, raw=fake, norm=None):
        return lib.mg_deltas_f32(x, d, b, offsets, seq_len, t_in, n_win, l, u, c, edge, p0, p1, item_row, s, kind, form, rows, raw, norm, None)

    for rc in (call(offsets=fake, seq_len=fake), call(offsets=None, seq_len=None)):
        assert rc == -1 and 'mg_deltas_f32' in _lib.last_error() and 'exactly one' in _lib.last_error()
    for d in (0, -3):
        assert call(d=d) == -1 and 'mg_deltas_f32: D=' in _lib.last_error()
    for n_win in (0, -1, _lib.MG_MLPG_MAX_WINDOWS + 1):
        assert call(n_win=n_win) == -1 and 'windows supported' in _lib.last_error()
    wide_l, wide_u = (ctypes.c_int * 3)(0, 3, 1), (ctypes.c_int * 3)(0, 2, 1)       # l + u + 1 = 6 coefficients
    assert call(l=wide_l, u=wide_u) == -1 and 'window 1 (l=3, u=2) is wider than 5' in _lib.last_error()
    assert call(l=(ctypes.c_int * 3)(0, -1, 1)) == -1 and 'window 1' in _lib.last_error()
    assert call(l=None) == -1 and call(c=None) == -1
    assert call(edge=2) == -1 and 'edge' in _lib.last_error()
    assert call(form=2) == -1 and 'output form' in _lib.last_error()
    assert call(rows=-1) == -1 and call(b=-1) == -1
    assert call(raw=None, norm=None) == -1 and 'no output' in _lib.last_error()
    assert call(norm=fake) == -1 and 'parameters' in _lib.last_error()
    assert call(norm=fake, p0=fake, p1=fake, kind=_lib.MG_DENORM_MVN) == -1 and 'MG_NORM_MVN' in _lib.last_error()
    assert call(norm=fake, p0=fake, p1=fake, kind=_lib.MG_NORM_MVN, item_row=fake, s=0) == -1 and 'S=0' in _lib.last_error()
    assert call(offsets=None, seq_len=fake, t_in=-1) == -1 and 'T_in' in _lib.last_error()
    assert call(offsets=None, seq_len=fake, t_in=5, form=1, b=_lib.MG_DELTAS_MAX_SCAN_ITEMS + 1) == -1 and 'at most' in _lib.last_error()
    assert call(x=None) == -1 and 'x must not be NULL' in _lib.last_error()
    assert call(x=fake + 2) == -1 and 'aligned' in _lib.last_error()
    assert call(b=0) == 0 and call(b=0, x=None, raw=fake) == 0      # nothing to launch
    assert call(rows=0) == 0                                        # an empty output
    with pytest.raises(ValueError, match='mg_deltas_f32'):
        _lib.check(call(d=0), 'mg_deltas_f32')


# ---------------------------------------------------------------------------------------------------------------- FilesDataset
@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    root = tmp_path_factory.mktemp('deltas_corpus')
    rng = np.random.RandomState(8)
    names = ['utt%d' % i for i in range(4)]
    feats = {}
    for name, frames in zip(names, (1, 2, 3, 25)):
        feats[name] = {'lf0': (rng.randn(frames, 1) * 0.3 + 5.0).astype(np.float32), 'bap': (rng.randn(frames, 5) - 3.0).astype(np.float32)}
        for key, value in feats[name].items():
            os.makedirs(root / 'train' / key, exist_ok=True)
            np.save(root / 'train' / key / (name + '.npy'), value)
    (root / 'ids.scp').write_text('\n'.join(names) + '\n')
    return root, names, feats


def _mvn(rng, name, width):
    return data.MeanVarianceNormaliser(name, use_deltas=True).set_params(
        {'mean': rng.randn(width), 'std_dev': rng.rand(width) + 0.5}, {'mean': rng.randn(3 * width), 'std_dev': rng.rand(3 * width) + 0.5})


def test_files_dataset_computes_deltas_on_the_host(corpus):
    root, names, feats = corpus
    rng = np.random.RandomState(9)
    normalisers = {'lf0': _mvn(rng, 'lf0', 1), 'bap': _mvn(rng, 'bap', 5)}
    sources = {'lf0': data.NumpyBinarySource('lf0', use_deltas=True, deltas='compute'),
               'bap': data.NumpyBinarySource('bap', use_deltas=True, deltas='compute', windows=ref.WINDOWS_5PT, edge='zero')}
    dataset = data.FilesDataset(sources, 'train', 'ids.scp', normalisers, data_root=str(root))
    specs = dataset.delta_specs()
    assert sorted(specs) == ['bap', 'lf0'] and specs['bap'].edge == 'zero' and specs['lf0'].edge == 'replicate'
    assert specs['lf0'].windows == ref.DEFAULT_WINDOWS and specs['bap'].windows == ref.WINDOWS_5PT
    for i, name in enumerate(names):
        raw, item = dataset.raw(i), dataset[i]
        assert sorted(raw) == ['bap', 'lf0', 'name']      # statics only: no _deltas directory exists
        assert sorted(item) == ['bap', 'bap_deltas', 'lf0', 'lf0_deltas', 'name', 'normalised_bap', 'normalised_bap_deltas',
                                'normalised_lf0', 'normalised_lf0_deltas']
        frames = len(feats[name]['lf0'])
        for key, width, windows, edge in (('lf0', 1, ref.DEFAULT_WINDOWS, 'replicate'), ('bap', 5, ref.WINDOWS_5PT, 'zero')):
            deltas = item[key + '_deltas']
            assert deltas.shape == (frames, 3 * width) and deltas.dtype == np.float32
            want = ref.reference(feats[name][key], windows, edge)
            assert not ref.misses(deltas, want, must_be_rounded=ref.exact_windows(windows))
            np.testing.assert_array_equal(deltas[:, :width], feats[name][key])
            twin = item['normalised_' + key + '_deltas']
            assert twin.dtype == np.float32 and twin.shape == deltas.shape
            np.testing.assert_array_equal(twin, normalisers[key].normalise(deltas, deltas=True).astype(np.float32))
    # the default is the reference's behaviour: the _deltas file is read, and missing here
    by_file = data.FilesDataset({'lf0': data.NumpyBinarySource('lf0', use_deltas=True)}, 'train', 'ids.scp', {}, data_root=str(root))
    assert by_file.delta_specs() == {}
    with pytest.raises(FileNotFoundError):
        by_file.raw(0)
    with pytest.raises(ValueError, match='use_deltas'):      # the constructor's check is the reference's, unchanged
        data.FilesDataset({'lf0': data.NumpyBinarySource('lf0')}, 'train', 'ids.scp', {'lf0': normalisers['lf0']}, data_root=str(root))
    with pytest.raises(ValueError, match="'file' or 'compute'"):
        data.NumpyBinarySource('lf0', use_deltas=True, deltas='device')
    with pytest.raises(ValueError, match='use_deltas=True'):
        data.NumpyBinarySource('lf0', deltas='compute')


def test_loaders_take_their_delta_specs_from_the_sources(corpus):
    root, names, feats = corpus
    sources = {'lf0': data.NumpyBinarySource('lf0', use_deltas=True, deltas='compute', edge='zero')}
    dataset = data.FilesDataset(sources, 'train', 'ids.scp', {}, data_root=str(root))
    loader = data.DeviceBatches(dataset, 2, {}, 'cpu')
    assert sorted(loader.delta_specs) == ['lf0'] and loader.delta_specs['lf0'].edge == 'zero'
    assert data.DeviceBatches(dataset, 2, {}, 'cpu', delta_specs={}).delta_specs == {}
    assert data.DeviceBatches([{'name': 'a'}], 2, {}, 'cpu').delta_specs == {}
    assert data.batch(dataset, batch_size=2, shuffle=False, device='cpu').delta_specs['lf0'].edge == 'zero'


def test_a_batch_that_already_carries_the_deltas_is_refused():
    utterances = [{'name': 'a', 'lf0': np.zeros((5, 1), np.float32), 'lf0_deltas': np.zeros((5, 3), np.float32)}]
    with pytest.raises(ValueError, match="'lf0_deltas' is in the utterances and in delta_specs"):
        data.collate_to_device(utterances, {}, 'cpu', delta_specs={'lf0': data.DeltaSpec()})
    with pytest.raises(ValueError, match="'lf0_deltas' is in the utterances and in delta_specs"):
        next(iter(data.DeviceBatches(utterances, 1, {}, 'cpu', delta_specs={'lf0': data.DeltaSpec()})))
    with pytest.raises(KeyError, match='mcep'):
        data.collate_to_device(utterances, {}, 'cpu', delta_specs={'mcep': data.DeltaSpec()})
