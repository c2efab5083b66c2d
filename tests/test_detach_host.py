"""CPU-only checks of the feature-output surface: ``utils.detach_batched_seqs`` (host path), the pure Python helpers and
``viz.io.save_batched_seqs`` against what the reference returned (tests/golden/g19_detach.npz, made by tests/golden/
make_golden_detach.py), the argument validation of ``mg_unpad_rows`` / ``mg_all_nonzero_f32`` through ctypes without a device, and the
chaining of the analysis hooks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import detach_ref
from morgana_amd import _lib, base_models, data, ops, utils
from morgana_amd.viz import io as viz_io


@pytest.fixture(scope='module')
def g19(golden):
    return golden('g19_detach.npz')


_same, check_detach_result = detach_ref.same, detach_ref.check_detach_result


def _call_detach(case, as_torch=True):
    names, kind, squeeze = detach_ref.DETACH_CASES[case]
    x = detach_ref.detach_inputs()
    seq_len = {'tensor': torch.from_numpy(detach_ref.SEQ_LEN.copy()), 'numpy': detach_ref.SEQ_LEN.copy(), 'none': None}[kind]
    feats = [torch.from_numpy(x[n].copy()).requires_grad_(x[n].dtype == np.float32) if as_torch else x[n].copy() for n in names]
    return names, utils.detach_batched_seqs(*feats, seq_len=seq_len, squeeze=squeeze)


@pytest.mark.parametrize('case', sorted(detach_ref.DETACH_CASES))
@pytest.mark.parametrize('as_torch', [True, False])
def test_detach_batched_seqs_host_path_equals_reference(g19, case, as_torch):
    names, got = _call_detach(case, as_torch)
    check_detach_result(g19, case, names, got)


def test_detach_batched_seqs_host_path_clamps_lengths_as_the_device_path_does():
    """A length above T counts as T and a negative one as 0, for CPU tensors and NumPy inputs alike."""
    x = detach_ref.detach_inputs()['f32_3']
    for feature in (torch.from_numpy(x.copy()), x.copy()):
        got = utils.detach_batched_seqs(feature, seq_len=np.array([99, -2, 3, 0]), squeeze=False)
        assert [item.shape for item in got] == [(7, 3), (0, 3), (3, 3), (0, 3)]
        assert np.array_equal(got[0], x[0]) and np.array_equal(got[2], x[2, :3])


def test_golden_covers_the_squeeze_corner_cases(g19):
    """What the cases are there for: np.squeeze of a length-1 item of width 1 is 0-d, of an empty item (0, 1) is (0,), and (B,) /
    (B, D) features come back whole."""
    assert g19['detach__single_w1_sq__0__2'].shape == () and g19['detach__single_w1_sq__0__3'].shape == (0,)
    assert g19['detach__single_w1_nosq__0__2'].shape == (1, 1) and g19['detach__single_w1_nosq__0__3'].shape == (0, 1)
    assert g19['detach__single_sq__0__2'].shape == (3,)
    assert g19['detach__whole__0__whole'].shape == (4,) and g19['detach__whole__1__whole'].shape == (4, 3)
    assert g19['detach__none_len__0__whole'].shape == (4, 7, 3)
    assert g19['detach__multi_sq__1__0'].dtype == np.bool_ and g19['detach__multi_sq__2__0'].dtype == np.int64


def test_pure_python_helpers_equal_reference(g19):
    want = json.loads(str(g19['listify_json']))
    assert [detach_ref.encode(utils.listify(v)) for v in detach_ref.LISTIFY_INPUTS] == want
    same = [1, 2]
    assert utils.listify(same) is same
    assert detach_ref.encode(utils.map_nested(detach_ref.double, detach_ref.nested_input())) == json.loads(str(g19['map_nested_json']))
    mapped = utils.map_nested(lambda t: t + 1, {'t': torch.zeros(2), 'n': [np.zeros(1)]})
    assert torch.equal(mapped['t'], torch.ones(2)) and np.array_equal(mapped['n'][0], np.ones(1))
    got = [utils.get_epoch_from_checkpoint_path(p) for p in detach_ref.CHECKPOINT_PATHS]
    assert got == g19['epochs'].tolist() == [12, 7, 3, 0]


def test_device_only_helpers_refuse_cpu_tensors():
    """batched_masked_select / both_voiced_mask run on the HIP kernels only, as every other op of the package."""
    x = torch.zeros(2, 3, 4)
    with pytest.raises(_lib.MorganaHipError):
        utils.batched_masked_select(x, torch.tensor([3, 2]))
    with pytest.raises(_lib.MorganaHipError):
        utils.both_voiced_mask(x, x)
    with pytest.raises(TypeError):
        utils.batched_masked_select(np.zeros((2, 3, 4)), np.array([3, 2]))


def test_unpad_layout_equals_the_numpy_restatement():
    lens = [37, 0, 1, 36, 17, 99, -3]
    shapes = [(37, 1), (37, 4), (50, 5), (37, 12), (0, 14), (37, 240)]
    blocks, size = ops.unpad_layout(shapes, lens)
    want_blocks, want_size = detach_ref.block_layout(shapes, lens)
    assert blocks == want_blocks and size == want_size
    assert all(off % 64 == 0 for off, _ in blocks) and blocks[1][1] == 37 + 0 + 1 + 36 + 17 + 37 + 0 and blocks[4][1] == 0
    starts, total = detach_ref.item_starts(lens, 37, 5)
    assert starts.tolist() == [0, 185, 185, 190, 370, 455, 640] and total == 640


# ------------------------------------------------------------------------------------------------------------- save_batched_seqs
def test_save_batched_seqs_on_cpu_tensors(tmp_path, g19):
    x = detach_ref.detach_inputs()
    feats = {n: torch.from_numpy(x[n].copy()) for n in ('f32_3', 'f32_1', 'i64_3', 'bool_5')}
    names = ['utt_a', 'utt_b', 'utt_c', 'utt_d']
    seq_len = torch.from_numpy(detach_ref.SEQ_LEN.copy())
    viz_io.save_batched_seqs(feats, names, str(tmp_path), seq_len=seq_len)
    assert sorted(os.listdir(str(tmp_path))) == ['feats']
    assert sorted(os.listdir(str(tmp_path / 'feats'))) == sorted(feats)
    for n in feats:
        assert sorted(os.listdir(str(tmp_path / 'feats' / n))) == [name + '.npy' for name in names]
        for b, name in enumerate(names):
            _same(np.load(str(tmp_path / 'feats' / n / (name + '.npy'))), x[n][b, :detach_ref.SEQ_LEN[b]].squeeze())
    # saved features round-trip through the package's own loader
    loaded = data.NumpyBinarySource('f32_3')('utt_b', str(tmp_path / 'feats'))
    _same(loaded['f32_3'], x['f32_3'][1, :4])

    # feat_names selects a subset of a dict
    sub = tmp_path / 'sub'
    viz_io.save_batched_seqs(feats, names, str(sub), seq_len=seq_len, feat_names=['i64_3'])
    assert os.listdir(str(sub / 'feats')) == ['i64_3']

    # a list needs feat_names; a single feature in a list is saved per utterance, not per frame
    with pytest.raises(ValueError, match='feat_names must be provided'):
        viz_io.save_batched_seqs([feats['f32_3']], names, str(tmp_path / 'bad'), seq_len=seq_len)
    one = tmp_path / 'one'
    viz_io.save_batched_seqs([feats['f32_3']], names, str(one), seq_len=seq_len.numpy(), feat_names=['lf0'])
    assert sorted(os.listdir(str(one / 'feats' / 'lf0'))) == [name + '.npy' for name in names]
    _same(np.load(str(one / 'feats' / 'lf0' / 'utt_a.npy')), x['f32_3'][0])


# ------------------------------------------------------------------------------------------------------------ argument validation
def _descs(n=1, **fields):
    descs = (_lib.mg_unpad_desc * n)()
    for i in range(n):
        descs[i].src, descs[i].T, descs[i].row_bytes, descs[i].dst_offset, descs[i].block_bytes = 4096, 8, 4, 128 * i, 64
    for key, value in fields.items():
        setattr(descs[0], key, value)
    return descs


def _unpad(descs, count, seq_len=8192, b=2, dst=16384, dst_bytes=4096):
    """mg_unpad_rows with fake device addresses: only calls that are refused, or that launch nothing, are made here."""
    return _lib.load().mg_unpad_rows(ctypes.cast(descs, ctypes.c_void_p), count, seq_len, b, dst, dst_bytes, None)


def test_unpad_rows_validates_its_arguments_without_a_gpu():
    assert ctypes.sizeof(_lib.mg_unpad_desc) == 40 and _lib.MG_UNPAD_MAX == 16
    for count in (0, 17, -1):
        assert _unpad(_descs(1), count) == -1 and 'count %d' % count in _lib.last_error()
    assert _unpad(_descs(1, row_bytes=0), 1) == -1 and 'row_bytes=0' in _lib.last_error()
    assert _unpad(_descs(1, row_bytes=-4), 1) == -1 and 'row_bytes=-4' in _lib.last_error()
    assert _unpad(_descs(1, T=-1), 1) == -1 and 'T=-1' in _lib.last_error()
    assert _unpad(_descs(1, dst_offset=8), 1) == -1 and 'dst_offset=8' in _lib.last_error()
    assert _unpad(_descs(1, dst_offset=-16), 1) == -1 and 'dst_offset=-16' in _lib.last_error()
    assert _unpad(_descs(1, block_bytes=-1), 1) == -1 and 'block_bytes=-1' in _lib.last_error()
    assert _unpad(_descs(1, dst_offset=4064), 1) == -1 and 'block_bytes=64' in _lib.last_error() and 'dst_bytes=4096' in _lib.last_error()
    assert _unpad(_descs(2, dst_offset=160), 2) == -1 and 'descriptors 0 and 1 overlap' in _lib.last_error()
    assert _unpad(_descs(1, src=None), 1) == -1 and 'src is NULL' in _lib.last_error()
    assert _unpad(_descs(1), 1, dst=None) == -1 and 'dst is NULL' in _lib.last_error()
    assert _unpad(_descs(1), 1, seq_len=None) == -1 and 'seq_len is NULL' in _lib.last_error()
    assert _unpad(_descs(1), 1, b=-1) == -1 and 'B=-1' in _lib.last_error()
    assert _unpad(_descs(1), 1, b=_lib.MG_UNPAD_MAX_ITEMS + 1) == -1 and 'B=4097' in _lib.last_error()
    assert _unpad(_descs(1, T=1 << 40, row_bytes=1 << 40), 1) == -1 and 'overflows' in _lib.last_error()
    with pytest.raises(ValueError, match='row_bytes=0'):
        _lib.check(_unpad(_descs(1, row_bytes=0), 1), 'mg_unpad_rows')
    # nothing to move: MG_OK without a launch - B == 0, every block empty or smaller than a row, T == 0 (NULL pointers are fine then)
    assert _unpad(_descs(2), 2, b=0, seq_len=None, dst=None) == 0
    empty = _descs(2, block_bytes=0, src=None)
    empty[1].block_bytes = 3
    assert _unpad(empty, 2, seq_len=None, dst=None) == 0
    assert _unpad(_descs(1, T=0, src=None), 1, seq_len=None, dst=None) == 0


def test_all_nonzero_validates_its_arguments_without_a_gpu():
    lib = _lib.load()
    ptrs = (ctypes.c_void_p * 9)(*([4096] * 9))
    xs = ctypes.cast(ptrs, ctypes.c_void_p)
    for count in (0, 9):
        assert lib.mg_all_nonzero_f32(xs, count, 16, 8192, 1, 0, None) == -1 and 'count %d' % count in _lib.last_error()
    assert lib.mg_all_nonzero_f32(None, 1, 16, 8192, 1, 0, None) == -1
    assert lib.mg_all_nonzero_f32(xs, 2, -1, 8192, 1, 0, None) == -1 and 'n=-1' in _lib.last_error()
    assert lib.mg_all_nonzero_f32(xs, 2, 16, 8192, 2, 0, None) == -1 and 'elem_size 2' in _lib.last_error()
    assert lib.mg_all_nonzero_f32(xs, 2, 16, None, 1, 0, None) == -1 and 'out is NULL' in _lib.last_error()
    ptrs[1] = None
    assert lib.mg_all_nonzero_f32(xs, 2, 16, 8192, 1, 0, None) == -1 and 'input 1 is NULL' in _lib.last_error()
    assert lib.mg_all_nonzero_f32(xs, 2, 0, None, 1, 0, None) == 0                                   # nothing to do: no launch
    with pytest.raises(ValueError):
        ops.all_nonzero([], torch.uint8)
    with pytest.raises(_lib.MorganaHipError):
        ops.all_nonzero([torch.zeros(3)], torch.uint8)
    with pytest.raises(_lib.MorganaHipError):
        ops.unpad_rows([torch.zeros(2, 3, 1)], torch.tensor([3, 2]), [3, 2])


# -------------------------------------------------------------------------------------------------------------------- the hooks
def test_valid_and_test_hooks_reach_an_overridden_train_hook():
    class Model(base_models.BaseModel):
        def __init__(self):
            super(Model, self).__init__()
            self.seen = []

        def analysis_for_train_batch(self, features, output_features, out_dir, **kwargs):
            self.seen.append(('batch', features, output_features, out_dir, kwargs))

        def analysis_for_train_epoch(self, out_dir, **kwargs):
            self.seen.append(('epoch', out_dir, kwargs))

    model = Model()
    model.analysis_for_valid_batch({'f': 1}, {'o': 2}, 'dir', sample_rate=16000)
    model.analysis_for_test_batch({'f': 3}, {'o': 4}, out_dir='dir2')
    model.analysis_for_valid_epoch('dir', x=1)
    model.analysis_for_test_epoch(out_dir='dir2')
    assert model.seen == [('batch', {'f': 1}, {'o': 2}, 'dir', {'sample_rate': 16000}), ('batch', {'f': 3}, {'o': 4}, 'dir2', {}),
                          ('epoch', 'dir', {'x': 1}), ('epoch', 'dir2', {})]


def test_stream_model_hook_saves_every_stream_output(tmp_path):
    """StreamModel.analysis_for_valid_batch on CPU outputs: one file per stream and utterance, cropped to n_frames; the classes of a
    categorical stream, (B, T), are cropped too; a stream without a generated output is skipped; no out_dir or no names: nothing."""
    from morgana_amd import models
    streams = [models.Stream('lf0', 3, 'mse'), models.Stream('vuv', 1, 'sigmoid_bce'), models.Stream('phone', 5, 'ce'),
               models.Stream('bap', 3, 'mse')]
    model = models.StreamModel(torch.nn.Sequential(), streams, generate=False)
    rng = np.random.RandomState(2)
    n_frames = torch.tensor([5, 2, 0])
    outputs = {'lf0': torch.from_numpy(rng.rand(3, 5, 1).astype(np.float32)), 'vuv': torch.from_numpy(rng.rand(3, 5, 1).astype(np.float32)),
               'phone': torch.from_numpy(rng.randint(0, 5, size=(3, 5))), 'normalised_bap_deltas': torch.zeros(3, 5, 3)}
    features = {'name': ['a', 'b', 'c'], 'n_frames': n_frames}
    model.analysis_for_valid_batch(features, outputs, None)
    model.analysis_for_valid_batch({'n_frames': n_frames}, outputs, str(tmp_path / 'unnamed'))
    assert not os.path.exists(str(tmp_path / 'unnamed'))
    model.analysis_for_test_batch(features, outputs, out_dir=str(tmp_path))
    assert sorted(os.listdir(str(tmp_path / 'feats'))) == ['lf0', 'phone', 'vuv']
    for stream in ('lf0', 'vuv', 'phone'):
        for b, name in enumerate(features['name']):
            want = outputs[stream][b, :int(n_frames[b])].numpy()
            _same(np.load(str(tmp_path / 'feats' / stream / (name + '.npy'))), want.squeeze())
