"""GPU tests of the ragged pack (csrc/unpad.hip) and what stands on it: ``mg_unpad_rows`` against the NumPy restatement of its layout
(tests/detach_ref.py) over the alignments a copy can meet, ``utils.detach_batched_seqs`` / ``batched_masked_select`` /
``both_voiced_mask`` against the reference's formulations, and the files ``ExperimentBuilder`` writes through the models' analysis
hook.  Every comparison is bit equality: the kernels move or compare bits."""
import ctypes
import os

import numpy as np
import pytest
import torch

import detach_ref
from morgana_amd import _lib, data, experiment_builder, models, ops, synthetic, utils

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
LENS = [37, 0, 1, 36, 17]

# row_bytes 1, 4, 5, 12, 14, 240, 8, 24
MATRIX = [(np.bool_, 1), (np.float32, 1), (np.bool_, 5), (np.float32, 3), (np.float16, 7), (np.float32, 60), (np.int64, 1), (np.float64, 3)]


def _array(rng, dtype, shape):
    if dtype == np.bool_:
        return rng.random_sample(shape) > 0.5
    if np.issubdtype(dtype, np.integer):
        return rng.randint(-2 ** 40, 2 ** 40, size=shape).astype(dtype)
    return rng.standard_normal(shape).astype(dtype)


def _run(arrays, lens_dev, lens_host):
    """ops.unpad_rows on device copies; returns (packed bytes as numpy, blocks)."""
    tensors = [torch.from_numpy(a).to(DEV) for a in arrays]
    buf, blocks = ops.unpad_rows(tensors, torch.tensor(lens_dev, dtype=torch.int64, device=DEV), lens_host)
    return buf.cpu().numpy(), blocks


def _check_blocks(got, blocks, arrays, lens):
    want, want_blocks = detach_ref.pack(arrays, lens)
    assert blocks == want_blocks
    for a, (off, rows) in zip(arrays, blocks):
        n = rows * detach_ref.row_bytes(a)
        assert np.array_equal(got[off:off + n], want[off:off + n]), (a.dtype, a.shape)


@pytest.mark.parametrize('lens', [LENS, [0, 0, 0, 0, 0], [99, -4, 37, 38, -1]], ids=['ragged', 'empty', 'clamped'])
def test_unpad_rows_alignment_matrix(lens):
    """All eight row sizes in ONE launch, B=5, T=37: with row_bytes 1, 5, 12, 14 and odd lengths the items start at arbitrary
    alignments in the destination, and the source rows at others."""
    rng = np.random.RandomState(7)
    arrays = [_array(rng, dt, (5, 37, w)) for dt, w in MATRIX]
    got, blocks = _run(arrays, lens, lens)
    _check_blocks(got, blocks, arrays, lens)


def test_unpad_rows_single_item_and_two_padded_axes():
    rng = np.random.RandomState(8)
    one = [_array(rng, dt, (1, 37, w)) for dt, w in MATRIX]
    got, blocks = _run(one, [23], [23])
    _check_blocks(got, blocks, one, [23])
    # features with different T in one launch: each clamps the lengths to its own axis
    pair = [_array(rng, np.float32, (5, 37, 3)), _array(rng, np.float16, (5, 50, 7)), _array(rng, np.bool_, (5, 50, 1))]
    lens = [50, 0, 41, 37, 17]
    got, blocks = _run(pair, lens, lens)
    assert [rows for _, rows in blocks] == [37 + 37 + 37 + 17, 50 + 41 + 37 + 17, 50 + 41 + 37 + 17]
    _check_blocks(got, blocks, pair, lens)


def test_unpad_rows_seventeen_features_take_two_launches():
    rng = np.random.RandomState(9)
    arrays = [_array(rng, MATRIX[k % 8][0], (5, 37, MATRIX[k % 8][1])) for k in range(17)]
    log = _lib.CALL_LOG = []
    try:
        got, blocks = _run(arrays, LENS, LENS)
    finally:
        _lib.CALL_LOG = None
    assert log.count('mg_unpad_rows') == 2
    _check_blocks(got, blocks, arrays, LENS)


def test_unpad_rows_items_straddle_chunk_boundaries():
    """B=3, T=700, D=60 float32: 240-byte rows, items of 168,000 / 79,920 / 167,760 bytes against 16 KiB chunks of the destination."""
    rng = np.random.RandomState(10)
    arrays = [_array(rng, np.float32, (3, 700, 60)), _array(rng, np.bool_, (3, 700, 5))]
    lens = [700, 333, 699]
    got, blocks = _run(arrays, lens, lens)
    _check_blocks(got, blocks, arrays, lens)


def test_unpad_rows_four_byte_path_on_a_destination_that_is_not_four_aligned():
    """row_bytes = 2 (float16 x1) with odd lengths, T=37: item 1 starts at destination byte 70 and source byte 74 - congruent modulo 4
    but not modulo 16, and not 4-aligned: the 4-byte body with bytes in front of it (items 3 and 4: the same with other heads)."""
    rng = np.random.RandomState(17)
    arrays = [_array(rng, np.float16, (5, 37, 1)), _array(rng, np.int16, (5, 37, 1))]
    lens = [35, 3, 37, 1, 36]
    assert (35 * 2) % 4 == 2 and ((35 * 2) ^ (37 * 2)) % 4 == 0 and ((35 * 2) ^ (37 * 2)) % 16 != 0
    got, blocks = _run(arrays, lens, lens)
    _check_blocks(got, blocks, arrays, lens)


def test_unpad_rows_more_items_than_one_launch_scans():
    """B = 4100 > MG_UNPAD_MAX_ITEMS: ops.unpad_rows packs in groups of 4096 items, each behind the rows of the groups before it;
    detach_batched_seqs and batched_masked_select work at any batch size, as the reference does."""
    rng = np.random.RandomState(18)
    b = _lib.MG_UNPAD_MAX_ITEMS + 4
    lens = rng.randint(0, 5, size=b).tolist()
    lens[-3:] = [3, 0, 2]
    arrays = [_array(rng, np.float32, (b, 4, 3)), _array(rng, np.bool_, (b, 4, 5))]
    got, blocks = _run(arrays, lens, lens)
    _check_blocks(got, blocks, arrays, lens)
    x = torch.from_numpy(arrays[0]).to(DEV)
    items = utils.detach_batched_seqs(x, seq_len=np.array(lens), squeeze=False)
    assert len(items) == b and all(np.array_equal(item, arrays[0][k, :min(lens[k], 4)]) for k, item in enumerate(items))
    seq_len = torch.tensor(lens, device=DEV)
    assert torch.equal(utils.batched_masked_select(x, seq_len), _reference_select(x, seq_len))


def test_unpad_rows_never_writes_outside_its_blocks():
    """Blocks sized from SHORTER lengths than the device seq_len holds, 64 guard bytes behind each, everything pre-filled with 0xA5:
    the guards and the next block's head stay untouched and every block holds the head of the expected stream."""
    rng = np.random.RandomState(11)
    arrays = [_array(rng, dt, (5, 37, w)) for dt, w in MATRIX]
    sized_from, on_device = [20, 0, 1, 10, 5], [37, 9, 30, 36, 37]
    blocks, size = detach_ref.block_layout([(a.shape[1], detach_ref.row_bytes(a)) for a in arrays], sized_from, guard=64)
    tensors = [torch.from_numpy(a).to(DEV) for a in arrays]
    dst = torch.full((size,), 0xA5, dtype=torch.uint8, device=DEV)
    seq_len = torch.tensor(on_device, dtype=torch.int64, device=DEV)
    descs = (_lib.mg_unpad_desc * len(arrays))()
    for i, (t, a, (off, rows)) in enumerate(zip(tensors, arrays, blocks)):
        descs[i].src, descs[i].T, descs[i].row_bytes = t.data_ptr(), a.shape[1], detach_ref.row_bytes(a)
        descs[i].dst_offset, descs[i].block_bytes = off, rows * detach_ref.row_bytes(a)
    _lib.check(_lib.load().mg_unpad_rows(ctypes.cast(descs, ctypes.c_void_p), len(arrays), ops._p(seq_len), 5, ops._p(dst), size,
                                         ops._stream()), 'mg_unpad_rows')
    got = dst.cpu().numpy()
    want = np.full(size, 0xA5, np.uint8)
    for a, (off, rows) in zip(arrays, blocks):
        n = rows * detach_ref.row_bytes(a)
        want[off:off + n] = detach_ref.packed_stream(a, on_device)[:n]
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------- detach_batched_seqs
def _assert_same_structure(got, want):
    if isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want)
        for g, w in zip(got, want):
            _assert_same_structure(g, w)
    else:
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got, want, equal_nan=want.dtype.kind == 'f')


@pytest.mark.parametrize('case', sorted(detach_ref.DETACH_CASES))
def test_detach_batched_seqs_on_device_tensors_equals_reference(golden, case):
    g19 = golden('g19_detach.npz')
    names, kind, squeeze = detach_ref.DETACH_CASES[case]
    x = detach_ref.detach_inputs()
    seq_len = {'tensor': torch.from_numpy(detach_ref.SEQ_LEN.copy()).to(DEV), 'numpy': detach_ref.SEQ_LEN.copy(), 'none': None}[kind]
    feats = [torch.from_numpy(x[n].copy()).to(DEV).requires_grad_(x[n].dtype == np.float32) for n in names]
    detach_ref.check_detach_result(g19, case, names, utils.detach_batched_seqs(*feats, seq_len=seq_len, squeeze=squeeze))


def test_detach_batched_seqs_equals_the_call_on_cpu_copies():
    rng = np.random.RandomState(12)
    feats = [torch.from_numpy(_array(rng, dt, (5, 37, w))).to(DEV) for dt, w in MATRIX]
    feats.append(torch.from_numpy(_array(rng, np.float32, (5, 4))).to(DEV))                          # (B, D): comes back whole
    feats.append(torch.from_numpy(_array(rng, np.float32, (5, 37, 2, 3))).to(DEV))                   # two trailing axes
    feats.append(torch.from_numpy(_array(rng, np.float32, (5, 37, 6))).to(DEV).requires_grad_(True) * 2.0)   # needs grad, not a leaf
    feats.append(torch.from_numpy(_array(rng, np.float32, (5, 8, 37))).to(DEV).transpose(1, 2))      # non-contiguous
    feats.append(torch.from_numpy(_array(rng, np.float32, (5, 37, 3))))                              # a CPU tensor among them
    assert not feats[-2].is_contiguous()
    lens = torch.tensor(LENS)
    for seq_len in (lens.to(DEV), lens, lens.numpy(), lens.to(DEV).int()):
        for squeeze in (True, False):
            want = utils.detach_batched_seqs(*[f.cpu() for f in feats], seq_len=lens, squeeze=squeeze)
            _assert_same_structure(utils.detach_batched_seqs(*feats, seq_len=seq_len, squeeze=squeeze), want)
    single = utils.detach_batched_seqs(feats[3], seq_len=lens.to(DEV))
    _assert_same_structure(single, utils.detach_batched_seqs(feats[3].cpu(), seq_len=lens))


def test_detach_batched_seqs_results_survive_later_calls():
    """The arrays are copies out of the reused pinned staging buffer: a second (and third: the buffers take turns) call with other
    data leaves the first call's results as they were."""
    rng = np.random.RandomState(13)
    first_np = _array(rng, np.float32, (5, 37, 60))
    first = utils.detach_batched_seqs(torch.from_numpy(first_np).to(DEV), seq_len=torch.tensor(LENS, device=DEV))
    kept = [a.copy() for a in first]
    for _ in range(3):
        utils.detach_batched_seqs(torch.from_numpy(_array(rng, np.float32, (5, 37, 60))).to(DEV), seq_len=torch.tensor(LENS, device=DEV))
    for b, (a, k) in enumerate(zip(first, kept)):
        want = first_np[b, :LENS[b]].squeeze()               # squeeze=True: the length-1 item comes back as (60,)
        assert a.shape == want.shape and np.array_equal(a, k) and np.array_equal(a, want)


def test_detach_batched_seqs_refuses_bfloat16_before_any_launch():
    x = torch.zeros(5, 37, 3, dtype=torch.bfloat16, device=DEV)
    log = _lib.CALL_LOG = []
    try:
        with pytest.raises(TypeError):
            utils.detach_batched_seqs(torch.zeros(5, 37, 3, device=DEV), x, seq_len=torch.tensor(LENS, device=DEV))
    finally:
        _lib.CALL_LOG = None
    assert log == []


# ----------------------------------------------------------------------------------------------------- batched_masked_select
def _reference_select(x, seq_len):
    mask = (torch.arange(x.shape[1], device=x.device)[None, :] < seq_len[:, None]).long()
    return x[mask.nonzero(as_tuple=True)]


@pytest.mark.parametrize('dtype,width', MATRIX)
def test_batched_masked_select_equals_the_reference_formulation(dtype, width):
    rng = np.random.RandomState(14)
    x = torch.from_numpy(_array(rng, dtype, (5, 37, width))).to(DEV)
    seq_len = torch.tensor(LENS, device=DEV)
    got = utils.batched_masked_select(x, seq_len)
    want = _reference_select(x, seq_len)
    assert got.dtype == want.dtype and got.shape == want.shape and got.device == x.device
    assert torch.equal(got.view(torch.uint8), want.contiguous().view(torch.uint8))
    assert torch.equal(utils.batched_masked_select(x, np.array(LENS)).view(torch.uint8), want.contiguous().view(torch.uint8))


def test_batched_masked_select_against_golden_and_its_gradient(golden):
    g19 = golden('g19_detach.npz')
    x = detach_ref.detach_inputs()
    seq_len = torch.from_numpy(detach_ref.SEQ_LEN.copy()).to(DEV)
    for name in detach_ref.SELECT_CASES:
        got = utils.batched_masked_select(torch.from_numpy(x[name].copy()).to(DEV), seq_len).cpu().numpy()
        want = g19['select__' + name]
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    # d (sum of w * selected) / d x = w scattered into a zero-padded tensor, bit for bit
    rng = np.random.RandomState(15)
    for lens in (LENS, [0, 0, 0, 0, 0]):
        xt = torch.from_numpy(_array(rng, np.float32, (5, 37, 60))).to(DEV).requires_grad_(True)
        lens_t = torch.tensor(lens, device=DEV)
        out = utils.batched_masked_select(xt, lens_t)
        w = torch.from_numpy(_array(rng, np.float32, tuple(out.shape))).to(DEV)
        (grad,) = torch.autograd.grad((out * w).sum(), xt)
        want = torch.zeros_like(xt)
        mask = (torch.arange(37, device=DEV)[None, :] < lens_t[:, None])
        want[mask] = w
        assert torch.equal(grad, want)


# ---------------------------------------------------------------------------------------------------------- both_voiced_mask
@pytest.mark.parametrize('n_inputs', [1, 2, 8])
@pytest.mark.parametrize('shape', [(5, 37, 1), (4, 64, 4)], ids=['odd', 'vector'])
def test_both_voiced_mask_equals_the_torch_formulation(n_inputs, shape):
    rng = np.random.RandomState(16 + n_inputs)
    xs = []
    for k in range(n_inputs):
        a = rng.standard_normal(shape).astype(np.float32)
        flat = a.reshape(-1)
        flat[rng.randint(0, flat.size, size=flat.size // 8)] = 0.0
        flat[k::17], flat[k + 3::19], flat[k + 5::23] = 0.0, -0.0, np.nan
        xs.append(torch.from_numpy(a).to(DEV))
    for dtype in (torch.ByteTensor, torch.uint8, torch.bool, torch.float32, torch.int64, torch.FloatTensor):
        got = utils.both_voiced_mask(*xs, dtype=dtype)
        want = torch.prod(torch.stack([~torch.eq(x, 0.) for x in xs]), dim=0).to(utils._as_dtype(dtype))
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)
    assert 0 < int(utils.both_voiced_mask(*xs, dtype=torch.int64).sum()) < xs[0].numel()


def test_both_voiced_mask_against_golden(golden):
    g19 = golden('g19_detach.npz')
    x = detach_ref.detach_inputs()
    dtypes = {'uint8': torch.ByteTensor, 'bool': torch.bool, 'float32': torch.float32}
    for case, names in detach_ref.VOICED_CASES.items():
        for key, dtype in dtypes.items():
            got = utils.both_voiced_mask(*[torch.from_numpy(x[n].copy()).to(DEV) for n in names], dtype=dtype).cpu().numpy()
            want = g19['voiced__%s__%s' % (case, key)]
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_valid_and_test_epochs_write_every_stream_per_utterance(tmp_path):
    """GRUF0Model (the smallest StreamModel tests/test_gpu_configs.py builds), B=3, T<=40, ragged: after valid_epoch(gen_output=True) and
    test_epoch every stream has feats/<stream>/<name>.npy, equal to the stream's output of a direct predict cropped to n_frames."""
    feats_np = synthetic.make_acoustic_batch(3, (20, 40), streams=(('lf0', 3, 'mse'),), seed=21, with_raw=True)
    feats = data.to_device(feats_np, DEV)
    torch.manual_seed(4)
    builder = experiment_builder.ExperimentBuilder(models.GRUF0Model, dict(precision='fp32'), device=DEV)
    synthetic.acoustic_normalisers(builder.model, device=DEV)
    n_frames = feats_np['n_frames']
    assert feats_np['normalised_counters'].shape[1] <= 40 and len(set(n_frames.tolist())) > 1
    with torch.no_grad():
        want = builder.model.predict(feats)['lf0'].cpu().numpy()
    valid_dir, test_dir = str(tmp_path / 'valid'), str(tmp_path / 'test')
    builder.valid_epoch([feats], gen_output=True, out_dir=valid_dir)
    builder.test_epoch([feats], out_dir=test_dir)
    for out_dir in (valid_dir, test_dir):
        assert os.listdir(os.path.join(out_dir, 'feats')) == ['lf0']
        for b, name in enumerate(feats_np['name']):
            got = np.load(os.path.join(out_dir, 'feats', 'lf0', name + '.npy'))
            assert got.dtype == np.float32 and np.array_equal(got, want[b, :n_frames[b]].squeeze())


def test_acoustic_model_hook_saves_trajectories_probabilities_and_classes(tmp_path):
    """A stream table with all three kinds of output (delta trajectory, probability, class) through the hook on device outputs."""
    feats_np = synthetic.make_acoustic_batch(3, (20, 40), seed=22, with_raw=True)
    feats = data.to_device(feats_np, DEV)
    torch.manual_seed(5)
    model = models.LSTMAcousticModel(precision='fp32', num_layers=2).to(DEV)
    synthetic.acoustic_normalisers(model, device=DEV)
    with torch.no_grad():
        outputs = model.predict(feats)
    outputs['phone'] = torch.argmax(outputs['normalised_mcep_deltas'], dim=-1)                      # (B, T) int64, as a 'ce' stream's classes
    model.streams = model.streams + (models.Stream('phone', 180, 'ce'),)
    model.analysis_for_test_batch(feats, outputs, out_dir=str(tmp_path))
    n_frames = feats_np['n_frames']
    assert sorted(os.listdir(str(tmp_path / 'feats'))) == ['bap', 'lf0', 'mcep', 'phone', 'vuv']
    for stream in ('lf0', 'vuv', 'mcep', 'bap', 'phone'):
        want = outputs[stream].cpu().numpy()
        for b, name in enumerate(feats_np['name']):
            got = np.load(str(tmp_path / 'feats' / stream / (name + '.npy')))
            assert got.dtype == want.dtype and np.array_equal(got, want[b, :n_frames[b]].squeeze())
