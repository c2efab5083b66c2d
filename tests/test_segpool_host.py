"""utils.pool_segments without a GPU: the long-double restatement (tests/segpool_ref64.py) against the reference's own recorded
split_to_segments arrays, the oracle's split_to_segments on a ragged case and torch float64 autograd; the refusals of the public
interface, the host-side argument validation of the C entry points and the encoder_pooling option of VAEF0Model."""
import numpy as np
import pytest
import torch

import segpool_ref64 as ref
from morgana_amd import _lib, models, utils
from oracle import ref_cpu

F64 = np.float64


def _reduce_padded(split, lens, mode):
    """The padded-block route done right, in float64: (B, S, L, F) reduced over each segment's first ``len`` entries."""
    b, s, _, f = split.shape
    out = np.zeros((b, s, f), dtype=F64)
    for i in range(b):
        for j in range(s):
            n = int(lens[i, j])
            if n > 0:
                block = split[i, j, :n].astype(F64)
                out[i, j] = {'sum': block.sum(0), 'mean': block.mean(0), 'max': block.max(0), 'min': block.min(0)}[mode]
    return out


# ---------------------------------------------------------------------------------------- the restatement against recorded arrays
@pytest.mark.parametrize('case', ['small', 'wide'])
@pytest.mark.parametrize('mode', ref.MODES)
def test_restatement_reduces_the_references_recorded_segments(golden, case, mode):
    g = golden('g14_segments.npz')
    x, lens, split = g[case + '__x'], g[case + '__lens'].reshape(g[case + '__x'].shape[0], -1), g[case + '__split']
    assert (lens == 0).any(), 'the recorded case holds an empty segment'
    got = ref.pool(x, lens, mode)
    want = _reduce_padded(split, lens, mode)
    # float64 against long double on at most L_max terms: 2^-52 relative to the sum of magnitudes covers both roundings
    tol = 2.0 ** -52 * split.shape[2] * np.abs(split).astype(F64).sum(2) + 1e-300
    assert np.all(np.abs(got['value'].astype(F64) - want) <= (0 if mode in ('max', 'min') else tol))
    empty = lens == 0
    assert not got['value'][empty].any() and not np.signbit(got['value'][empty]).any()
    assert np.all(got['index'][empty] == -1) and np.array_equal(got['m'], np.maximum(lens, 0))
    if mode in ('max', 'min'):
        b, s, f = got['index'].shape
        for i, j, k in np.ndindex(b, s, f):
            if lens[i, j] > 0:
                assert x[i, got['index'][i, j, k], k] == got['value'][i, j, k]


@pytest.mark.parametrize('mode', ref.MODES)
def test_restatement_equals_the_oracles_split_on_a_ragged_case(mode):
    rng = np.random.RandomState(11)
    b, t, f = 3, 23, 5
    x = rng.standard_normal((b, t, f)).astype(np.float32)
    lens = np.array([[4, 0, 7, 1, 11], [1, 1, 1, 0, 20], [0, 9, 0, 9, 3]], dtype=np.int64)      # every row sums to T or less
    split = ref_cpu.split_to_segments(x, lens[:, :, None])
    got = ref.pool(x, lens, mode)
    want = _reduce_padded(split, lens, mode)
    tol = 2.0 ** -52 * split.shape[2] * np.abs(split).astype(F64).sum(2) + 1e-300
    assert np.all(np.abs(got['value'].astype(F64) - want) <= (0 if mode in ('max', 'min') else tol))
    assert np.array_equal(ref.frames_read(lens, None, t).sum(1), lens.sum(1))


# ----------------------------------------------------------------------------------------------- the restatement against autograd
def _torch_pool(x, lens, seq_len, mode):
    """The definition composed of torch float64 ops on slices; the extremum through a gather at the lowest frame that holds it."""
    b, t, f = x.shape
    n = ref.valid_frames(seq_len, b, t)
    rows = []
    for i in range(b):
        pos, row = 0, []
        for length in lens[i]:
            length = max(int(length), 0)
            seg = x[i, min(pos, n[i]):min(pos + length, n[i])]
            pos += length
            if seg.shape[0] == 0:
                row.append(torch.zeros(f, dtype=x.dtype))
            elif mode in ('sum', 'mean'):
                row.append(seg.sum(0) if mode == 'sum' else seg.mean(0))
            else:
                best = (seg.max(0) if mode == 'max' else seg.min(0)).values.detach()
                frames = torch.arange(seg.shape[0])[:, None].expand_as(seg)
                first = torch.where(seg.detach() == best, frames, torch.full_like(frames, seg.shape[0])).min(0).values
                row.append(seg.gather(0, first[None, :])[0])
        rows.append(torch.stack(row))
    return torch.stack(rows)


@pytest.mark.parametrize('mode', ref.MODES)
def test_restatement_equals_torch_float64_autograd(mode):
    rng = np.random.RandomState(5)
    b, t, f = 3, 19, 4
    x = rng.standard_normal((b, t, f)).astype(np.float32)
    lens = np.array([[3, 0, 8, -2, 6, 5], [19, 0, 0, 0, 0, 0], [2, 2, 2, 2, 2, 2]], dtype=np.int64)
    seq_len = np.array([19, 11, 30], dtype=np.int64)            # item 0's last segment overhangs T, item 1's one segment is cut by seq_len
    x[0, 4, 1] = x[0, 6, 1] = x[0, 9, 1] = 7.0                   # a tie inside segment 2 of item 0: the lowest frame takes the gradient
    x[0, 5, 2] = x[0, 8, 2] = -7.0
    g = rng.standard_normal((b, lens.shape[1], f)).astype(np.float32)
    got = ref.pool(x, lens, mode, seq_len)
    grad = ref.pool_grad(g, lens, mode, t, seq_len, got['index'])
    tx = torch.tensor(x.astype(F64), requires_grad=True)
    want = _torch_pool(tx, lens, seq_len, mode)
    (want * torch.tensor(g.astype(F64))).sum().backward()
    np.testing.assert_allclose(got['value'].astype(F64), want.detach().numpy(), rtol=1e-14, atol=1e-300)
    np.testing.assert_allclose(grad['grad'].astype(F64), tx.grad.numpy(), rtol=1e-14, atol=0)
    assert got['m'][1, 0] == 11 and got['m'][0, 5] == 2 and got['m'][0, 3] == 0
    if mode == 'max':
        assert got['index'][0, 2, 1] == 4 and grad['grad'][0, 4, 1] == g[0, 2, 1] and grad['grad'][0, 6, 1] == 0
    if mode == 'min':
        assert got['index'][0, 2, 2] == 5 and grad['grad'][0, 5, 2] == g[0, 2, 2] and grad['grad'][0, 8, 2] == 0
    assert not grad['grad'][1, 11:].any() and not grad['grad'][~ref.frames_read(lens, seq_len, t)].any()


def test_restatement_edge_rules():
    x = np.array([[[0.0], [-0.0], [np.nan], [3.0], [np.nan], [-np.inf], [np.inf], [-1.0], [-2.0]]], dtype=np.float32)
    lens = np.array([[2, 3, 2, 2, 0]], dtype=np.int64)
    for mode in ('max', 'min'):
        got = ref.pool(x, lens, mode)
        assert got['index'][0, :, 0].tolist() == [0, 2, 6 if mode == 'max' else 5, 7 if mode == 'max' else 8, -1]
        assert not np.signbit(got['value'][0, 0, 0]) and np.isnan(got['value'][0, 1, 0])
    assert ref.pool(x, lens, 'max')['value'][0, 3, 0] == -1.0             # all negative: the padded block's zeros must not win
    assert ref.pool(-x[:, :2], lens[:, :1], 'max')['index'][0, 0, 0] == 0 and np.signbit(ref.pool(-x[:, :2], lens[:, :1], 'max')['value'][0, 0, 0])
    assert ref.same_bits(np.float32([0.0]), np.float32([0.0])) and not ref.same_bits(np.float32([0.0]), np.float32([-0.0]))


# ------------------------------------------------------------------------------------------------------------ the interface
def test_interface_refusals_need_no_device():
    x, lens = torch.zeros(2, 5, 3), torch.ones(2, 4, 1, dtype=torch.int64)
    with pytest.raises(TypeError):
        utils.pool_segments(x, torch.ones(2, 4, 1))                       # float lengths, as split_to_segments
    with pytest.raises(ValueError):
        utils.pool_segments(x, lens, mode='median')
    with pytest.raises(_lib.MorganaHipError):
        utils.pool_segments(x, lens)                                      # CPU tensors: there is no CPU fallback
    with pytest.raises(_lib.MorganaHipError):
        utils.pool_segments(x, lens, mode='max', seq_len=torch.tensor([5, 3]))


def test_entry_points_validate_their_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.mg_segment_pool_chunk() > 0
    assert (_lib.MG_POOL_SUM, _lib.MG_POOL_MEAN, _lib.MG_POOL_MAX, _lib.MG_POOL_MIN) == (0, 1, 2, 3)
    # (x, strides, seg_lens, seq_len, B, S, T, F, mode, out, arg, stream)
    assert lib.mg_segment_pool_f32(16, 12, 3, 1, 16, None, 2, 4, 5, 3, 4, 16, 16, None) == -1 and 'unknown mode 4' in _lib.last_error()
    assert lib.mg_segment_pool_f32(16, 12, 3, 1, 16, None, 2, 4, 5, 3, -1, 16, 16, None) == -1 and 'unknown mode' in _lib.last_error()
    assert lib.mg_segment_pool_f32(16, 0, 0, 1, 16, None, 2, 4, 5, 0, 0, 16, None, None) == -1 and 'F=0' in _lib.last_error()
    assert lib.mg_segment_pool_f32(16, 12, 3, 1, 16, None, 2, -4, 5, 3, 0, 16, None, None) == -1 and 'negative size' in _lib.last_error()
    assert lib.mg_segment_pool_f32(16, 12, -3, 1, 16, None, 2, 4, 5, 3, 0, 16, None, None) == -1 and 'negative stride' in _lib.last_error()
    assert lib.mg_segment_pool_f32(16, 12, 3, 1, None, None, 2, 4, 5, 3, 0, 16, None, None) == -1 and 'NULL' in _lib.last_error()
    assert lib.mg_segment_pool_f32(16, 12, 3, 1, 16, None, 2, 4, 5, 3, 2, 16, None, None) == -1 and 'arg' in _lib.last_error()
    assert lib.mg_segment_pool_f32(16, 12, 3, 1, 16, None, 2, 12289, 5, 3, 0, 16, None, None) == -1 and 'S=12289' in _lib.last_error()
    assert lib.mg_segment_pool_f32(None, 0, 0, 0, None, None, 0, 4, 5, 3, 1, None, None, None) == 0       # zero work: no launch
    assert lib.mg_segment_pool_f32(None, 0, 0, 0, None, None, 2, 0, 5, 3, 3, None, None, None) == 0
    # (grad_out, seg_lens, seq_len, arg, B, S, T, F, mode, grad, stream)
    assert lib.mg_segment_pool_bwd_f32(16, 16, None, None, 2, 4, 5, 3, 7, 16, None) == -1 and 'unknown mode 7' in _lib.last_error()
    assert lib.mg_segment_pool_bwd_f32(16, 16, None, None, 2, 4, 5, 0, 1, 16, None) == -1 and 'F=0' in _lib.last_error()
    assert lib.mg_segment_pool_bwd_f32(16, 16, None, None, 2, 4, -5, 3, 1, 16, None) == -1 and 'negative size' in _lib.last_error()
    assert lib.mg_segment_pool_bwd_f32(16, 16, None, None, 2, 4, 5, 3, 1, None, None) == -1 and 'NULL' in _lib.last_error()
    assert lib.mg_segment_pool_bwd_f32(16, 16, None, None, 2, 4, 5, 3, 3, 16, None) == -1 and 'arg' in _lib.last_error()
    assert lib.mg_segment_pool_bwd_f32(None, None, None, None, 0, 4, 5, 3, 1, None, None) == 0
    assert lib.mg_segment_pool_bwd_f32(None, None, None, None, 2, 4, 0, 3, 2, None, None) == 0
    with pytest.raises(ValueError):
        _lib.check(lib.mg_segment_pool_f32(16, 12, 3, 1, 16, None, 2, 4, 5, 3, 9, 16, 16, None), 'mg_segment_pool_f32')


def test_bounds_come_from_the_formats():
    """One worked element: the bound of a sum is one float32 rounding of the result plus m float64 roundings of the magnitudes."""
    x = np.array([[[1.0], [2.0], [-4.0]]], dtype=np.float32)
    got = ref.pool(x, np.array([[3]]), 'sum')
    assert got['value'][0, 0, 0] == -1.0 and got['bound'][0, 0, 0] == 2.0 ** -24 + 2.0 ** -149 + 3 * 2.0 ** -52 * 7.0
    got = ref.pool(x, np.array([[3]]), 'mean')
    assert got['bound'][0, 0, 0] == 2.0 ** -24 / 3 + 2.0 ** -149 + 2.0 ** -52 * 7.0
    grad = ref.pool_grad(np.float32([[[3.0]]]), np.array([[3]]), 'mean', 3)
    assert np.all(grad['grad'] == 1.0) and np.all(grad['bound'] == 2.0 ** -24 + 2.0 ** -149 + 2.0 ** -52)


# ---------------------------------------------------------------------------------------------------------------- the model
def test_vae_f0_model_encoder_pooling_option():
    with pytest.raises(ValueError):
        models.VAEF0Model(encoder_pooling='median')
    default = models.VAEF0Model()
    assert default.encoder_pooling == 'last'
    for pooling in ('mean', 'max'):
        model = models.VAEF0Model(encoder_pooling=pooling)
        assert model.encoder_pooling == pooling
        assert list(model.state_dict()) == list(default.state_dict())
        assert [tuple(v.shape) for v in model.state_dict().values()] == [tuple(v.shape) for v in default.state_dict().values()]
