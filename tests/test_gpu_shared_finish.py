"""What the masked losses share (csrc/seq_reduce.h, ops._lengths): the one-workgroup finish beyond its 256 threads, and the size
check of seq_len in the four wrappers that used to check its dtype alone."""
import numpy as np
import pytest
import torch

import ce_ref64
import mdn_ref64
from morgana_amd import _lib, ops
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
B_FINISH = 257                                             # one utterance more than the finish has threads
T_FINISH = 2
SEQ_LEN_FINISH = (1 + (np.arange(B_FINISH) % 2)).astype(np.int64)      # ragged: 1, 2, 1, ...; utterance 256 has one valid frame


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------- 1. more utterances than the finish has threads
# The finish walks b = tid, tid + 256, ... before its tree: utterance 256 is the second one of thread 0.  Each loss is held to the
# reference and bound its family's file uses, and utterance 256 is then moved by an amount the reference knows: the loss must move
# by that utterance's share - a finish that dropped it would not move at all.
def test_mse_finish_beyond_256_utterances():
    rng = np.random.RandomState(11)
    pred = rng.standard_normal((B_FINISH, T_FINISH, 1)).astype(np.float32)
    target = rng.standard_normal((B_FINISH, T_FINISH, 1)).astype(np.float32)
    loss, grad = ops.masked_mse(_dev(pred), _dev(target), _dev(SEQ_LEN_FINISH), want_grad=True)
    want = float(ref_cpu.mse(pred, target, SEQ_LEN_FINISH))
    print('mse B=%d: loss %.9g, float64 mirror %.9g' % (B_FINISH, loss.item(), want))
    np.testing.assert_allclose(loss.item(), want, rtol=1e-5)
    np.testing.assert_allclose(grad.cpu().numpy(), ref_cpu.mse_grad(pred, target, SEQ_LEN_FINISH), rtol=1e-5, atol=1e-12)
    pred2 = pred.copy()
    pred2[256, 0, 0] += 300.0
    loss2, _ = ops.masked_mse(_dev(pred2), _dev(target), _dev(SEQ_LEN_FINISH), want_grad=False)
    d1 = float(pred[256, 0, 0]) - float(target[256, 0, 0])
    d2 = float(pred2[256, 0, 0]) - float(target[256, 0, 0])
    share = (d2 * d2 - d1 * d1) / (1 * B_FINISH * 1)       # n_256 = 1, D = 1
    print('mse B=%d: moved by %.9g, share of utterance 256 %.9g' % (B_FINISH, loss2.item() - loss.item(), share))
    assert abs((loss2.item() - loss.item()) - share) <= 1e-5 * (abs(loss.item()) + abs(loss2.item()))


def test_ce_finish_beyond_256_utterances():
    rng = np.random.RandomState(12)
    pred = (3.0 * rng.standard_normal((B_FINISH, T_FINISH, 3))).astype(np.float32)
    target = rng.randint(0, 3, size=(B_FINISH, T_FINISH)).astype(np.int64)
    ref = ce_ref64.ce(pred, target, SEQ_LEN_FINISH)
    loss, grad, argmax = ops.masked_ce(_dev(pred), _dev(target), _dev(SEQ_LEN_FINISH), want_grad=True, want_argmax=True)
    loss_err = abs(loss.item() - ref['loss'])
    grad_err = np.abs(grad.cpu().numpy().astype(np.float64) - ref['grad'])
    print('ce B=%d: loss err %.3e (bound %.3e), worst gradient err / bound %.3f'
          % (B_FINISH, loss_err, ref['loss_bound'], float((grad_err / np.maximum(ref['grad_bound'], 1e-300)).max())))
    assert loss_err <= ref['loss_bound']
    assert np.all(grad_err <= ref['grad_bound'])
    assert np.array_equal(argmax.cpu().numpy(), ref['argmax'])
    # utterance 256's only valid frame, its target's logit 60 lower: the loss gains that frame's change / (n_256 B)
    pred2 = pred.copy()
    pred2[256, 0, target[256, 0]] -= 60.0
    ref2 = ce_ref64.ce(pred2, target, SEQ_LEN_FINISH)
    loss2, _, _ = ops.masked_ce(_dev(pred2), _dev(target), _dev(SEQ_LEN_FINISH), want_grad=False)
    share = ref2['loss'] - ref['loss']
    assert share == pytest.approx((ref2['frame_loss'][256, 0] - ref['frame_loss'][256, 0]) / B_FINISH, rel=1e-9)
    bound = ref['loss_bound'] + ref2['loss_bound']
    print('ce B=%d: moved by %.9g, share of utterance 256 %.9g (bound %.3e)' % (B_FINISH, loss2.item() - loss.item(), share, bound))
    assert abs(share) > 100 * bound                        # the move stands clear of the rounding it is measured in
    assert abs((loss2.item() - loss.item()) - share) <= bound


def test_mdn_finish_beyond_256_utterances():
    rng = np.random.RandomState(13)
    k, d = 1, 1
    target = (1.5 * rng.standard_normal((B_FINISH, T_FINISH, d))).astype(np.float32)
    pred = np.concatenate([rng.standard_normal((B_FINISH, T_FINISH, k)), target + 0.5 * rng.standard_normal((B_FINISH, T_FINISH, d)),
                           -0.5 + 0.1 * rng.standard_normal((B_FINISH, T_FINISH, d))], axis=2).astype(np.float32)
    ref = mdn_ref64.mdn(pred, target, SEQ_LEN_FINISH, k)
    loss, grad = ops.masked_mdn(_dev(pred), _dev(target), _dev(SEQ_LEN_FINISH), k, want_grad=True)
    loss_err = abs(loss.item() - ref['loss'])
    grad_err = np.abs(grad.cpu().numpy().astype(np.float64) - ref['grad'])
    print('mdn B=%d: loss err %.3e (bound %.3e), worst gradient err / bound %.3f'
          % (B_FINISH, loss_err, ref['loss_bound'], float((grad_err / np.maximum(ref['grad_bound'], 1e-300)).max())))
    assert loss_err <= ref['loss_bound']
    assert np.all(grad_err <= ref['grad_bound'])
    assert np.all(grad.cpu().numpy()[~ref['mask']] == 0.0)
    # utterance 256's only valid frame, its target three units further from the mean: the loss gains that frame's change / (n_256 B)
    target2 = target.copy()
    target2[256, 0, 0] += 3.0 if target[256, 0, 0] >= pred[256, 0, 1] else -3.0
    ref2 = mdn_ref64.mdn(pred, target2, SEQ_LEN_FINISH, k)
    loss2, _ = ops.masked_mdn(_dev(pred), _dev(target2), _dev(SEQ_LEN_FINISH), k, want_grad=False)
    share = ref2['loss'] - ref['loss']
    assert share == pytest.approx((ref2['frame_loss'][256, 0] - ref['frame_loss'][256, 0]) / B_FINISH, rel=1e-9)
    bound = ref['loss_bound'] + ref2['loss_bound']
    print('mdn B=%d: moved by %.9g, share of utterance 256 %.9g (bound %.3e)' % (B_FINISH, loss2.item() - loss.item(), share, bound))
    assert abs(share) > 100 * bound
    assert abs((loss2.item() - loss.item()) - share) <= bound


# ------------------------------------------------------------------------------------------------------- 2. the size of seq_len
# The kernels read seq_len[b] for every b < B: a shorter tensor would be read past its end.  B = 2, T = 3, D = 1.
def _size_cases():
    rng = np.random.RandomState(14)
    pred = _dev(rng.standard_normal((2, 3, 1)).astype(np.float32))
    target = _dev(rng.standard_normal((2, 3, 1)).astype(np.float32))
    classes = _dev(np.zeros((2, 3), dtype=np.int64))
    return {
        'masked_mse': lambda sl: ops.masked_mse(pred, target, sl, want_grad=True),
        'stream_loss': lambda sl: ops.stream_loss(pred, [target], ['mse'], sl, want_grad=True),
        'masked_ce': lambda sl: ops.masked_ce(pred, classes, sl, want_grad=True),
        'stream_loss_ce': lambda sl: ops.stream_loss_ce(pred, [classes], ['ce'], [1], sl, want_grad=True),
    }


@pytest.mark.parametrize('name', ['masked_mse', 'stream_loss', 'masked_ce', 'stream_loss_ce'])
def test_seq_len_with_fewer_than_b_lengths_is_refused_before_any_launch(name):
    call = _size_cases()[name]
    calls = []
    _lib.CALL_LOG = calls
    try:
        with pytest.raises(ValueError, match='seq_len'):
            call(_dev(np.array([2], dtype=np.int64)))
    finally:
        _lib.CALL_LOG = None
    assert calls == [], calls


@pytest.mark.parametrize('name', ['masked_mse', 'stream_loss', 'masked_ce', 'stream_loss_ce'])
def test_seq_len_as_a_column_gives_the_bits_of_its_flat_view(name):
    call = _size_cases()[name]
    column = _dev(np.array([[3], [2]], dtype=np.int64))
    flat, tall = call(column.view(2)), call(column)
    for a, b in zip(flat, tall):
        if isinstance(a, torch.Tensor):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
