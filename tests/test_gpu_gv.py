"""losses.gv on the device (run with ``-m gpu`` on an MI355X): mg_gv_f32 / mg_gv_bwd_f32 against the long-double restatement of
tests/gv_ref64.py inside its derived bounds (the cases and bounds are that module's; tests/test_gv_host.py shows they are honest),
bit equality across layouts, the semantics of pad frames and short utterances, determinism, graph replay, and the global-variance
term of models.Stream on the shipped F0 model."""
import functools

import numpy as np
import pytest
import torch

import gv_ref64 as ref
from morgana_amd import _lib, data, losses, models, ops, synthetic

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GRAD_SCALE = 0.75


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def lengths(seq_len):
    return None if seq_len is None else torch.tensor(seq_len, dtype=torch.int64, device=DEV)


@functools.lru_cache(maxsize=None)
def chunk():
    return _lib.load().mg_gv_chunk_frames()


def run(pred, tgt, seq_len=None, log=True, eps=1e-6, grad_scale=GRAD_SCALE):
    """(loss 0-d, grad (B, T, D)) of losses.gv through autograd; pred / tgt are device tensors, used as they are (layout included)."""
    pred = pred.detach().requires_grad_()
    loss = losses.gv(pred, tgt, seq_len, log=log, eps=eps)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    (grad,) = torch.autograd.grad(loss * grad_scale, pred)
    return loss.detach(), grad


def assert_same_bits(got, want):
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------------------------------------------------- 1. bounds
@pytest.mark.parametrize('log', [True, False], ids=['log', 'linear'])
@pytest.mark.parametrize('kind', ref.SEQ_LENS, ids=['head', 'tail', 'none'])
@pytest.mark.parametrize('d', [1, 5, 60, 67])
def test_loss_and_gradient_inside_the_derived_bounds(d, kind, log):
    pred, tgt = ref.case(chunk(), d)
    seq_len = ref.seq_len_case(kind, chunk())
    want = ref.gv(pred, tgt, seq_len, log=log, grad_scale=GRAD_SCALE)
    loss, grad = run(dev(pred), dev(tgt), lengths(seq_len), log=log)
    loss, grad = loss.item(), grad.cpu().numpy()
    ref.report('D=%d seq_len=%s log=%s' % (d, kind, log), want, loss, grad)
    assert np.isfinite(grad).all() and np.abs(want['grad']).max() > 0
    assert abs(loss - want['loss']) <= want['loss_bound']
    assert np.all(np.abs(grad.astype(np.float64) - want['grad']) <= want['grad_bound'])
    assert not grad[~want['mask']].any() and not np.signbit(grad[~want['mask']]).any()      # pad frames: +0.0 exactly


@pytest.mark.parametrize('log', [True, False], ids=['log', 'linear'])
def test_offset_column(log):
    """A column at 16384 with standard deviation 2^-6 next to an lf0-like one at 5 +- 0.25: a sum of raw squares misses this bound by
    orders of magnitude (tests/test_gv_host.py asserts it on the same input)."""
    pred, tgt = ref.offset_case(chunk())
    want = ref.gv(pred, tgt, None, log=log, grad_scale=GRAD_SCALE)
    loss, grad = run(dev(pred), dev(tgt), None, log=log)
    loss, grad = loss.item(), grad.cpu().numpy()
    ref.report('offset log=%s' % log, want, loss, grad)
    assert abs(loss - want['loss']) <= want['loss_bound']
    assert np.all(np.abs(grad.astype(np.float64) - want['grad']) <= want['grad_bound'])
    got_v = losses.global_variance(dev(tgt)).cpu().numpy()
    v, bound = ref.variance_bound(tgt)
    assert np.all(np.abs(got_v.astype(np.float64) - v) <= bound)


# ------------------------------------------------------------------------------------------------------------------ 2. bit equality
@pytest.mark.parametrize('d', [5, 60, 67])
def test_layouts_give_the_bits_of_the_contiguous_tensor(d):
    pred_np, tgt_np = ref.case(chunk(), d, seed=1)
    seq_len = lengths(ref.seq_len_case('tail', chunk()))
    pred, tgt = dev(pred_np), dev(tgt_np)
    b, t, _ = pred.shape
    want = run(pred, tgt, seq_len)
    # a column slice of a wider tensor (both operands)
    wide_p, wide_y = torch.randn(b, t, d + 7, device=DEV), torch.randn(b, t, d + 9, device=DEV)
    wide_p[:, :, 3:3 + d] = pred
    wide_y[:, :, 2:2 + d] = tgt
    assert_same_bits(run(wide_p[:, :, 3:3 + d], wide_y[:, :, 2:2 + d], seq_len), want)
    # a base that is 1, 2 and 3 floats off a 16-byte boundary, rows still contiguous
    for off in (1, 2, 3):
        flat_p, flat_y = torch.zeros(pred.numel() + 4, device=DEV), torch.zeros(tgt.numel() + 4, device=DEV)
        view_p, view_y = flat_p[off:off + pred.numel()].view(b, t, d), flat_y[4 - off:4 - off + tgt.numel()].view(b, t, d)
        view_p.copy_(pred)
        view_y.copy_(tgt)
        assert view_p.data_ptr() % 16 == 4 * off and view_p.is_contiguous()
        assert_same_bits(run(view_p, view_y, seq_len), want)
    # a transposed-stride view: (B, D, T) storage
    trans_p, trans_y = pred.transpose(1, 2).contiguous().transpose(1, 2), tgt.transpose(1, 2).contiguous().transpose(1, 2)
    assert trans_p.stride() == (t * d, 1, t) and torch.equal(trans_p, pred)
    assert_same_bits(run(trans_p, trans_y, seq_len), want)
    assert_same_bits(run(trans_p, tgt, seq_len), want)


@pytest.mark.parametrize('d', [1, 60])
def test_an_expanded_target_gives_the_bits_of_its_copy(d):
    pred_np, tgt_np = ref.case(chunk(), d, seed=2)
    seq_len = lengths(ref.seq_len_case('head', chunk()))
    pred = dev(pred_np)
    one = dev(tgt_np[:1])                                         # one natural utterance for the whole batch: stride_b == 0
    expanded = one.expand(pred.shape[0], -1, -1)
    assert expanded.stride(0) == 0
    assert_same_bits(run(pred, expanded, seq_len), run(pred, expanded.contiguous(), seq_len))
    column = dev(tgt_np[:, :, :1]).expand(-1, -1, d)              # stride_d == 0
    assert column.stride(2) == 0 or d == 1
    assert_same_bits(run(pred, column, seq_len), run(pred, column.contiguous(), seq_len))


# --------------------------------------------------------------------------------------------------------------------- 3. semantics
def test_a_nan_in_a_pad_frame_changes_no_bit():
    pred_np, tgt_np = ref.case(chunk(), 5, seed=3)
    seq_len = ref.seq_len_case('tail', chunk())
    want = run(dev(pred_np), dev(tgt_np), lengths(seq_len))
    past = np.arange(pred_np.shape[1])[None, :] >= np.array(seq_len)[:, None]
    poisoned_p, poisoned_y = pred_np.copy(), tgt_np.copy()
    poisoned_p[past] = np.nan
    poisoned_y[past] = np.inf
    assert_same_bits(run(dev(poisoned_p), dev(poisoned_y), lengths(seq_len)), want)
    trans = dev(poisoned_p).transpose(1, 2).contiguous().transpose(1, 2)       # the generic path
    assert_same_bits(run(trans, dev(poisoned_y), lengths(seq_len)), want)
    v = losses.global_variance(dev(poisoned_p), lengths(seq_len))
    assert torch.equal(v, losses.global_variance(dev(pred_np), lengths(seq_len))) and torch.isfinite(v).all()


def test_an_empty_utterance_gives_nan_on_its_own_frames_only():
    pred_np, tgt_np = ref.case(chunk(), 5, seed=4)
    loss, grad = run(dev(pred_np), dev(tgt_np), lengths([chunk() + 1, 0, 7]))
    assert torch.isnan(loss)
    assert torch.isnan(grad[1]).all() and torch.isfinite(grad[[0, 2]]).all() and grad[0].abs().max() > 0
    assert not grad[2, 7:].any() and not grad[0, chunk() + 1:].any()
    loss, grad = run(dev(pred_np), dev(tgt_np), lengths([chunk() + 1, -3, 7]))       # negative lengths clamp to 0
    assert torch.isnan(loss) and torch.isnan(grad[1]).all()
    v = losses.global_variance(dev(pred_np), lengths([chunk() + 1, 0, 7]))
    assert torch.isnan(v[1]).all() and torch.isfinite(v[[0, 2]]).all()


@pytest.mark.parametrize('log', [True, False], ids=['log', 'linear'])
def test_one_valid_frame_gives_finite_results_and_a_zero_gradient(log):
    pred_np, tgt_np = ref.case(chunk(), 5, seed=5)
    seq_len = [1, 1, chunk() + 2]
    want = ref.gv(pred_np, tgt_np, seq_len, log=log, grad_scale=GRAD_SCALE)
    loss, grad = run(dev(pred_np), dev(tgt_np), lengths(seq_len), log=log)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    assert not grad[:2].any() and grad[2].abs().max() > 0
    assert abs(loss.item() - want['loss']) <= want['loss_bound']
    only = run(dev(pred_np), dev(tgt_np), lengths([1, 1, 1]), log=log)      # v == 0 on both sides everywhere
    assert only[0].item() == 0.0 and not only[1].any()


def test_global_variance():
    pred_np, _ = ref.case(chunk(), 67, seed=6)
    pred_np[:, :, 3] = 2.5                                        # constant columns: exactly 0
    pred_np[:, :, 66] = -16384.25
    for kind in ref.SEQ_LENS:
        seq_len = ref.seq_len_case(kind, chunk())
        got = losses.global_variance(dev(pred_np), lengths(seq_len))
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, 67) and not got.requires_grad
        got = got.cpu().numpy()
        v, bound = ref.variance_bound(pred_np, seq_len)
        assert np.all(got[:, [3, 66]] == 0.0) and not np.signbit(got[:, [3, 66]]).any()
        assert np.all(np.abs(got.astype(np.float64) - v) <= bound)
        if kind == 'head':
            assert np.all(got[0] == 0.0)                          # one frame
    x = dev(pred_np).requires_grad_()
    assert not losses.global_variance(x).requires_grad
    # the variances of the loss's own pass are the same numbers
    _, _, v_pred, v_tgt = ops.gv(dev(pred_np), dev(pred_np[::-1].copy()), None, want_variances=True)
    assert torch.equal(v_pred, losses.global_variance(dev(pred_np))) and torch.equal(v_tgt, v_pred.flip(0))


def test_targets_get_no_gradient_and_other_dtypes_are_refused():
    pred_np, tgt_np = ref.case(chunk(), 5, seed=7)
    pred, tgt = dev(pred_np).requires_grad_(), dev(tgt_np).requires_grad_()
    losses.gv(pred, tgt).backward()
    assert tgt.grad is None and pred.grad is not None
    with pytest.raises(TypeError, match='float32'):
        losses.gv(pred, tgt.double())
    with pytest.raises(TypeError, match='float32'):
        losses.gv(pred.double(), tgt)
    int_lengths = torch.tensor([5, 9, 2], dtype=torch.int32, device=DEV)
    assert torch.equal(losses.gv(pred, tgt, int_lengths), losses.gv(pred, tgt, int_lengths.long()))


# ------------------------------------------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize('d', [5, 67])
def test_three_calls_give_equal_bits(d):
    pred_np, tgt_np = ref.case(chunk(), d, seed=8)
    pred, tgt, seq_len = dev(pred_np), dev(tgt_np), lengths(ref.seq_len_case('tail', chunk()))
    first = run(pred, tgt, seq_len)
    for _ in range(2):
        assert_same_bits(run(pred, tgt, seq_len), first)


# ------------------------------------------------------------------------------------------------------------------------- 5. graph
def test_graph_replay_equals_the_eager_call():
    rng = np.random.RandomState(9)
    shape = (3, chunk() + 3, 5)
    pred = dev(rng.standard_normal(shape).astype(np.float32)).requires_grad_()
    target = dev(rng.standard_normal(shape).astype(np.float32))
    n = lengths([chunk() + 3, 5, chunk()])
    static_loss, static_grad = torch.empty((), device=DEV), torch.empty(shape, device=DEV)

    def step():
        loss = losses.gv(pred, target, n)
        (grad,) = torch.autograd.grad(loss, pred)
        return loss.detach(), grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grad = step()
        static_loss.copy_(loss)
        static_grad.copy_(grad)
    for seq_len in ([chunk() + 1, 11, 1], [17, chunk() + 3, 3]):           # refreshed inputs, lengths included
        with torch.no_grad():
            pred.copy_(dev(rng.standard_normal(shape).astype(np.float32)))
            target.copy_(dev((2.0 * rng.standard_normal(shape)).astype(np.float32)))
            n.copy_(lengths(seq_len))
        graph.replay()
        torch.cuda.synchronize()
        want_loss, want_grad = step()
        assert torch.isfinite(want_loss) and want_grad.abs().max() > 0
        assert_same_bits((static_loss, static_grad), (want_loss, want_grad))


# ------------------------------------------------------------------------------------------------------------ 6. Stream and the models
@functools.lru_cache(maxsize=None)
def _batch_np():
    return synthetic.make_acoustic_batch(2, (30, 40), streams=(('lf0', 3, 'mse'),), seed=41, with_raw=True)


def _model(speakers=False, **kwargs):
    if speakers:
        kwargs['speaker_id_list'] = 'speakers.scp'
    model = models.GRUF0Model(precision='fp32', **kwargs).to(DEV)
    own = model.state_dict()
    for key, value in synthetic.gru_f0_state().items():
        own[key].copy_(torch.from_numpy(value))
    if speakers:
        synthetic.speaker_acoustic_normalisers(model, n_speakers=5, device=DEV)
    else:
        synthetic.acoustic_normalisers(model, device=DEV)
    model.mode = 'train'
    return model


def _batch(model, speakers=False):
    feats = dict(_batch_np())
    if speakers:
        feats['speaker_id'], _ = synthetic.speaker_batch_ids(len(feats['n_frames']), n_speakers=5, seed=41)
    return data.to_device(feats, DEV, normalisers=model.normalisers)


def _step(model, batch):
    calls = []
    _lib.CALL_LOG = calls
    try:
        loss, out = model(batch)
        loss.backward()
    finally:
        _lib.CALL_LOG = None
    return loss.detach().clone(), out, [p.grad.clone() for p in model.parameters()], calls


def _gv_term(model, batch, out, log=True):
    """losses.gv of the model's own trajectory, normalised as StreamModel._trajectory_loss normalises it."""
    normaliser = model.normalisers['lf0']
    args = (batch[data.SPEAKER_INDEX_KEY],) if isinstance(normaliser, data._SpeakerDependentNormaliser) else ()
    target = batch.get('normalised_lf0')
    if target is None:
        target = normaliser.normalise(batch['lf0'], *args)
    return losses.gv(normaliser.normalise(out['lf0'].detach(), *args), target, batch['n_frames'], log=log)


@pytest.mark.parametrize('speakers', [False, True], ids=['global', 'per_speaker'])
def test_model_loss_gains_the_weighted_term(speakers):
    plain, varied = _model(speakers), _model(speakers, gv_weight=0.5)
    batch = _batch(plain, speakers)
    assert batch['n_frames'].shape[0] == 2 and batch['lf0'].shape[1] <= 40
    loss0, out0, grads0, calls0 = _step(plain, batch)
    loss, out, grads, calls = _step(varied, batch)
    assert out['lf0'].requires_grad and not out0['lf0'].requires_grad
    assert torch.equal(out['lf0'].detach(), out0['lf0'])
    term = _gv_term(varied, batch, out)
    want = loss0.double() + 0.5 * term.double()
    print('loss %.9g = %.9g + 0.5 * %.9g (off by %.3e)' % (loss.item(), loss0.item(), term.item(), abs(loss.double() - want).item()))
    assert term.item() > 0
    # both parts come from the same kernels on the same bits; what is left is the float32 sum: each part's rounding size
    assert abs(loss.double() - want).item() <= ref.U * (abs(loss0.item()) + 0.5 * abs(term.item()))
    assert calls.count('mg_gv_f32') == 1 and calls.count('mg_gv_bwd_f32') == 1 and calls.count('mg_mlpg_f32') == 1
    assert 'mg_gv_f32' not in calls0 and 'mg_gv_bwd_f32' not in calls0
    assert all(torch.isfinite(g).all() for g in grads)
    assert any(not torch.equal(a, b) for a, b in zip(grads, grads0))
    assert varied.metrics.results_as_json_dict('train')['LF0_RMSE_Hz'] > 0


def test_gv_log_reaches_the_loss():
    stream = models.Stream('lf0', 3, 'mse', ('LF0_RMSE_Hz', models.metrics.LF0Distortion, 'voiced_trajectory'), gv_weight=0.5, gv_log=False)
    plain = _model()
    model = models.StreamModel(plain.layers, [stream], fused_loss=False).to(DEV)
    model.output_dim = 3
    synthetic.acoustic_normalisers(model, device=DEV)
    model.mode = 'train'
    batch = _batch(plain)
    loss0, _, _, _ = _step(plain, batch)
    loss, out, _, _ = _step(model, batch)
    term = _gv_term(model, batch, out, log=False)
    assert abs(loss.double() - (loss0.double() + 0.5 * term.double())).item() <= ref.U * (abs(loss0.item()) + 0.5 * abs(term.item()))
    assert term.item() != _gv_term(model, batch, out, log=True).item()


def test_weight_zero_is_the_model_of_today_bit_for_bit():
    results = []
    for kwargs in ({}, {'gv_weight': 0.}):
        model = _model(**kwargs)
        loss, out, grads, calls = _step(model, _batch(model))
        assert not out['lf0'].requires_grad and not any(c.startswith('mg_gv') for c in calls)
        results.append((loss, out['lf0'].clone(), grads, calls))
    (loss_a, traj_a, grads_a, calls_a), (loss_b, traj_b, grads_b, calls_b) = results
    assert torch.equal(loss_a, loss_b) and torch.equal(traj_a, traj_b) and calls_a == calls_b
    assert len(grads_a) == len(grads_b) and all(torch.equal(a, b) for a, b in zip(grads_a, grads_b))
    # with a trajectory weight as well, weight 0 is the trajectory model of today
    results = []
    for kwargs in ({'trajectory_weight': 1.}, {'trajectory_weight': 1., 'gv_weight': 0.}):
        model = _model(**kwargs)
        loss, _, grads, calls = _step(model, _batch(model))
        results.append((loss, grads, calls))
    assert torch.equal(results[0][0], results[1][0]) and results[0][2] == results[1][2]
    assert all(torch.equal(a, b) for a, b in zip(results[0][1], results[1][1]))


def test_both_weights_solve_and_normalise_the_trajectory_once():
    trained, both = _model(trajectory_weight=1.), _model(trajectory_weight=1., gv_weight=0.5)
    batch = _batch(trained)
    loss_t, _, grads_t, calls_t = _step(trained, batch)
    loss, out, grads, calls = _step(both, batch)
    assert calls.count('mg_mlpg_f32') == 1 == calls_t.count('mg_mlpg_f32')
    assert calls.count('mg_mlpg_grad_f32') == 1 == calls_t.count('mg_mlpg_grad_f32')
    extra = sorted(c for c in set(calls) if calls.count(c) != calls_t.count(c))
    assert extra == ['mg_gv_bwd_f32', 'mg_gv_f32'], extra       # nothing else ran more often: one normalisation feeds both terms
    term = _gv_term(both, batch, out)
    want = loss_t.double() + 0.5 * term.double()
    # three float32 roundings apart: the sum of the two trajectory terms, the sum with the delta loss, and loss_t's own
    assert abs(loss.double() - want).item() <= 3 * ref.U * (abs(loss_t.item()) + 0.5 * abs(term.item()))
    assert any(not torch.equal(a, b) for a, b in zip(grads, grads_t))
