"""losses.ce on the HIP path (csrc/ce.hip, mg_masked_ce_f32): the reference's recorded numbers, a class-count sweep across both
kernel forms against the float64 restatement and its derived fp32 bound (tests/ce_ref64.py) and against torch on the device, strided
inputs, range, masking and target edge cases, autograd, the categorical kind of losses.multi_stream and of models.StreamModel."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ce_ref64
import parity_report
from morgana_amd import data, losses, metrics, models, ops, optim, synthetic, utils
from morgana_amd import functional as F_hip

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GOLDEN_CASES = ('ragged', 'full', 'c2', 'c65', 'ignore')


def _dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_(True) if grad else t


def _torch_ce(x, y, seq_len):
    """The reference's composition (losses.py:29-46 around :59-61) in torch, on whatever device x is on."""
    frame = F.cross_entropy(x.transpose(1, 2), y, reduction='none').unsqueeze(-1)
    if seq_len is None:
        return torch.mean(torch.sum(frame, dim=1) / frame.shape[1])
    mask = (torch.arange(frame.shape[1], device=x.device)[None, :] < seq_len[:, None]).to(frame.dtype).unsqueeze(-1)
    return torch.mean(torch.sum(frame * mask, dim=1) / torch.sum(mask, dim=1))


def _run(pred, target, seq_len, grad_scale=1.0):
    """ops.masked_ce on numpy inputs -> (loss, grad, argmax) as numpy."""
    loss, grad, argmax = ops.masked_ce(_dev(pred), _dev(target), None if seq_len is None else _dev(seq_len), want_grad=True,
                                       grad_scale=grad_scale, want_argmax=True)
    return float(loss.item()), grad.cpu().numpy(), argmax.cpu().numpy()


def _check_against_ref64(name, pred, target, seq_len):
    """Loss, every gradient element and the argmax of the valid frames inside the float64 reference's derived fp32 bound."""
    ref = ce_ref64.ce(pred, target, seq_len)
    loss, grad, argmax = _run(pred, target, seq_len)
    loss_err, grad_err = abs(loss - ref['loss']), np.abs(grad.astype(np.float64) - ref['grad'])
    worst = float((grad_err / np.maximum(ref['grad_bound'], 1e-300)).max())
    print('%s: loss err %.3e (bound %.3e), worst gradient err / bound %.3f' % (name, loss_err, ref['loss_bound'], worst))
    parity_report.note(loss_err / ref['loss_bound'], label='%s: loss err / derived bound' % name, bound=1.0)
    parity_report.note(worst, label='%s: gradient err / derived bound' % name, bound=1.0)
    assert loss_err <= ref['loss_bound'], (name, loss_err, ref['loss_bound'])
    assert np.all(grad_err <= ref['grad_bound']), (name, worst)
    assert np.array_equal(argmax, ref['argmax']), name
    assert np.all(grad[~ref['mask']] == 0.0), name
    return loss, grad


# ---------------------------------------------------------------------------------------------------------------- 1. golden cases
@pytest.mark.parametrize('name', GOLDEN_CASES)
def test_golden_cases(golden, name):
    g = golden('g18_ce.npz')
    seq_len = g.get(name + '__seq_len')
    x = _dev(g[name + '__pred'], grad=True)
    loss = losses.ce(x, _dev(g[name + '__target']), None if seq_len is None else _dev(seq_len))
    loss.backward()
    want_loss = float(g[name + '__loss'])
    assert parity_report.note(abs(loss.item() - want_loss) / abs(want_loss), 'loss') <= 1e-4
    assert parity_report.rel_err(x.grad.cpu().numpy(), g[name + '__grad'], 'grad') <= 1e-4


# ------------------------------------------------------------------------------------------------------------ 2. class-count sweep
@pytest.mark.parametrize('c', ce_ref64.SWEEP_CLASSES)
def test_class_count_sweep(c):
    pred, target, seq_len = ce_ref64.sweep_case(c)
    loss, grad = _check_against_ref64('C=%d' % c, pred, target, seq_len)
    x = _dev(pred, grad=True)
    want = _torch_ce(x, _dev(target), _dev(seq_len))
    want.backward()
    assert parity_report.note(abs(loss - want.item()) / max(abs(want.item()), 1e-30), 'loss vs torch on the device') <= 1e-4
    if c > 1:                                              # C == 1: the gradient is identically zero
        assert parity_report.rel_err(grad, x.grad.cpu().numpy(), 'grad vs torch on the device') <= 1e-4
    else:
        assert np.all(grad == 0.0) and loss == 0.0


# ---------------------------------------------------------------------------------------------------------------- 3. strided input
def test_column_slice_is_read_and_written_in_place():
    c, extra = 65, 7
    pred, target, seq_len = ce_ref64.sweep_case(c)
    rng = np.random.RandomState(3)
    wide_np = rng.standard_normal((2, 5, c + extra)).astype(np.float32)
    wide_np[:, :, 3:3 + c] = pred
    wide = _dev(wide_np)
    y, n = _dev(target), _dev(seq_len)
    loss_c, grad_c, argmax_c = ops.masked_ce(_dev(pred), y, n, want_grad=True, want_argmax=True)
    # through the column arguments, into a shared gradient buffer
    shared = torch.full((2, 5, c + extra), 7.5, device=DEV)
    loss_s, grad_s, argmax_s = ops.masked_ce(wide, y, n, want_grad=True, want_argmax=True, col0=3, width=c, grad_out=shared)
    assert grad_s is shared and torch.equal(loss_s, loss_c) and torch.equal(argmax_s, argmax_c)
    assert torch.equal(shared[:, :, 3:3 + c], grad_c)
    assert torch.all(shared[:, :, :3] == 7.5) and torch.all(shared[:, :, 3 + c:] == 7.5)
    # through a non-contiguous view whose last dimension is contiguous (losses.ce reads it through its row stride)
    view = wide[:, :, 3:3 + c]
    assert not view.is_contiguous()
    x = view.detach().requires_grad_(True)
    loss_v = losses.ce(x, y, n)
    loss_v.backward()
    assert torch.equal(loss_v.detach(), loss_c) and torch.equal(x.grad, grad_c)
    assert torch.equal(wide, _dev(wide_np))               # the prediction itself is only read


# ------------------------------------------------------------------------------------------------------------------------ 4. range
@pytest.mark.parametrize('name', ['pm80', 'spike_1e4', 'minus_inf'])
def test_range(name):
    pred, target, seq_len = ce_ref64.range_cases()[name]
    loss, grad = _check_against_ref64(name, pred, target, seq_len)
    assert np.isfinite(loss) and np.isfinite(grad).all()
    if name == 'minus_inf':
        assert np.all(grad[np.isneginf(pred)] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------- 5. masking
def test_masking():
    pred, target, _ = ce_ref64.sweep_case(65)
    b, t, c = pred.shape
    # an utterance without a valid frame: NaN, and only through that utterance
    loss, grad, _ = _run(pred, target, np.array([5, 0], dtype=np.int64))
    assert np.isnan(loss) and np.isfinite(grad).all() and np.all(grad[1] == 0.0)
    alone = ce_ref64.ce(pred[:1], target[:1], np.array([5]))
    loss0, grad0, _ = _run(pred[:1], target[:1], np.array([5], dtype=np.int64))
    assert abs(loss0 - alone['loss']) <= alone['loss_bound']
    np.testing.assert_array_equal(grad[0], grad0[0] * np.float32(0.5))          # 1 / (n_b B): B = 2 against B = 1, a power of two
    # seq_len > T is clamped, a negative one counts as 0
    clamped = _run(pred, target, np.array([9, 3], dtype=np.int64))
    plain = _run(pred, target, np.array([5, 3], dtype=np.int64))
    assert clamped[0] == plain[0] and np.array_equal(clamped[1], plain[1])
    assert np.isnan(_run(pred, target, np.array([5, -2], dtype=np.int64))[0])
    # pad frames: an exactly zero gradient over a NaN pre-fill, targets of 10^9 never looked at
    wild = target.copy()
    wild[1, 3:] = 10 ** 9
    shared = torch.full((b, t, c), float('nan'), device=DEV)
    loss_w, _, argmax_w = ops.masked_ce(_dev(pred), _dev(wild), _dev(np.array([5, 3], dtype=np.int64)), want_grad=True, want_argmax=True,
                                        grad_out=shared)
    assert loss_w.item() == plain[0] and np.array_equal(shared.cpu().numpy(), plain[1]) and np.array_equal(argmax_w.cpu().numpy(), plain[2])
    assert torch.all(shared[1, 3:] == 0.0) and torch.all(argmax_w[1, 3:] == 0)
    # no gradient wanted: the same loss
    assert ops.masked_ce(_dev(pred), _dev(target), _dev(np.array([5, 3], dtype=np.int64)), want_grad=False)[0].item() == plain[0]


# ------------------------------------------------------------------------------------------------------------------ 6. bad targets
@pytest.mark.parametrize('c', [65, ce_ref64.REG_MAX + 1])
def test_target_edge_cases(c):
    """Defined behaviour, not faults: a target outside [0, C) in a valid frame gives a NaN loss and a zero gradient row; -100 is
    F.cross_entropy's ignore_index."""
    pred, target, seq_len = ce_ref64.sweep_case(c)
    plain = _run(pred, target, seq_len)
    for bad_value in (c, -1):
        bad = target.copy()
        bad[0, 2] = bad_value
        loss, grad, argmax = _run(pred, bad, seq_len)
        assert np.isnan(loss) and np.isfinite(grad).all() and np.all(grad[0, 2] == 0.0)
        others = np.ones(grad.shape[:2], dtype=bool)
        others[0, 2] = False
        assert np.array_equal(grad[others], plain[1][others]) and np.array_equal(argmax, plain[2])
    ignored = target.copy()
    ignored[0, 2] = ignored[1, 0] = -100
    loss, grad, _ = _run(pred, ignored, seq_len)
    x = _dev(pred, grad=True)
    want = _torch_ce(x, _dev(ignored), _dev(seq_len))
    want.backward()
    assert parity_report.note(abs(loss - want.item()) / abs(want.item()), 'ignore_index loss vs torch') <= 1e-4
    assert parity_report.rel_err(grad, x.grad.cpu().numpy(), 'ignore_index grad vs torch') <= 1e-4
    assert np.all(grad[0, 2] == 0.0) and np.all(grad[1, 0] == 0.0)
    ref = ce_ref64.ce(pred, ignored, seq_len)
    assert abs(loss - ref['loss']) <= ref['loss_bound'] and np.all(np.abs(grad - ref['grad']) <= ref['grad_bound'])


# --------------------------------------------------------------------------------------------------------------------- 7. autograd
def test_autograd_scaled_loss_and_determinism():
    pred, target, seq_len = ce_ref64.sweep_case(255)
    y, n = _dev(target.astype(np.int32)), _dev(seq_len.astype(np.int32))           # narrower integers are widened

    def run():
        x = _dev(pred, grad=True)
        loss = losses.ce(x, y[:, :, None], n)                                      # (B, T, 1) targets, as a loader yields them
        (0.5 * loss).backward()
        return loss.detach().clone(), x.grad.clone()

    loss_a, grad_a = run()
    loss_b, grad_b = run()
    assert torch.equal(loss_a, loss_b) and torch.equal(grad_a, grad_b)             # no atomics: the same bits
    x = _dev(pred, grad=True)
    want = _torch_ce(x, _dev(target), _dev(seq_len))
    (0.5 * want).backward()
    assert parity_report.note(abs(loss_a.item() - want.item()) / abs(want.item()), 'loss') <= 1e-4
    assert parity_report.rel_err(grad_a.cpu().numpy(), x.grad.cpu().numpy(), 'grad of 0.5 loss') <= 1e-4
    # functional.backward's cached gradient of one: the saved gradient goes out as it is
    x1 = _dev(pred, grad=True)
    F_hip.backward(losses.ce(x1, _dev(target), _dev(seq_len)))
    assert parity_report.rel_err(x1.grad.cpu().numpy(), 2.0 * grad_a.cpu().numpy(), 'unit grad') <= 1e-6
    # the argmax output is not differentiable and comes from the same pass
    x2 = _dev(pred, grad=True)
    loss2, argmax = losses.ce(x2, _dev(target), _dev(seq_len), want_argmax=True)
    assert not argmax.requires_grad and argmax.dtype == torch.int64
    valid = torch.arange(5, device=DEV)[None, :] < _dev(seq_len)[:, None]
    assert torch.equal(argmax[valid], torch.argmax(x2.detach(), dim=-1)[valid]) and torch.equal(loss2.detach(), loss_a)


# ----------------------------------------------------------------------------------------------------------------- 8. multi_stream
def _stream_inputs():
    rng = np.random.RandomState(11)
    pred = rng.standard_normal((2, 6, 3 + 1 + 5)).astype(np.float32)
    y_mse = rng.standard_normal((2, 6, 3)).astype(np.float32)
    y_bce = (rng.random_sample((2, 6, 1)) > 0.4).astype(np.float32)
    y_ce = rng.randint(0, 5, size=(2, 6)).astype(np.int64)
    return pred, y_mse, y_bce, y_ce, np.array([6, 4], dtype=np.int64)


def test_multi_stream_with_a_categorical_stream():
    pred, y_mse, y_bce, y_ce, seq_len = _stream_inputs()
    n = _dev(seq_len)
    x = _dev(pred, grad=True)
    loss, prob, classes = losses.multi_stream(x, [_dev(y_mse), _dev(y_bce), _dev(y_ce)], ['mse', 'sigmoid_bce', 'ce'], n, want_prob=True,
                                              want_argmax=True)
    loss.backward()
    x2 = _dev(pred, grad=True)
    parts = torch.split(x2, [3, 1, 5], dim=-1)
    want = (losses.mse(parts[0], _dev(y_mse), n) + losses.bce(torch.sigmoid(parts[1]), _dev(y_bce), n) + losses.ce(parts[2], _dev(y_ce), n)) / 3.
    want.backward()
    assert parity_report.note(abs(loss.item() - want.item()) / abs(want.item()), 'loss vs (mse + bce + ce) / 3') <= 1e-6
    assert parity_report.rel_err(x.grad.cpu().numpy(), x2.grad.cpu().numpy(), 'grad vs the separate losses') <= 1e-5
    assert parity_report.rel_err(prob.cpu().numpy(), torch.sigmoid(parts[1]).detach().cpu().numpy(), 'prob') <= 1e-6
    valid = torch.arange(6, device=DEV)[None, :] < n[:, None]
    assert list(classes) == [2] and torch.equal(classes[2][valid], torch.argmax(parts[2].detach(), dim=-1)[valid])
    # the categorical stream first and alone: the same means
    order = [3 + 1 + np.arange(5), np.arange(3), 3 + np.arange(1)]
    x3 = _dev(pred[:, :, np.concatenate(order)], grad=True)
    loss3, _ = losses.multi_stream(x3, [_dev(y_ce), _dev(y_mse), _dev(y_bce)], ['ce', 'mse', 'sigmoid_bce'], n)
    assert abs(loss3.item() - want.item()) <= 1e-6 * abs(want.item())
    x4 = _dev(pred[:, :, 4:], grad=True)
    loss4, _ = losses.multi_stream(x4, [_dev(y_ce)], ['ce'], n)
    loss4.backward()
    x5 = _dev(pred[:, :, 4:], grad=True)
    alone = losses.ce(x5, _dev(y_ce), n)
    alone.backward()
    assert torch.equal(loss4.detach(), alone.detach()) and torch.equal(x4.grad, x5.grad)


def test_multi_stream_without_a_categorical_stream_takes_the_old_path():
    pred, y_mse, y_bce, _, seq_len = _stream_inputs()
    n = _dev(seq_len)
    x = _dev(pred[:, :, :4], grad=True)
    loss, prob = losses.multi_stream(x, [_dev(y_mse), _dev(y_bce)], ['mse', 'sigmoid_bce'], n, want_prob=True)
    loss.backward()
    want_loss, want_grad, want_prob = ops.stream_loss(_dev(pred[:, :, :4]), [_dev(y_mse), _dev(y_bce)], ['mse', 'sigmoid_bce'], n,
                                                      want_grad=True, want_prob=True)
    assert torch.equal(loss.detach(), want_loss) and torch.equal(x.grad, want_grad) and torch.equal(prob, want_prob)
    assert type(loss.grad_fn).__name__.startswith('StreamLossFn')


# ------------------------------------------------------------------------------------------------- 9. StreamModel, categorical stream
N_CLASSES = 37


def _categorical_batch():
    feats = synthetic.make_acoustic_batch(4, (30, 40), streams=(('lf0', 3, 'mse'),), seed=61, with_raw=True)
    rng = np.random.RandomState(62)
    b, t = feats['normalised_counters'].shape[:2]
    mask = np.arange(t)[None, :] < feats['n_frames'][:, None]
    feats['phone'] = (rng.randint(0, N_CLASSES, size=(b, t)) * mask).astype(np.int64)[:, :, None]     # (B, T, 1), zero padded
    return feats


def _categorical_model(fused_loss, seed=7):
    torch.manual_seed(seed)
    layers = utils.SequentialWithRecurrent(nn.Linear(609, 64), nn.Sigmoid(), nn.Linear(64, 3 + N_CLASSES), precision='fp32')
    streams = [models.Stream('lf0', 3, 'mse'),
               models.Stream('phone', N_CLASSES, 'ce', ('phone_accuracy', metrics.DeviceMean, 'accuracy'))]
    model = models.StreamModel(layers, streams, fused_loss=fused_loss).to(DEV)
    model.output_dims = {'lf0': 3}
    return model


def test_stream_model_fused_equals_unfused_and_learns():
    feats = data.to_device(_categorical_batch(), DEV)
    fused, unfused = _categorical_model(True), _categorical_model(False)
    unfused.load_state_dict(fused.state_dict())
    for model in (fused, unfused):
        synthetic.acoustic_normalisers(model, device=DEV)
        model.mode = 'train'
        model.metrics.reset_state('train')
    loss_f, out_f = fused(feats)
    loss_u, out_u = unfused(feats)
    loss_f.backward()
    loss_u.backward()
    assert parity_report.note(abs(loss_f.item() - loss_u.item()) / abs(loss_u.item()), 'fused vs unfused loss') <= 1e-4
    for (name, p), (_, q) in zip(fused.named_parameters(), unfused.named_parameters()):
        assert parity_report.rel_err(p.grad.cpu().numpy(), q.grad.cpu().numpy(), 'fused vs unfused d' + name) <= 1e-4, name
    assert set(out_f) == set(out_u) == {'normalised_lf0_deltas', 'lf0', 'phone_logits', 'phone'}
    assert out_f['phone'].dtype == torch.int64 and tuple(out_f['phone'].shape) == tuple(feats['phone'].shape[:2])
    valid = torch.arange(feats['phone'].shape[1], device=DEV)[None, :] < feats['n_frames'][:, None]
    want_class = torch.argmax(out_f['phone_logits'].detach(), dim=-1)
    assert torch.equal(out_f['phone'][valid], want_class[valid]) and torch.equal(out_u['phone'], torch.argmax(out_u['phone_logits'], dim=-1))
    # the accuracy metric: the hit rate over the valid frames, recomputed with torch
    hits = (feats['phone'][:, :, 0] == want_class)[valid].double()
    for model in (fused, unfused):
        got = model.metrics.results_as_json_dict('train')['phone_accuracy']
        assert abs(got - hits.mean().item()) <= 1e-9, (got, hits.mean().item())
    # against torch end to end: the loss is the mean of the lf0 stream's masked MSE and the phone stream's cross entropy
    seq = feats['n_frames']
    want = (losses.mse(out_u['normalised_lf0_deltas'].detach(), feats['normalised_lf0_deltas'], seq) +
            _torch_ce(out_u['phone_logits'].detach(), feats['phone'][:, :, 0], seq)) / 2.
    assert abs(loss_u.item() - want.item()) <= 1e-4 * abs(want.item())
    # ten Adam steps lower the loss
    opt = optim.Adam(fused.parameters(), lr=0.01)
    history = []
    for _ in range(10):
        opt.zero_grad()
        loss, _ = fused(feats)
        loss.backward()
        opt.step()
        history.append(loss.item())
    assert history[-1] < history[0] and np.isfinite(history).all(), history


def test_stream_model_graphed_step_replays_bit_equal():
    from morgana_amd import graphs
    feats = data.to_device(_categorical_batch(), DEV)

    def fresh():
        model = _categorical_model(True)
        return model, optim.Adam(model.parameters(), lr=0.01)

    model_e, opt_e = fresh()
    losses_e = []
    for _ in range(6):
        opt_e.zero_grad()
        loss, _ = model_e(feats)
        loss.backward()
        opt_e.step()
        losses_e.append(loss.item())
    model_g, opt_g = fresh()
    step = graphs.GraphedTrainStep(model_g, opt_g, feats, warmup=2)
    losses_g = [step().clone() for _ in range(2, 6)]
    assert [v.item() for v in losses_g] == losses_e[2:]
    flat_e, flat_g = opt_e.flat_buffers(), opt_g.flat_buffers()
    for key in ('param', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(flat_e[key], flat_g[key]), key


def test_integer_feature_through_the_device_collate():
    """An integer per-frame feature next to float features through data.collate_to_device: zero padded, int64, on the device, not
    normalised - and accepted by losses.ce as it comes out."""
    rng = np.random.RandomState(5)
    lens = [4, 7, 2]
    batch = [{'name': 'u%d' % i, 'n_frames': n, 'lf0': rng.rand(n, 1).astype(np.float32),
              'phone': rng.randint(1, 9, size=(n, 1)).astype(np.int64)} for i, n in enumerate(lens)]
    norms = {'lf0': data.MeanVarianceNormaliser('lf0').set_params({'mean': np.array([0.5], np.float32), 'std_dev': np.array([2.0], np.float32)},
                                                                   device=DEV)}
    out = data.collate_to_device(batch, norms, DEV)
    want = np.zeros((3, 7, 1), dtype=np.int64)
    for i, item in enumerate(batch):
        want[i, :lens[i]] = item['phone']
    assert out['phone'].is_cuda and out['phone'].dtype == torch.int64 and np.array_equal(out['phone'].cpu().numpy(), want)
    assert 'normalised_phone' not in out and 'normalised_lf0' in out
    logits = torch.zeros(3, 7, 9, device=DEV)
    loss = losses.ce(logits, out['phone'], out['n_frames'])
    assert abs(loss.item() - np.log(9.0)) <= 1e-6 * np.log(9.0)
