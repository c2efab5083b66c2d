"""losses.mdn / losses.mdn_select on the HIP path (csrc/mdn.hip, mg_masked_mdn_f32 / mg_mdn_select_f32): a (K, D) sweep across every
kernel form against the float64 restatement and its derived fp32 bound (tests/mdn_ref64.py) and against the torch composition on the
device, in-place column slices, masking, range, determinism, autograd, the selection, the caps, the mixture-density kind of
models.StreamModel (loss, training, outputs, trajectory, graph capture) and a guard on the models that have no such stream."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import mdn_ref64
import parity_report
from morgana_amd import _lib, data, losses, metrics, models, ops, optim, synthetic, utils, viz
from morgana_amd import functional as F_hip

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
_REFS = {}


def _dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_(True) if grad else t


def _sweep(k, d):
    """The sweep input at (K, D) and its float64 reference, computed once and shared (never modified)."""
    if (k, d) not in _REFS:
        pred, target, seq_len = mdn_ref64.sweep_case(k, d)
        _REFS[(k, d)] = (pred, target, seq_len, mdn_ref64.mdn(pred, target, seq_len, k))
    return _REFS[(k, d)]


def _torch_mdn(x, y, seq_len, k, min_log_std=None):
    """The definition composed of torch ops, on whatever device x is on."""
    b, t, d = y.shape
    a, mu, s = x[:, :, :k], x[:, :, k:k + k * d].reshape(b, t, k, d), x[:, :, k + k * d:].reshape(b, t, k, d)
    if min_log_std is not None:
        s = torch.clamp(s, min=min_log_std)
    z = (y[:, :, None, :] - mu) * torch.exp(-s)
    q = torch.log_softmax(a, dim=-1) - (0.5 * z * z + s).sum(dim=-1) - d * mdn_ref64.HALF_LOG_2PI
    frame = (-torch.logsumexp(q, dim=-1) / d).unsqueeze(-1)
    if seq_len is None:
        return torch.mean(torch.sum(frame, dim=1) / frame.shape[1])
    mask = (torch.arange(t, device=x.device)[None, :] < seq_len[:, None]).to(frame.dtype).unsqueeze(-1)
    return torch.mean(torch.sum(frame * mask, dim=1) / torch.sum(mask, dim=1))


def _run(pred, target, seq_len, k, **kwargs):
    """ops.masked_mdn on numpy inputs -> (loss, grad) as numpy."""
    loss, grad = ops.masked_mdn(_dev(pred), _dev(target), None if seq_len is None else _dev(seq_len), k, want_grad=True, **kwargs)
    return float(loss.item()), grad.cpu().numpy()


def _check_against_ref64(name, pred, target, seq_len, k, ref=None, min_log_std=None):
    """The loss and EVERY gradient element inside the float64 reference's derived fp32 bound; pad frames exactly zero."""
    if ref is None:
        ref = mdn_ref64.mdn(pred, target, seq_len, k, min_log_std=min_log_std)
    loss, grad = _run(pred, target, seq_len, k, min_log_std=min_log_std)
    loss_err, grad_err = abs(loss - ref['loss']), np.abs(grad.astype(np.float64) - ref['grad'])
    worst = float((grad_err / np.maximum(ref['grad_bound'], 1e-300)).max())
    print('%s: loss err %.3e (bound %.3e), worst gradient err / bound %.3f' % (name, loss_err, ref['loss_bound'], worst))
    parity_report.note(loss_err / ref['loss_bound'], label='%s: loss err / derived bound' % name, bound=1.0)
    parity_report.note(worst, label='%s: gradient err / derived bound' % name, bound=1.0)
    assert loss_err <= ref['loss_bound'], (name, loss_err, ref['loss_bound'])
    assert np.all(grad_err <= ref['grad_bound']), (name, worst)
    assert np.all(grad[~ref['mask']] == 0.0), name
    return loss, grad, ref


# ------------------------------------------------------------------------------------------------------------------------ 1. sweep
@pytest.mark.parametrize('k, d', mdn_ref64.SWEEP)
def test_sweep(k, d):
    pred, target, seq_len, ref = _sweep(k, d)
    loss, grad, _ = _check_against_ref64('K=%d D=%d' % (k, d), pred, target, seq_len, k, ref=ref)
    x = _dev(pred, grad=True)
    want = _torch_mdn(x, _dev(target), _dev(seq_len), k)
    want.backward()
    assert parity_report.note(abs(loss - want.item()) / max(abs(want.item()), 1e-30), 'loss vs torch on the device') <= 1e-4
    assert parity_report.rel_err(grad, x.grad.cpu().numpy(), 'grad vs torch on the device') <= 1e-4


# --------------------------------------------------------------------------------------------------------------------- 2. in place
@pytest.mark.parametrize('k, d', [(8, 3), (4, 180), (5, 205)])
def test_column_slice_is_read_and_written_in_place(k, d):
    pred, target, seq_len, _ = _sweep(k, d)
    b, t, w = pred.shape
    col0, extra = 7, 12
    rng = np.random.RandomState(3)
    wide_np = rng.standard_normal((b, t, w + extra)).astype(np.float32)
    wide_np[:, :, col0:col0 + w] = pred
    wide, y, n = _dev(wide_np), _dev(target), _dev(seq_len)
    loss_c, grad_c = ops.masked_mdn(_dev(pred), y, n, k, want_grad=True)
    shared = torch.full((b, t, w + extra), 7.5, device=DEV)
    loss_s, grad_s = ops.masked_mdn(wide, y, n, k, want_grad=True, col0=col0, grad_out=shared)
    assert grad_s is shared and torch.equal(loss_s, loss_c)
    assert torch.equal(shared[:, :, col0:col0 + w], grad_c)
    assert torch.all(shared[:, :, :col0] == 7.5) and torch.all(shared[:, :, col0 + w:] == 7.5)
    # through a non-contiguous view whose last dimension is contiguous, and a target that is a column slice itself
    view = wide[:, :, col0:col0 + w]
    assert not view.is_contiguous()
    x = view.detach().requires_grad_(True)
    y_wide = torch.cat((torch.zeros(b, t, 2, device=DEV), y, torch.ones(b, t, 1, device=DEV)), dim=2)
    loss_v = losses.mdn(x, y_wide[:, :, 2:2 + d], n, n_components=k)
    loss_v.backward()
    assert torch.equal(loss_v.detach(), loss_c) and torch.equal(x.grad, grad_c)
    assert torch.equal(wide, _dev(wide_np))               # the prediction itself is only read
    # the loss accumulated on the device: loss_out = loss_weight * loss + loss_keep * loss_out
    slot = torch.full((), 2.0, device=DEV)
    ops.masked_mdn(_dev(pred), y, n, k, want_grad=False, loss_out=slot, loss_weight=0.5, loss_keep=0.25)
    assert abs(slot.item() - (0.5 * loss_c.item() + 0.5)) <= 1e-6 * (abs(loss_c.item()) + 1.0)


# ----------------------------------------------------------------------------------------------------------------------- 3. masking
@pytest.mark.parametrize('k, d', [(8, 3), (5, 205)])
def test_masking(k, d):
    pred, target, seq_len, ref = _sweep(k, d)
    clean = _run(pred, target, seq_len, k)
    # NaN in the pad frames of predictions and targets: the same bits as without
    dirty_pred, dirty_target = pred.copy(), target.copy()
    dirty_pred[~ref['mask']] = np.nan
    dirty_target[~ref['mask']] = np.nan
    dirty = _run(dirty_pred, dirty_target, seq_len, k)
    assert np.isfinite(dirty[0]) and dirty[0] == clean[0] and np.array_equal(dirty[1], clean[1])
    # a NaN pre-fill of the gradient buffer: pad rows are written, as zero
    shared = torch.full(pred.shape, float('nan'), device=DEV)
    ops.masked_mdn(_dev(pred), _dev(target), _dev(seq_len), k, want_grad=True, grad_out=shared)
    assert np.array_equal(shared.cpu().numpy(), clean[1]) and torch.all(shared[2, 1:] == 0.0)
    # no seq_len == every frame valid
    b, t = pred.shape[:2]
    full = _run(pred, target, np.full(b, t, dtype=np.int64), k)
    none = _run(pred, target, None, k)
    assert none[0] == full[0] and np.array_equal(none[1], full[1])
    # seq_len > T is clamped, an utterance without a valid frame gives NaN - through that utterance only
    clamped = _run(pred, target, np.array([99, 20, 1], dtype=np.int64), k)
    assert clamped[0] == clean[0] and np.array_equal(clamped[1], clean[1])
    empty = _run(pred, target, np.array([37, 0, 1], dtype=np.int64), k)
    assert np.isnan(empty[0]) and np.isfinite(empty[1]).all() and np.all(empty[1][1] == 0.0) and np.array_equal(empty[1][0], clean[1][0])
    assert np.isnan(_run(pred, target, np.array([37, -2, 1], dtype=np.int64), k)[0])
    # no gradient wanted: the same loss
    assert ops.masked_mdn(_dev(pred), _dev(target), _dev(seq_len), k, want_grad=False)[0].item() == clean[0]


# ------------------------------------------------------------------------------------------------------------------------ 4. range
@pytest.mark.parametrize('name', ['far', 'dominant', 's_minus10', 's_plus10', 'minus_inf'])
def test_range(name):
    k, d, cases = mdn_ref64.range_cases()
    pred, target, seq_len = cases[name]
    loss, grad, ref = _check_against_ref64(name, pred, target, seq_len, k)
    assert np.isfinite(loss) and np.isfinite(grad).all()
    if name == 'far':
        assert loss > 1e5
    if name == 'minus_inf':
        gone = np.isneginf(pred[:, :, :k])
        assert np.all(grad[:, :, :k][gone] == 0.0)
        assert np.all(grad[:, :, k:k + k * d].reshape(gone.shape + (d,))[gone] == 0.0)
        assert np.all(grad[:, :, k + k * d:].reshape(gone.shape + (d,))[gone] == 0.0)


def test_all_logits_minus_inf_give_nan():
    pred, target, seq_len, _ = _sweep(8, 3)
    gone = pred.copy()
    gone[0, 5, :8] = -np.inf
    assert np.isnan(_run(gone, target, seq_len, 8)[0])
    gone = pred.copy()
    gone[1, 30, :8] = -np.inf                              # a pad frame: not read
    assert _run(gone, target, seq_len, 8)[0] == _run(pred, target, seq_len, 8)[0]


@pytest.mark.parametrize('k, d', [(8, 3), (4, 180), (5, 205)])
def test_floor(k, d):
    """min_log_std = -3 with half the log-stds below it: those get gradient exactly 0, loss and gradient are the clamped reference's."""
    pred, target, seq_len, _ = _sweep(k, d)
    rng = np.random.RandomState(17)
    pred = pred.copy()
    pred[:, :, k + k * d:] = (-3.0 + 0.5 * min(1.0, 2.0 / np.sqrt(d)) * rng.standard_normal((pred.shape[0], pred.shape[1], k * d))).astype(np.float32)
    pred[:, :, k:k + k * d] = (target[:, :, None, :] + np.exp(-3.0) * min(1.0, 2.0 / np.sqrt(d))
                               * rng.standard_normal(pred.shape[:2] + (k, d))).reshape(pred.shape[0], pred.shape[1], k * d).astype(np.float32)
    _, grad, ref = _check_against_ref64('floor K=%d D=%d' % (k, d), pred, target, seq_len, k, min_log_std=-3.0)
    below = ref['floored'] & ref['mask'][:, :, None, None]
    assert 0.3 < below[ref['mask']].mean() < 0.7
    g_s = grad[:, :, k + k * d:].reshape(below.shape)
    assert np.all(g_s[below] == 0.0) and np.any(g_s[~below] != 0.0)
    x = _dev(pred, grad=True)
    want = _torch_mdn(x, _dev(target), _dev(seq_len), k, min_log_std=-3.0)
    want.backward()
    assert parity_report.rel_err(grad, x.grad.cpu().numpy(), 'floored grad vs torch.clamp on the device') <= 1e-4


# ------------------------------------------------------------------------------------------------------- 5. determinism, 6. autograd
@pytest.mark.parametrize('k, d', [(16, 3), (4, 180), (5, 205)])
def test_determinism_and_autograd(k, d):
    pred, target, seq_len, _ = _sweep(k, d)
    y, n = _dev(target), _dev(seq_len.astype(np.int32))                                # narrower integers are widened

    def run(factor):
        x = _dev(pred, grad=True)
        t = y.clone().requires_grad_(True)
        loss = losses.mdn(x, t, n, n_components=k)
        (factor * loss).backward()
        assert t.grad is None                                                          # targets get no gradient
        return loss.detach().clone(), x.grad.clone()

    loss_a, grad_a = run(0.375)
    loss_b, grad_b = run(0.375)
    assert torch.equal(loss_a, loss_b) and torch.equal(grad_a, grad_b)                 # no atomics: the same bits
    direct = ops.masked_mdn(_dev(pred), y, _dev(seq_len), k, want_grad=True)
    assert torch.equal(direct[0], loss_a)
    # a non-unit upstream factor scales the saved gradient: one rounding
    want = direct[1].double() * 0.375
    err = (grad_a.double() - want).abs()
    assert torch.all(err <= want.abs() * 2.0 ** -23 + 2.0 ** -149)
    # functional.backward's cached gradient of one: the saved gradient goes out as it is
    x1 = _dev(pred, grad=True)
    F_hip.backward(losses.mdn(x1, y, _dev(seq_len), n_components=k))
    assert torch.equal(x1.grad, direct[1])
    with pytest.raises(RuntimeError):                                                  # no double backward
        x2 = _dev(pred, grad=True)
        (g,) = torch.autograd.grad(losses.mdn(x2, y, _dev(seq_len), n_components=k), x2, create_graph=True)
        g.sum().backward()


# ----------------------------------------------------------------------------------------------------------------------- 7. select
@pytest.mark.parametrize('k, d', [(1, 1), (8, 3), (64, 3), (4, 180), (16, 1024)])
def test_select(k, d):
    pred, target, seq_len, ref = _sweep(k, d)
    x, n = _dev(pred), _dev(seq_len)
    component, mean, variance = losses.mdn_select(x, k, d, seq_len=n)
    assert component.dtype == torch.int64 and tuple(component.shape) == pred.shape[:2] and tuple(mean.shape) == tuple(variance.shape) == target.shape
    assert not mean.requires_grad and not variance.requires_grad
    assert np.array_equal(component.cpu().numpy(), ref['component'])
    mu = x[:, :, k:k + k * d].reshape(pred.shape[0], pred.shape[1], k, d)
    gathered = torch.gather(mu, 2, component[:, :, None, None].expand(-1, -1, 1, d))[:, :, 0]
    valid = _dev(ref['mask'])
    assert torch.equal(mean[valid], gathered[valid])                                   # exact copies
    err = np.abs(variance.cpu().numpy().astype(np.float64) - ref['variance'])
    parity_report.note(float((err / np.maximum(ref['variance_bound'], 1e-300))[ref['mask']].max()), 'variance err / derived bound', bound=1.0)
    assert np.all(err <= ref['variance_bound'])
    assert torch.all(component[~valid] == 0) and torch.all(mean[~valid] == 0.0) and torch.all(variance[~valid] == 1.0)
    # a floor under the log-stds
    floored = mdn_ref64.mdn(pred, target, seq_len, k, min_log_std=-0.5)
    _, mean_f, variance_f = losses.mdn_select(x, k, d, seq_len=n, min_log_std=-0.5)
    assert torch.equal(mean_f, mean) and np.all(np.abs(variance_f.cpu().numpy() - floored['variance']) <= floored['variance_bound'])
    assert variance_f[valid].min().item() >= np.float32(np.exp(-1.0)) * (1 - 1e-6)
    # a column slice of a wider prediction, without seq_len
    wide = torch.cat((torch.full(pred.shape[:2] + (7,), 9.0, device=DEV), x, torch.full(pred.shape[:2] + (2,), -9.0, device=DEV)), dim=2)
    c_s, m_s, v_s = ops.mdn_select(wide, None, k, d, col0=7)
    c_v, m_v, v_v = losses.mdn_select(wide[:, :, 7:7 + pred.shape[2]], k, d)
    for got in ((c_s, m_s, v_s), (c_v, m_v, v_v)):
        assert torch.equal(got[0][valid], component[valid]) and torch.equal(got[1][valid], mean[valid]) and torch.equal(got[2][valid], variance[valid])
    assert torch.equal(c_s, torch.argmax(x[:, :, :k], dim=-1))                         # no NaN, no tie: torch.argmax on every frame
    # an exact tie: the lowest index
    if k > 2:
        tied = pred.copy()
        tied[0, 0, :k] = 0.0
        tied[0, 0, k - 1] = tied[0, 0, 1] = 5.0
        assert losses.mdn_select(_dev(tied), k, d, seq_len=n)[0][0, 0].item() == 1


# ------------------------------------------------------------------------------------------------------------------------- 8. caps
def test_caps_are_refused_before_any_launch():
    calls = _lib.CALL_LOG = []
    try:
        with pytest.raises(_lib.MorganaHipError, match='cap of 64'):
            ops.masked_mdn(torch.zeros(1, 2, 65 * 3, device=DEV), torch.zeros(1, 2, 1, device=DEV), None, 65, want_grad=True)
        with pytest.raises(_lib.MorganaHipError, match='cap of 16384'):
            ops.masked_mdn(torch.zeros(1, 2, 2 * 16385 + 1, device=DEV), torch.zeros(1, 2, 16385, device=DEV), None, 1, want_grad=True)
        with pytest.raises(_lib.MorganaHipError, match='cap of 64'):
            ops.mdn_select(torch.zeros(1, 2, 65 * 3, device=DEV), None, 65, 1)
        with pytest.raises(_lib.MorganaHipError, match='cap of 16384'):
            losses.mdn_select(torch.zeros(1, 2, 2 * 16385 + 1, device=DEV), 1, 16385)
        with pytest.raises(_lib.MorganaHipError, match='cap of 16384'):
            losses.mdn(torch.zeros(1, 2, 2 * 16385 + 1, device=DEV), torch.zeros(1, 2, 16385, device=DEV))
        assert calls == []                                                             # no entry point was reached
    finally:
        _lib.CALL_LOG = None
    with pytest.raises(ValueError, match='do not fit'):
        ops.masked_mdn(torch.zeros(1, 2, 27, device=DEV), torch.zeros(1, 2, 3, device=DEV), None, 4, want_grad=True)
    with pytest.raises(ValueError, match='targets'):
        ops.masked_mdn(torch.zeros(1, 2, 28, device=DEV), torch.zeros(1, 3, 3, device=DEV), None, 4, want_grad=True)


# ------------------------------------------------------------------------------------------------------------------ 9. StreamModel
K_MODEL, D_MODEL = 4, 3
W_MODEL = K_MODEL * (1 + 2 * D_MODEL)
STREAMS = (('lf0', D_MODEL, 'mse'), ('vuv', 1, 'sigmoid_bce'))


def _batch():
    return data.to_device(synthetic.make_acoustic_batch(2, (30, 40), streams=STREAMS, seed=71, with_raw=True), DEV)


def _mixture_model(seed=7, normalisers=True, **stream_kwargs):
    torch.manual_seed(seed)
    layers = utils.SequentialWithRecurrent(nn.Linear(609, 64), nn.Sigmoid(), nn.Linear(64, W_MODEL + 1), precision='fp32')
    streams = [models.Stream('lf0', D_MODEL, 'mdn', ('LF0_RMSE_Hz', metrics.LF0Distortion, 'voiced_trajectory'), n_components=K_MODEL,
                             **stream_kwargs),
               models.Stream('vuv', 1, 'sigmoid_bce', ('VUV_accuracy', metrics.Mean, 'accuracy'))]
    model = models.StreamModel(layers, streams, fused_loss=False).to(DEV)
    model.output_dims = {'lf0': D_MODEL}
    if normalisers:
        synthetic.acoustic_normalisers(model, device=DEV)
    model.mode = 'train'
    model.metrics.reset_state('train')
    return model


def _composed_loss(model, feats, min_log_std=None):
    """The same model's loss with the mixture term composed of torch ops (the probability stream through losses.bce, as shipped)."""
    prediction = model._run_layers(feats)
    n = feats['n_frames']
    nll = _torch_mdn(prediction[:, :, :W_MODEL], feats['normalised_lf0_deltas'], n, K_MODEL, min_log_std=min_log_std)
    return (nll + losses.bce(torch.sigmoid(prediction[:, :, W_MODEL:]), feats['vuv'], n)) / 2.


def test_stream_model_loss_training_and_outputs():
    feats = _batch()
    model, twin = _mixture_model(min_log_std=-4.), _mixture_model(min_log_std=-4.)
    loss, outputs = model(feats)
    want = _composed_loss(twin, feats, min_log_std=-4.)
    assert parity_report.note(abs(loss.item() - want.item()) / abs(want.item()), 'loss vs the torch-composed loss') <= 1e-4
    # three Adam steps next to the torch-composed twin
    opt, opt_twin = optim.Adam(model.parameters(), lr=0.01), optim.Adam(twin.parameters(), lr=0.01)
    history = []
    for _ in range(3):
        opt.zero_grad()
        loss, outputs = model(feats)
        loss.backward()
        opt.step()
        opt_twin.zero_grad()
        _composed_loss(twin, feats, min_log_std=-4.).backward()
        opt_twin.step()
        history.append(loss.item())
    assert np.isfinite(history).all(), history
    for (name, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert parity_report.rel_err(p.detach().cpu().numpy(), q.detach().cpu().numpy(), 'three Adam steps: ' + name) <= 1e-4, name
    # outputs: the raw parameters, the selected mean and variance, the trajectory under the per-frame variances
    assert set(outputs) == {'lf0_mdn', 'normalised_lf0_deltas', 'normalised_lf0_deltas_variance', 'lf0', 'vuv'}
    n = feats['n_frames']
    raw = outputs['lf0_mdn']
    assert tuple(raw.shape) == tuple(n.shape) + (feats['vuv'].shape[1], W_MODEL) and raw.requires_grad
    _, mean, variance = ops.mdn_select(raw.detach(), n, K_MODEL, D_MODEL, min_log_std=-4.)
    assert torch.equal(outputs['normalised_lf0_deltas'], mean) and torch.equal(outputs['normalised_lf0_deltas_variance'], variance)
    assert not outputs['normalised_lf0_deltas'].requires_grad and not outputs['normalised_lf0_deltas_variance'].requires_grad
    assert variance.min().item() >= np.float32(np.exp(-8.0)) * (1 - 1e-6)
    normaliser = model.normalisers['lf0']
    std_dev = normaliser.delta_params_torch['std_dev'].to(device=DEV, dtype=torch.float32)
    by_hand = ops.mlpg(normaliser.denormalise(mean, deltas=True), variance * std_dev ** 2, viz.synthesis.DEFAULT_WINDOWS, padding_size=100,
                       seq_len=n)
    assert torch.equal(outputs['lf0'], by_hand) and tuple(by_hand.shape) == tuple(feats['lf0'].shape)
    # the per-frame variances matter: the global-variance trajectory of the same means differs
    global_var = ops.mlpg(normaliser.denormalise(mean, deltas=True), std_dev ** 2, viz.synthesis.DEFAULT_WINDOWS, padding_size=100, seq_len=n)
    assert not torch.equal(global_var, by_hand)
    results = model.metrics.results_as_json_dict('train')
    assert np.isfinite(results['LF0_RMSE_Hz']) and 0.0 <= results['VUV_accuracy'] <= 1.0
    # without delta parameters on the normaliser: parameters, mean and variance, no trajectory
    bare = _mixture_model(normalisers=False)
    loss_bare, out_bare = bare(feats)
    assert set(out_bare) == {'lf0_mdn', 'normalised_lf0_deltas', 'normalised_lf0_deltas_variance', 'vuv'} and np.isfinite(loss_bare.item())


def test_stream_model_refusals():
    layers = utils.SequentialWithRecurrent(nn.Linear(609, 8), nn.Sigmoid(), nn.Linear(8, W_MODEL + 1), precision='fp32')
    streams = [models.Stream('lf0', D_MODEL, 'mdn', n_components=K_MODEL), models.Stream('vuv', 1, 'sigmoid_bce')]
    with pytest.raises(ValueError, match='no MDN term'):
        models.StreamModel(layers, streams, fused_loss=True)
    with pytest.raises(ValueError, match='not a differentiable function of the weights'):
        models.Stream('lf0', D_MODEL, 'mdn', n_components=K_MODEL, trajectory_weight=1.)


def test_speaker_dependent_trajectory_takes_per_frame_variances():
    feats = _batch()
    names, rows = synthetic.speaker_batch_ids(2, n_speakers=3, seed=5)
    feats['speaker_id'], feats[data.SPEAKER_INDEX_KEY] = names, torch.from_numpy(rows).to(DEV)
    torch.manual_seed(9)
    model = models.GRUF0Model(n_components=K_MODEL, speaker_id_list=synthetic.speaker_names(3), precision='fp32').to(DEV)
    synthetic.speaker_acoustic_normalisers(model, n_speakers=3, device=DEV)
    model.mode = 'train'
    model.metrics.reset_state('train')
    loss, outputs = model(feats)
    assert np.isfinite(loss.item())
    normaliser, n = model.normalisers['lf0'], feats['n_frames']
    mean, variance = outputs['normalised_lf0_deltas'], outputs['normalised_lf0_deltas_variance']
    index = normaliser.speaker_index(feats[data.SPEAKER_INDEX_KEY], DEV)
    std_dev = ops.item_rows(normaliser.tables(DEV, deltas=True)[1], index)
    by_hand = ops.mlpg(normaliser.denormalise(mean, feats[data.SPEAKER_INDEX_KEY], deltas=True), variance * (std_dev ** 2)[:, None, :],
                       viz.synthesis.DEFAULT_WINDOWS, padding_size=100, seq_len=n)
    assert torch.equal(outputs['lf0'], by_hand)


# ------------------------------------------------------------------------------------------------------------------------ 10. graph
def test_graphed_step_replays_bit_equal():
    from morgana_amd import graphs
    feats = _batch()

    def fresh():
        model = _mixture_model()
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


# --------------------------------------------------------------------------------------------------------------- 11. regression guard
def test_models_without_a_mixture_stream_are_unchanged():
    feats = data.to_device(synthetic.make_acoustic_batch(2, (30, 40), streams=(('lf0', 3, 'mse'),), seed=72, with_raw=True), DEV)

    def run(model):
        model = model.to(DEV)
        synthetic.acoustic_normalisers(model, device=DEV)
        model.mode = 'train'
        model.metrics.reset_state('train')
        loss, outputs = model(feats)
        loss.backward()
        return model, loss.detach(), outputs

    torch.manual_seed(3)
    shipped, loss_a, out_a = run(models.GRUF0Model(precision='fp32'))
    assert [(st.loss, st.dim, st.width, st.n_components) for st in shipped.streams] == [('mse', 3, 3, 1)]
    torch.manual_seed(3)
    table = models.StreamModel(models._gru_f0_stack(609, 3, 0., 'fp32'),
                               [models.Stream('lf0', 3, 'mse', ('LF0_RMSE_Hz', metrics.LF0Distortion, 'voiced_trajectory'))], fused_loss=False)
    table.output_dim = 3
    table, loss_b, out_b = run(table)
    assert torch.equal(loss_a, loss_b) and set(out_a) == set(out_b) == {'normalised_lf0_deltas', 'lf0'}
    for key in out_a:
        assert torch.equal(out_a[key], out_b[key]), key
    for p, q in zip(shipped.parameters(), table.parameters()):
        assert torch.equal(p.grad, q.grad)
    # _split of a table without a mixture stream: torch.split by dim, under the old keys
    acoustic = models.LSTMAcousticModel(num_layers=1, precision='fp32', fused_loss=False)
    assert all(st.width == st.dim for st in acoustic.streams)
    prediction = torch.randn(2, 5, 199, device=DEV)
    parts = acoustic._split(prediction)
    want = dict(zip(('normalised_lf0_deltas', 'vuv', 'normalised_mcep_deltas', 'normalised_bap_deltas'), torch.split(prediction, [3, 1, 180, 15], dim=-1)))
    want['vuv'] = torch.sigmoid(want['vuv'])
    assert set(parts) == set(want) and all(torch.equal(parts[key], want[key]) for key in want)
