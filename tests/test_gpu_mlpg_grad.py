"""Differentiable MLPG on the device (run with ``-m gpu`` on an MI355X): mg_mlpg_grad_f32 against the dense float64 reference of
tests/mlpg_grad_ref64.py (whose bounds and cases these are), the frames it must not read, determinism, autograd through
viz.synthesis.mlpg_trajectory, the trajectory loss of the shipped F0 model against a float64 restatement, and graph replay."""
import functools

import numpy as np
import pytest
import torch

import mlpg_grad_ref64 as ref
from morgana_amd import data, graphs, losses, models, ops, optim, synthetic, viz
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)         # a copy: the shared cases are read-only


def _run(name, layout, masked=True, out_dtype=torch.float32, grad_out=None):
    g, variances, windows, padding, seq_len, _, _ = ref.case(name, layout, masked)
    return ops.mlpg_backward(dev(g if grad_out is None else grad_out), dev(variances), windows, padding_size=padding,
                             seq_len=None if seq_len is None else dev(seq_len), out_dtype=out_dtype)


# ----------------------------------------------------------------------------------------------------- 1. kernel against the reference
@pytest.mark.parametrize('out_dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('layout', ref.VAR_LAYOUTS)
@pytest.mark.parametrize('name,masked', [(n, True) for n in sorted(ref.CASES)] + [('no_padding', False)])
def test_kernel_equals_the_float64_reference(name, masked, layout, out_dtype):
    want = ref.case(name, layout, masked)[5]
    n_win = len(ref.case(name, layout, masked)[2])
    got = _run(name, layout, masked, out_dtype)
    assert got.dtype == out_dtype and tuple(got.shape) == want.shape
    got = got.cpu().numpy().astype(np.float64)
    limit = ref.bound(want, n_win, f32=out_dtype == torch.float32)
    excess = np.abs(got - want)[limit > 0] / limit[limit > 0]             # an empty item: bound 0, and 0 is what must come back
    print('%s / %s / %s: max |got - want| %.3e (max |want| %.3e), worst error / bound %.3f' % (
        name, layout, 'masked' if masked else 'seq_len=None', np.abs(got - want).max(), np.abs(want).max(), excess.max()))
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= limit).all()


# ------------------------------------------------------------------------------------------------- 2. frames past seq_len: never read
@pytest.mark.parametrize('layout', ref.VAR_LAYOUTS)
@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_frames_past_seq_len_are_not_read_and_come_back_zero(name, layout):
    g, _, _, _, seq_len, _, _ = ref.case(name, layout)
    past = np.arange(g.shape[1])[None, :] >= seq_len[:, None]
    assert past.any()
    zeroed, poisoned = g.copy(), g.copy()
    zeroed[past] = 0.0
    poisoned[past] = np.nan
    want, got = _run(name, layout, grad_out=zeroed), _run(name, layout, grad_out=poisoned)
    assert torch.equal(got, want)                         # NaN != NaN: equal bits here also means no NaN came through
    assert not got.cpu().numpy()[past].any()


# ------------------------------------------------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize('name', ['crosses_a_workgroup', 'five_point'])
def test_two_calls_give_equal_bits(name):
    assert torch.equal(_run(name, 'frame'), _run(name, 'frame'))


# ---------------------------------------------------------------------------------------------------------------------- 4. autograd
def _mse64(pred, target, seq_len):
    """losses.mse and its gradient in float64 (morgana/losses.py:29-51): mean over (b, d) of the per-utterance masked frame mean."""
    pred, target = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    bsz, t, dim = pred.shape
    mask = (np.arange(t)[None, :] < np.asarray(seq_len)[:, None])[..., None]
    n_valid = np.asarray(seq_len, np.float64)[:, None, None]
    diff = (pred - target) * mask
    return float((diff ** 2 / n_valid).sum() / (bsz * dim)), 2.0 * diff / (n_valid * bsz * dim)


def test_autograd_through_mlpg_trajectory():
    rng = np.random.RandomState(5)
    bsz, t, dim = 4, 40, 3
    seq_len = np.array([40, 23, 1, 8], np.int64)
    means = rng.standard_normal((bsz, t, 3 * dim)).astype(np.float32)
    variances = ref.make_variances(rng, 'global', bsz, t, 3 * dim)
    target = rng.standard_normal((bsz, t, dim)).astype(np.float32)
    means_dev = dev(means).requires_grad_()
    trajectory = viz.synthesis.mlpg_trajectory(means_dev, dev(variances), padding_size=7, seq_len=dev(seq_len))
    assert trajectory.requires_grad and trajectory.dtype == torch.float32
    loss = losses.mse(trajectory, dev(target), dev(seq_len))
    loss.backward()
    traj64 = ref_cpu.mlpg(means, variances, padding_size=7, seq_len=seq_len)
    want_loss, grad_traj = _mse64(traj64, target, seq_len)
    want, _ = ref.grad_means_ref(grad_traj, variances, ref.DEFAULT_WINDOWS, 7, seq_len)
    got = means_dev.grad.cpu().numpy()
    err = np.abs(got - want).max() / np.abs(want).max()
    print('loss %.8f / %.8f, means.grad: max difference / max |want| %.3e' % (loss.item(), want_loss, err))
    assert abs(loss.item() - want_loss) <= 1e-5 * abs(want_loss)
    assert err <= 1e-5
    # the reference-shaped entry point keeps its detached result, and equals the differentiable forward bit for bit
    plain = viz.synthesis.MLPG(means_dev, dev(variances), padding_size=7, seq_len=dev(seq_len))
    assert not plain.requires_grad and plain.grad_fn is None
    assert torch.equal(plain, trajectory.detach())
    with pytest.raises(ValueError, match='variances'):
        viz.synthesis.mlpg_trajectory(means_dev, dev(variances).requires_grad_(), padding_size=7)


# ------------------------------------------------------------------------------------------------------------------------- 5. model
@functools.lru_cache(maxsize=None)
def _batch_np():
    return synthetic.make_acoustic_batch(6, (30, 120), streams=(('lf0', 3, 'mse'),), seed=37, with_raw=True)


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
        feats['speaker_id'], _ = synthetic.speaker_batch_ids(len(feats['n_frames']), n_speakers=5, seed=37)
    return feats, data.to_device(feats, DEV, normalisers=model.normalisers)


def _restate(model, feats, pred_norm_deltas, rows=None):
    """The model's loss, and d loss / d prediction, in float64 from its own normalised delta outputs: denormalise (float32, as the model
    does), MLPG (oracle, float64), static normaliser, masked MSE against normalise(lf0); the delta term on the prediction itself."""
    normaliser = model.normalisers['lf0']
    n_frames = feats['n_frames']
    if rows is None:
        static, delta = normaliser.params, normaliser.delta_params
        mean_s, std_s, mean_d, std_d = static['mean'], static['std_dev'], delta['mean'], delta['std_dev']
        variances = (std_d ** 2).astype(np.float32)
    else:
        names = [normaliser.speaker_ids[r] for r in rows]
        pick = lambda params, key: np.stack([params[n][key] for n in names])[:, None, :]          # noqa: E731  (B, 1, D)
        mean_s, std_s = pick(normaliser.params, 'mean'), pick(normaliser.params, 'std_dev')
        mean_d, std_d = pick(normaliser.delta_params, 'mean'), pick(normaliser.delta_params, 'std_dev')
        variances = (std_d[:, 0, :] ** 2).astype(np.float32)                                      # (B, W D): per item
    deltas = (pred_norm_deltas * std_d + mean_d).astype(np.float32)
    if rows is None:
        trajectory = ref_cpu.mlpg(deltas, variances, padding_size=100, seq_len=n_frames)
    else:
        expanded = np.broadcast_to(variances[:, None, :], deltas.shape)
        trajectory = ref_cpu.mlpg(deltas, expanded, padding_size=100, seq_len=n_frames)
    scale = 1.0 / (std_s.astype(np.float64) + 1e-8)
    target = (feats['lf0'].astype(np.float64) - mean_s) * scale
    term, grad_norm_traj = _mse64((trajectory - mean_s) * scale, target, n_frames)
    delta_loss, grad_delta = _mse64(pred_norm_deltas, feats['normalised_lf0_deltas'], n_frames)
    grad_means, _ = ref.grad_means_ref(grad_norm_traj * scale, variances, ref.DEFAULT_WINDOWS, 100, n_frames)
    return delta_loss, term, grad_delta + grad_means * std_d, trajectory


def test_model_loss_and_gradient_equal_the_float64_restatement():
    model = _model(trajectory_weight=1.)
    feats, batch = _batch(model)
    loss, out = model(batch)
    assert out['lf0'].requires_grad
    loss.backward()
    last = model.layers[12]
    got_grad = last.weight.grad.cpu().numpy().copy()
    delta_loss, term, grad_pred, trajectory = _restate(model, feats, out['normalised_lf0_deltas'].detach().cpu().numpy())
    want = delta_loss + term
    print('loss %.8f, restated %.8f (delta %.8f + trajectory %.8f)' % (loss.item(), want, delta_loss, term))
    assert term > 1e-3 * delta_loss                        # the term is there to be seen
    assert abs(loss.item() - want) <= 1e-4 * abs(want)
    got_traj = out['lf0'].detach().cpu().numpy()
    assert np.abs(got_traj - trajectory).max() <= 1e-5 * np.abs(trajectory).max()
    # chain rule: the restated d loss / d prediction pushed through the stack's own backward
    model.zero_grad()
    _, again = model(batch)
    again['normalised_lf0_deltas'].backward(dev(grad_pred.astype(np.float32)))
    want_grad = last.weight.grad.cpu().numpy()
    err = np.abs(got_grad - want_grad).max() / np.abs(want_grad).max()
    print('d loss / d last weight: max difference / max |want| %.3e' % err)
    assert np.abs(want_grad).max() > 0 and err <= 1e-4
    # the metric reads the same trajectory, detached
    assert model.metrics.results_as_json_dict('train')['LF0_RMSE_Hz'] > 0


def test_model_loss_with_speaker_dependent_normalisers():
    model = _model(speakers=True, trajectory_weight=1.)
    feats, batch = _batch(model, speakers=True)
    loss, out = model(batch)
    rows = model.normalisers['lf0'].speaker_rows(feats['speaker_id'])
    delta_loss, term, _, _ = _restate(model, feats, out['normalised_lf0_deltas'].detach().cpu().numpy(), rows=rows)
    want = delta_loss + term
    print('loss %.8f, restated %.8f (delta %.8f + trajectory %.8f)' % (loss.item(), want, delta_loss, term))
    assert abs(loss.item() - want) <= 1e-4 * abs(want)
    loss.backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())


def test_weight_zero_is_the_model_of_today_bit_for_bit():
    results = []
    for kwargs in ({}, {'trajectory_weight': 0.}):
        model = _model(**kwargs)
        _, batch = _batch(model)
        loss, out = model(batch)
        loss.backward()
        assert not out['lf0'].requires_grad
        results.append((loss.detach().clone(), out['lf0'].clone(), [p.grad.clone() for p in model.parameters()]))
    (loss_a, traj_a, grads_a), (loss_b, traj_b, grads_b) = results
    assert torch.equal(loss_a, loss_b) and torch.equal(traj_a, traj_b)
    assert len(grads_a) == len(grads_b) and all(torch.equal(a, b) for a, b in zip(grads_a, grads_b))
    # and the weight changes the loss and the gradients
    model = _model(trajectory_weight=1.)
    loss, _ = model(_batch(model)[1])
    assert loss.item() != loss_a.item()


# ------------------------------------------------------------------------------------------------------------------------- 6. graph
def test_graphed_steps_equal_eager_steps():
    """graphs.GraphedTrainStep on the model of check 5: two eager warm-up steps, the capture, then three replays - parameters, both Adam
    moments and the losses EQUAL bit for bit to five eager steps (the same kernels in the same order on the same data)."""
    def fresh():
        model = _model(trajectory_weight=1.)
        return model, optim.Adam(model.parameters(), lr=0.01), _batch(model)[1]

    model_e, opt_e, batch = fresh()
    losses_e = []
    for _ in range(5):
        opt_e.zero_grad()
        loss, _ = model_e(batch)
        loss.backward()
        opt_e.step()
        losses_e.append(loss.item())
    model_g, opt_g, batch = fresh()
    step = graphs.GraphedTrainStep(model_g, opt_g, batch, warmup=2)
    assert step.steps_done == 2
    losses_g = [step().clone() for _ in range(3)]
    assert [v.item() for v in losses_g] == losses_e[2:]
    flat_e, flat_g = opt_e.flat_buffers(), opt_g.flat_buffers()
    assert flat_e['step'] == flat_g['step'] == 5
    for key in ('param', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(flat_e[key], flat_g[key]), key
