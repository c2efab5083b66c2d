"""The variance gradient of MLPG on the device (run with ``-m gpu`` on an MI355X): mg_mlpg_grad_mv_f32 against the dense float64
reference of tests/mlpg_var_grad_ref64.py (whose bounds and cases these are), bit equality of its grad_means with mg_mlpg_grad_f32,
the frames it must not read, determinism, autograd through viz.synthesis.mlpg_trajectory(variance_grad=True), a 'gaussian' stream
trained through trajectory and global-variance terms against a float64 torch restatement, and graph replay."""
import functools

import numpy as np
import pytest
import torch

import mlpg_var_grad_ref64 as ref
from morgana_amd import _lib, data, graphs, losses, models, ops, optim, synthetic, viz
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CASE_IDS = [(n, True) for n in sorted(ref.VAR_CASES)] + [(n, False) for n in sorted(ref.VAR_CASES)]


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)         # a copy: the shared cases are read-only


def _run(name, masked=True, out_dtype=torch.float32, grad_out=None, means=None, variances=None):
    g, mu, var, windows, padding, seq_len, _ = ref.case(name, masked)
    return ops.mlpg_backward_mv(dev(g if grad_out is None else grad_out), dev(mu if means is None else means),
                                dev(var if variances is None else variances), windows, padding_size=padding,
                                seq_len=None if seq_len is None else dev(seq_len), out_dtype=out_dtype)


# ----------------------------------------------------------------------------------------------------- 1. kernel against the reference
@pytest.mark.parametrize('out_dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('name,masked', CASE_IDS)
def test_kernel_equals_the_float64_reference(name, masked, out_dtype):
    _, _, _, windows, _, _, want = ref.case(name, masked)
    got_means, got_vars = _run(name, masked, out_dtype)
    f32 = out_dtype == torch.float32
    for what, got, wanted, limit in (
            ('grad_means', got_means, want['grad_means'], ref.bound_means(want['grad_means'], len(windows), f32=f32)),
            ('grad_variances', got_vars, want['grad_variances'], ref.bound_variances(want['grad_variances'], want['scale'], f32=f32))):
        assert got.dtype == out_dtype and tuple(got.shape) == wanted.shape
        got = got.cpu().numpy().astype(np.float64)
        err = np.abs(got - wanted)
        excess = err[limit > 0] / limit[limit > 0]        # an empty item: bound 0, and 0 is what must come back
        print('%s / %s / %s: max |got - want| %.3e (max |want| %.3e), worst error / bound %.3f' % (
            name, 'masked' if masked else 'seq_len=None', what, err.max(), np.abs(wanted).max(), excess.max()))
        assert np.isfinite(got).all()
        assert (err <= limit).all()


@pytest.mark.parametrize('out_dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('name,masked', CASE_IDS)
def test_grad_means_is_bit_equal_to_the_means_only_backward(name, masked, out_dtype):
    g, _, var, windows, padding, seq_len, _ = ref.case(name, masked)
    alone = ops.mlpg_backward(dev(g), dev(var), windows, padding_size=padding, seq_len=None if seq_len is None else dev(seq_len),
                              out_dtype=out_dtype)
    assert torch.equal(_run(name, masked, out_dtype)[0], alone)


# ------------------------------------------------------------------------------------------------- 2. frames past seq_len: never read
@pytest.mark.parametrize('name', sorted(ref.VAR_CASES))
def test_frames_past_seq_len_are_not_read_and_come_back_zero(name):
    g, mu, var, _, _, seq_len, _ = ref.case(name)
    past = np.arange(g.shape[1])[None, :] >= seq_len[:, None]
    assert past.any()
    poisoned = [a.copy() for a in (g, mu, var)]
    for a in poisoned:
        a[past] = np.nan
    want = _run(name)
    got = _run(name, grad_out=poisoned[0], means=poisoned[1], variances=poisoned[2])
    for a, b in zip(got, want):
        assert torch.equal(a, b)                          # NaN != NaN: equal bits here also means no NaN came through
        values = a.cpu().numpy()
        assert np.isfinite(values).all() and not values[past].any()
        assert np.abs(values[~past]).max() > 0


# ------------------------------------------------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize('name', ['crosses_a_workgroup', 'five_point'])
def test_two_calls_give_equal_bits(name):
    first, second = _run(name), _run(name)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


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
    """d losses.mse(trajectory) / d (means, variances) through MLPGVarFn against the reference fed the float64 restatement of the loss's
    gradient.  The device's upstream gradient comes from its float32 trajectory: 2^-24 of |trajectory| against a difference
    trajectory - target of the same size, a few 1e-7 of it; both gradients are linear in it, and 1e-5 of their largest entry is the
    bound test_gpu_mlpg_grad.py holds the means' gradient to in the same setting."""
    rng = np.random.RandomState(6)
    bsz, t, dim = 4, 40, 3
    seq_len = np.array([40, 23, 1, 8], np.int64)
    means = rng.standard_normal((bsz, t, 3 * dim)).astype(np.float32)
    variances = (rng.uniform(0.2, 0.6, (bsz, t, 3 * dim)).astype(np.float32) ** 2).astype(np.float32)
    target = rng.standard_normal((bsz, t, dim)).astype(np.float32)
    means_dev, var_dev = dev(means).requires_grad_(), dev(variances).requires_grad_()
    trajectory = viz.synthesis.mlpg_trajectory(means_dev, var_dev, padding_size=7, seq_len=dev(seq_len), variance_grad=True)
    assert trajectory.requires_grad and trajectory.dtype == torch.float32
    loss = losses.mse(trajectory, dev(target), dev(seq_len))
    loss.backward()
    traj64 = ref_cpu.mlpg(means, variances, padding_size=7, seq_len=seq_len)
    want_loss, grad_traj = _mse64(traj64, target, seq_len)
    want = ref.grads_ref(grad_traj, means, variances, ref.DEFAULT_WINDOWS, 7, seq_len)
    assert abs(loss.item() - want_loss) <= 1e-5 * abs(want_loss)
    for what, got, wanted in (('means', means_dev.grad, want['grad_means']), ('variances', var_dev.grad, want['grad_variances'])):
        err = np.abs(got.cpu().numpy() - wanted).max() / np.abs(wanted).max()
        print('%s.grad: max difference / max |want| %.3e' % (what, err))
        assert err <= 1e-5
    # the forward is the forward of before; constant variances take the means-only layer and get the same means' gradient, bit for bit
    plain = viz.synthesis.MLPG(means_dev, var_dev, padding_size=7, seq_len=dev(seq_len))
    assert torch.equal(plain, trajectory.detach())
    again = dev(means).requires_grad_()
    losses.mse(viz.synthesis.mlpg_trajectory(again, dev(variances), padding_size=7, seq_len=dev(seq_len)), dev(target), dev(seq_len)).backward()
    assert torch.equal(again.grad, means_dev.grad)
    with pytest.raises(ValueError, match='variance_grad=True'):
        viz.synthesis.mlpg_trajectory(means_dev, var_dev, padding_size=7)


# ------------------------------------------------------------------------------------------------------------------------- 5. model
@functools.lru_cache(maxsize=None)
def _batch_np():
    return synthetic.make_acoustic_batch(2, (30, 40), streams=(('lf0', 3, 'mse'),), seed=43, with_raw=True)


def _model(speakers=False, **kwargs):
    if speakers:
        kwargs['speaker_id_list'] = 'speakers.scp'
    model = models.GRUF0Model(precision='fp32', **kwargs).to(DEV)
    own = model.state_dict()
    for key, value in synthetic.gru_f0_state(output_dim=model.streams[0].width).items():
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
        feats['speaker_id'], _ = synthetic.speaker_batch_ids(len(feats['n_frames']), n_speakers=5, seed=43)
    return feats, data.to_device(feats, DEV, normalisers=model.normalisers)


def _step(model, batch):
    calls = []
    _lib.CALL_LOG = calls
    try:
        loss, out = model(batch)
        loss.backward()
    finally:
        _lib.CALL_LOG = None
    return loss.detach().clone(), out, [p.grad.clone() for p in model.parameters()], calls


def _masked_mean64(term, n_frames):
    """mean over (b, d) of the per-utterance mean over the valid frames, float64 torch."""
    t = term.shape[1]
    mask = (torch.arange(t)[None, :] < n_frames[:, None])[..., None]
    return ((term * mask).sum(dim=1) / n_frames.double()[:, None]).mean()


def _restate(model, feats, prediction, rows=None, trajectory_weight=1., gv_weight=0.5, eps=1e-6):
    """The loss of a 'gaussian' lf0 stream with both trajectory terms, float64 torch on the CPU from the model's own prediction
    tensor (B, T, 6), every step restated: the Gaussian likelihood, denormalisation, a DENSE MLPG (torch.linalg.solve on
    P = sum_w W^T diag(1 / var) W per utterance and dimension, padding 100), the static normaliser, masked MSE and the log
    global-variance gap.  Autograd supplies d loss / d prediction, the variance path included, with nothing of the kernel's algebra."""
    normaliser = model.normalisers['lf0']
    n_frames = torch.tensor(feats['n_frames'], dtype=torch.int64)
    bsz = len(n_frames)
    if rows is None:
        static, delta = normaliser.params, normaliser.delta_params
        pick = lambda params, key: torch.tensor(np.broadcast_to(params[key], (bsz,) + params[key].shape).astype(np.float64))[:, None, :]   # noqa: E731
    else:
        names = [normaliser.speaker_ids[r] for r in rows]
        static, delta = normaliser.params, normaliser.delta_params
        pick = lambda params, key: torch.tensor(np.stack([params[n][key] for n in names]).astype(np.float64))[:, None, :]      # noqa: E731
    mean_s, std_s, mean_d, std_d = pick(static, 'mean'), pick(static, 'std_dev'), pick(delta, 'mean'), pick(delta, 'std_dev')
    pred = torch.tensor(prediction, dtype=torch.float64, requires_grad=True)
    dim = 3
    nll = _masked_mean64(losses.gaussian_nll(pred, torch.tensor(feats['normalised_lf0_deltas'], dtype=torch.float64)), n_frames)
    deltas = pred[..., :dim] * std_d + mean_d
    variances = torch.exp(2. * pred[..., dim:]) * std_d ** 2
    padding = 100
    trajectory = torch.zeros(bsz, pred.shape[1], 1, dtype=torch.float64)
    rows_out = []
    for b in range(bsz):
        length = int(n_frames[b])
        n = length + 2 * padding
        frames = torch.tensor(np.clip(np.arange(n) - padding, 0, length - 1))
        p_mat, rhs = torch.zeros(n, n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        for w, window in enumerate(ref.DEFAULT_WINDOWS):
            mat = torch.tensor(ref.window_matrix(window, n))
            tau = 1. / variances[b, frames, w]
            p_mat = p_mat + mat.T @ (tau[:, None] * mat)
            rhs = rhs + mat.T @ (tau * deltas[b, frames, w])
        x = torch.linalg.solve(p_mat, rhs)[padding:padding + length]
        rows_out.append(torch.cat([x, torch.zeros(pred.shape[1] - length, dtype=torch.float64)]))
    trajectory = torch.stack(rows_out)[..., None]
    scale = 1. / (std_s + 1e-8)
    norm_traj = (trajectory - mean_s) * scale
    target = (torch.tensor(feats['lf0'], dtype=torch.float64) - mean_s) * scale
    mse = _masked_mean64((norm_traj - target) ** 2, n_frames)
    mask = (torch.arange(pred.shape[1])[None, :] < n_frames[:, None])[..., None]
    count = n_frames.double()[:, None]

    def variance(x):
        mean = (x * mask).sum(dim=1) / count
        return (((x - mean[:, None, :]) * mask) ** 2).sum(dim=1) / count

    gv = ((torch.log(variance(norm_traj) + eps) - torch.log(variance(target) + eps)) ** 2).mean()
    total = nll + trajectory_weight * mse + gv_weight * gv
    total.backward()
    return dict(loss=total.item(), nll=nll.item(), mse=mse.item(), gv=gv.item(), grad=pred.grad.numpy(),
                trajectory=trajectory.detach().numpy())


@pytest.mark.parametrize('speakers', [False, True], ids=['global', 'per_speaker'])
def test_gaussian_stream_loss_and_gradient_equal_the_float64_restatement(speakers):
    """Loss and d loss / d prediction of a 'gaussian' lf0 stream with trajectory_weight=1 and gv_weight=0.5.  The bound is the one
    test_gpu_mlpg_grad.py::test_model_loss_and_gradient_equal_the_float64_restatement holds the means-only model to, 1e-4 of the loss
    and 1e-4 of the largest gradient entry, for its reason: the device runs the chain in float32 - exp, denormalise, the float32
    trajectory, normalise - each step 2^-24 = 6e-8 of its result, and the static normaliser subtracts a mean of 5 from a trajectory
    around 5 and divides by a standard deviation of 0.2 to 0.6, which amplifies the trajectory's rounding by up to 5 / 0.2 = 25, to
    1.5e-6 of the normalised value; the squared gap of log variances and the sums over up to 40 frames take that to a few 1e-6 of
    the loss and, through the variances' 1 / n-weighted differences, some 1e-5 of the largest gradient entry.  Means and log standard
    deviations are compared each against their own largest entry, so that the variance path cannot hide behind the means'."""
    model = _model(speakers, predict_variance=True, trajectory_weight=1., gv_weight=0.5)
    feats, batch = _batch(model, speakers)
    assert batch['n_frames'].shape[0] == 2 and batch['lf0'].shape[1] <= 40
    loss, out = model(batch)
    assert set(out) == {'lf0_gaussian', 'normalised_lf0_deltas', 'normalised_lf0_deltas_variance', 'lf0'}
    assert out['lf0'].requires_grad and out['normalised_lf0_deltas_variance'].requires_grad
    prediction = out['lf0_gaussian']
    assert tuple(prediction.shape)[2] == 6
    prediction.retain_grad()
    calls = []
    _lib.CALL_LOG = calls
    try:
        loss.backward()
    finally:
        _lib.CALL_LOG = None
    assert calls.count('mg_mlpg_grad_mv_f32') == 1 and 'mg_mlpg_grad_f32' not in calls
    rows = model.normalisers['lf0'].speaker_rows(feats['speaker_id']) if speakers else None
    want = _restate(model, feats, prediction.detach().cpu().numpy(), rows=rows)
    print('loss %.8f, restated %.8f (nll %.8f + trajectory %.8f + 0.5 * gv %.8f)' % (loss.item(), want['loss'], want['nll'], want['mse'], want['gv']))
    assert want['mse'] > 1e-3 * abs(want['nll']) and want['gv'] > 1e-3 * abs(want['nll'])          # the terms are there to be seen
    assert abs(loss.item() - want['loss']) <= 1e-4 * abs(want['loss'])
    got_traj = out['lf0'].detach().cpu().numpy()
    assert np.abs(got_traj - want['trajectory']).max() <= 1e-5 * np.abs(want['trajectory']).max()
    got = prediction.grad.cpu().numpy()
    n_frames = feats['n_frames']
    past = np.arange(got.shape[1])[None, :] >= n_frames[:, None]
    for what, cols in (('means', slice(0, 3)), ('log standard deviations', slice(3, 6))):
        err = np.abs(got[:, :, cols] - want['grad'][:, :, cols]).max() / np.abs(want['grad'][:, :, cols]).max()
        print('d loss / d %s: max difference / max |want| %.3e' % (what, err))
        assert np.abs(want['grad'][:, :, cols]).max() > 0 and err <= 1e-4
    assert not got[past].any()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
    assert model.metrics.results_as_json_dict('train')['LF0_RMSE_Hz'] > 0


def test_without_weights_the_outputs_are_detached_and_mlpg_runs_per_frame():
    model = _model(predict_variance=True, min_log_std=-1.)
    _, batch = _batch(model)
    loss, out, grads, calls = _step(model, batch)
    assert not out['lf0'].requires_grad and not out['normalised_lf0_deltas'].requires_grad
    assert not out['normalised_lf0_deltas_variance'].requires_grad and out['lf0_gaussian'].requires_grad
    assert calls.count('mg_mlpg_f32') == 1 and not any(c.startswith('mg_mlpg_grad') for c in calls)
    raw = out['lf0_gaussian'].detach()
    assert torch.equal(out['normalised_lf0_deltas'], raw[..., :3])
    assert torch.equal(out['normalised_lf0_deltas_variance'], torch.exp(2. * torch.clamp(raw[..., 3:], min=-1.)))
    normaliser = model.normalisers['lf0']
    std_dev = normaliser.delta_params_torch['std_dev'].to(device=DEV, dtype=torch.float32)
    by_hand = ops.mlpg(normaliser.denormalise(raw[..., :3], deltas=True), out['normalised_lf0_deltas_variance'] * std_dev ** 2,
                       viz.synthesis.DEFAULT_WINDOWS, padding_size=100, seq_len=batch['n_frames'])
    assert torch.equal(out['lf0'], by_hand)
    # the loss is losses.gaussian of the raw slice
    assert torch.equal(loss, losses.gaussian(raw, batch['normalised_lf0_deltas'], batch['n_frames'], min_log_std=-1.))
    assert all(torch.isfinite(g).all() for g in grads)


def test_models_without_a_gaussian_stream_are_the_models_of_today():
    for kwargs in ({}, {'trajectory_weight': 1., 'gv_weight': 1.}, {'n_components': 2}):
        results = []
        for extra in ({}, {'predict_variance': False}):
            model = _model(**dict(kwargs, **extra))
            loss, out, grads, calls = _step(model, _batch(model)[1])
            assert 'mg_mlpg_grad_mv_f32' not in calls
            results.append((loss, out['lf0'].detach().clone(), grads, calls))
        (loss_a, traj_a, grads_a, calls_a), (loss_b, traj_b, grads_b, calls_b) = results
        assert torch.equal(loss_a, loss_b) and torch.equal(traj_a, traj_b) and calls_a == calls_b
        assert len(grads_a) == len(grads_b) and all(torch.equal(a, b) for a, b in zip(grads_a, grads_b))
    assert calls_a.count('mg_mlpg_f32') == 1


# ------------------------------------------------------------------------------------------------------------------------- 6. graph
def test_graphed_steps_equal_eager_steps():
    """graphs.GraphedTrainStep on the variance-predicting model with both trajectory terms: two eager warm-up steps, the capture, one
    replay - parameters, both Adam moments and the loss EQUAL bit for bit to three eager steps."""
    def fresh():
        model = _model(predict_variance=True, trajectory_weight=1., gv_weight=1.)
        return model, optim.Adam(model.parameters(), lr=0.01), _batch(model)[1]

    model_e, opt_e, batch = fresh()
    losses_e = []
    for _ in range(3):
        opt_e.zero_grad()
        loss, _ = model_e(batch)
        loss.backward()
        opt_e.step()
        losses_e.append(loss.item())
    model_g, opt_g, batch = fresh()
    step = graphs.GraphedTrainStep(model_g, opt_g, batch, warmup=2)
    assert step.steps_done == 2
    replayed = step().clone()
    assert np.isfinite(losses_e).all() and replayed.item() == losses_e[2]
    flat_e, flat_g = opt_e.flat_buffers(), opt_g.flat_buffers()
    assert flat_e['step'] == flat_g['step'] == 3
    for key in ('param', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(flat_e[key], flat_g[key]), key
