"""Host-side checks of the mixture-density loss (no GPU): the float64 restatement (tests/mdn_ref64.py) against torch.distributions and
against finite differences, two honest fp32 evaluations that are not the kernel inside the derived fp32 bound on every sweep input,
the floor rule, argument validation of mg_masked_mdn_f32 / mg_mdn_select_f32, and what the host layers know and refuse."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import mdn_ref64
from morgana_amd import _lib, losses, models, utils

C32 = np.float32(mdn_ref64.HALF_LOG_2PI)


def _mask(seq_len, b, t):
    n = mdn_ref64.valid_frames(seq_len, b, t)
    return np.arange(t)[None, :] < n[:, None], n


# ------------------------------------------------------------------------------------------ float64: torch.distributions, differences
def _mixture_same_family(pred, target, seq_len, k):
    """Loss and autograd gradient of the definition through torch.distributions, float64, CPU."""
    from torch.distributions import Categorical, Independent, MixtureSameFamily, Normal
    b, t, d = target.shape
    x = torch.from_numpy(np.asarray(pred, dtype=np.float64)).requires_grad_(True)
    y = torch.from_numpy(np.asarray(target, dtype=np.float64))
    logits, mu, s = x[:, :, :k], x[:, :, k:k + k * d].reshape(b, t, k, d), x[:, :, k + k * d:].reshape(b, t, k, d)
    mixture = MixtureSameFamily(Categorical(logits=logits), Independent(Normal(mu, torch.exp(s)), 1))
    frame = -mixture.log_prob(y) / d
    mask, n = _mask(seq_len, b, t)
    loss = torch.mean(torch.sum(frame * torch.from_numpy(mask), dim=1) / torch.from_numpy(n.astype(np.float64)))
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


@pytest.mark.parametrize('k, d', mdn_ref64.SWEEP)
def test_ref64_equals_mixture_same_family(k, d):
    pred, target, seq_len = mdn_ref64.sweep_case(k, d)
    ref = mdn_ref64.mdn(pred, target, seq_len, k)
    loss, grad = _mixture_same_family(pred, target, seq_len, k)
    assert abs(ref['loss'] - loss) <= 1e-12 * abs(loss), (ref['loss'], loss)
    assert np.abs(ref['grad'] - grad).max() <= 1e-12 * np.abs(grad).max()
    assert np.all(ref['grad'][~ref['mask']] == 0.0) and np.isfinite(ref['grad']).all()
    assert ref['responsibility'][ref['mask']].min() < 0.5 or k == 1


def test_ref64_gradient_equals_central_differences():
    rng = np.random.RandomState(7)
    k, d, t = 2, 3, 4
    pred = rng.standard_normal((1, t, mdn_ref64.width(k, d)))
    target = rng.standard_normal((1, t, d))
    seq_len = np.array([3])
    ref = mdn_ref64.mdn(pred, target, seq_len, k)
    h = 1e-5
    numeric = np.zeros_like(pred)
    for index in np.ndindex(*pred.shape):
        up, down = pred.copy(), pred.copy()
        up[index] += h
        down[index] -= h
        numeric[index] = (mdn_ref64.mdn(up, target, seq_len, k)['loss'] - mdn_ref64.mdn(down, target, seq_len, k)['loss']) / (2 * h)
    assert np.abs(numeric - ref['grad']).max() <= 1e-7 * np.abs(ref['grad']).max()
    assert np.all(numeric[0, 3] == 0.0) and np.all(ref['grad'][0, 3] == 0.0)


def test_ref64_floor_rule():
    """min_log_std: the loss is the evaluation at max(s, floor), a floored s gets gradient 0, the others the clamped point's gradient."""
    k, d = 4, 3
    pred, target, seq_len = mdn_ref64.sweep_case(k, d)
    floor = -0.5                                            # the sweep's log-stds are -0.5 + noise: about half lie below
    _, _, s = mdn_ref64.split(pred, k, d)
    below = s < floor
    assert 0.3 < below.mean() < 0.7
    clamped = pred.copy()
    clamped[:, :, k + k * d:] = np.maximum(s, floor).reshape(pred.shape[0], pred.shape[1], k * d)
    ref, want = mdn_ref64.mdn(pred, target, seq_len, k, min_log_std=floor), mdn_ref64.mdn(clamped, target, seq_len, k)
    assert ref['loss'] == want['loss'] and np.array_equal(ref['frame_loss'], want['frame_loss'])
    g_s, want_s = ref['grad'][:, :, k + k * d:].reshape(s.shape), want['grad'][:, :, k + k * d:].reshape(s.shape)
    assert np.all(g_s[below] == 0.0) and np.array_equal(g_s[~below], want_s[~below]) and np.any(want_s[below] != 0.0)
    assert np.array_equal(ref['grad'][:, :, :k + k * d], want['grad'][:, :, :k + k * d])
    assert np.array_equal(ref['variance'], np.where(ref['mask'][:, :, None], np.exp(2 * np.maximum(
        np.take_along_axis(s.astype(np.float64), ref['component'][:, :, None, None], axis=2)[:, :, 0], floor)), 1.0))
    # torch.clamp's autograd agrees (float64)
    x = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    parts = torch.cat((x[:, :, :k + k * d], torch.clamp(x[:, :, k + k * d:], min=floor)), dim=2)
    b, t, _ = pred.shape
    from torch.distributions import Categorical, Independent, MixtureSameFamily, Normal
    mix = MixtureSameFamily(Categorical(logits=parts[:, :, :k]),
                            Independent(Normal(parts[:, :, k:k + k * d].reshape(b, t, k, d), torch.exp(parts[:, :, k + k * d:].reshape(b, t, k, d))), 1))
    mask, n = _mask(seq_len, b, t)
    loss = torch.mean(torch.sum(-mix.log_prob(torch.from_numpy(target.astype(np.float64))) / d * torch.from_numpy(mask), dim=1)
                      / torch.from_numpy(n.astype(np.float64)))
    loss.backward()
    assert abs(float(loss.detach()) - ref['loss']) <= 1e-12 * abs(ref['loss'])
    assert np.abs(x.grad.numpy() - ref['grad']).max() <= 1e-12 * np.abs(ref['grad']).max()


def test_ref64_edge_semantics():
    k, d = 4, 3
    pred, target, seq_len = mdn_ref64.sweep_case(k, d)
    ref = mdn_ref64.mdn(pred, target, seq_len, k)
    assert np.all(ref['component'][1, 20:] == 0) and np.all(ref['mean'][2, 1:] == 0.0) and np.all(ref['variance'][2, 1:] == 1.0)
    assert np.array_equal(ref['component'][ref['mask']], np.argmax(pred[:, :, :k], axis=2)[ref['mask']])
    dirty_pred, dirty_target = pred.copy(), target.copy()
    dirty_pred[~ref['mask']] = np.nan
    dirty_target[~ref['mask']] = np.nan
    dirty = mdn_ref64.mdn(dirty_pred, dirty_target, seq_len, k)
    assert dirty['loss'] == ref['loss'] and np.array_equal(dirty['grad'], ref['grad'])
    assert np.isnan(mdn_ref64.mdn(pred, target, np.array([37, 0, 1]), k)['loss'])
    assert mdn_ref64.mdn(pred, target, np.array([99, 20, 1]), k)['loss'] == ref['loss']
    removed = pred.copy()
    removed[:, :, 1] = -np.inf
    out = mdn_ref64.mdn(removed, target, seq_len, k)
    keep = [c for c in range(pred.shape[2]) if c != 1 and not k + d <= c < k + 2 * d and not k + k * d + d <= c < k + k * d + 2 * d]
    three = mdn_ref64.mdn(removed[:, :, keep], target, seq_len, k - 1)
    assert abs(out['loss'] - three['loss']) <= 1e-15 * abs(three['loss']) and np.all(out['grad'][:, :, 1] == 0.0)
    assert np.all(out['grad'][:, :, k + d:k + 2 * d] == 0.0) and np.isfinite(out['grad']).all() and np.isfinite(out['grad_bound']).all()
    removed[:, :, :k] = -np.inf
    assert np.isnan(mdn_ref64.mdn(removed, target, seq_len, k)['loss'])
    assert mdn_ref64.depth(3) == 2 and mdn_ref64.depth(64) == 63 and mdn_ref64.depth(180) == 31 and mdn_ref64.depth(1024) == 136


# ------------------------------------------------------------------------------------------------ fp32: is the bound honest?
def _fp32_torch(pred, target, seq_len, k):
    """Section 1 of the definition in float32 torch ops on the CPU, in the natural order."""
    b, t, d = target.shape
    x, y = torch.from_numpy(pred), torch.from_numpy(target)
    a, mu, s = x[:, :, :k], x[:, :, k:k + k * d].reshape(b, t, k, d), x[:, :, k + k * d:].reshape(b, t, k, d)
    es = torch.exp(-s)
    z = (y[:, :, None, :] - mu) * es
    q = torch.log_softmax(a, dim=-1) - (0.5 * z * z + s).sum(dim=-1) - d * float(C32)
    lse = torch.logsumexp(q, dim=-1)
    frame = -lse / d
    mask, n = _mask(seq_len, b, t)
    mask_t, n_t = torch.from_numpy(mask), torch.from_numpy(n.astype(np.float32))
    loss = torch.mean(torch.sum(torch.where(mask_t, frame, torch.zeros(())), dim=1) / n_t)
    r = torch.exp(q - lse[:, :, None])
    coef = (1.0 / (d * n_t * b))[:, None, None]
    g_a = coef * (torch.softmax(a, dim=-1) - r)
    g_mu = -(coef * r)[:, :, :, None] * z * es
    g_s = (coef * r)[:, :, :, None] * (1.0 - z * z)
    grad = torch.cat((g_a, g_mu.reshape(b, t, k * d), g_s.reshape(b, t, k * d)), dim=2)
    grad = torch.where(mask_t[:, :, None], grad, torch.zeros(()))
    assert frame.dtype == loss.dtype == grad.dtype == torch.float32
    return frame.numpy(), float(loss), grad.numpy()


def _fp32_numpy_reversed(pred, target, seq_len, k):
    """The same in float32 numpy with the sum over d taken from the last dimension to the first, the logits' and the components'
    logsumexp written out (maximum subtracted) and the responsibilities as a quotient."""
    f = np.float32
    b, t, d = target.shape
    a, mu, s = mdn_ref64.split(pred, k, d)
    with np.errstate(all='ignore'):
        es = np.exp(-s)
        z = (target[:, :, None, :] - mu) * es
        big_s = (f(0.5) * z * z + s)[:, :, :, ::-1].sum(axis=3, dtype=f)
        amax = a.max(axis=2, keepdims=True)
        ea = np.exp(a - amax)
        sa = ea.sum(axis=2, keepdims=True, dtype=f)
        q = ((a - (amax + np.log(sa))) - big_s) - f(d) * C32
        qmax = q.max(axis=2, keepdims=True)
        eq = np.exp(q - qmax)
        sq = eq.sum(axis=2, keepdims=True, dtype=f)
        frame = -(qmax + np.log(sq))[:, :, 0] / f(d)
        mask, n = _mask(seq_len, b, t)
        nf = n.astype(f)
        loss = (np.where(mask, frame, f(0)).sum(axis=1, dtype=f) / nf).sum(dtype=f) / f(b)
        r = eq / sq
        coef = (f(1) / (f(d) * nf * f(b)))[:, None, None]
        g_a = coef * (ea / sa - r)
        g_mu = -(coef * r)[:, :, :, None] * z * es
        g_s = (coef * r)[:, :, :, None] * (f(1) - z * z)
    grad = np.where(mask[:, :, None], np.concatenate((g_a, g_mu.reshape(b, t, k * d), g_s.reshape(b, t, k * d)), axis=2), f(0))
    assert frame.dtype == grad.dtype == f and np.asarray(loss).dtype == f
    return frame, float(loss), grad


def _inside_the_bound(label, k, d, pred, target, seq_len):
    ref = mdn_ref64.mdn(pred, target, seq_len, k)
    mask = ref['mask']
    for name, evaluate in (('torch', _fp32_torch), ('numpy reversed', _fp32_numpy_reversed)):
        frame, loss, grad = evaluate(pred, target, seq_len, k)
        err = np.abs(frame.astype(np.float64) - ref['frame_loss'])[mask]
        frame_ratio = float((err / ref['frame_bound'][mask]).max())
        loss_ratio = abs(loss - ref['loss']) / ref['loss_bound']
        gerr = np.abs(grad.astype(np.float64) - ref['grad'])
        grad_ratio = float((gerr / np.maximum(ref['grad_bound'], 1e-300)).max())
        print('%s %s: worst error / bound: frame %.3f, loss %.3f, gradient %.3f' % (label, name, frame_ratio, loss_ratio, grad_ratio))
        assert np.all(err <= ref['frame_bound'][mask]), (name, frame_ratio)
        assert abs(loss - ref['loss']) <= ref['loss_bound'], (name, loss_ratio)
        assert np.all(gerr <= ref['grad_bound']), (name, grad_ratio)
        assert np.all(grad[~mask] == 0.0) and np.isfinite(grad).all() and np.isfinite(loss)
    return ref


@pytest.mark.parametrize('k, d', mdn_ref64.SWEEP)
def test_fp32_evaluations_sit_inside_the_derived_bound(k, d):
    """The bound must hold for honest fp32 evaluations that are not the kernel, per frame, in total and for EVERY gradient element.
    The worst error / bound is printed: a ratio far below 1e-3 would mean a vacuous bound."""
    pred, target, seq_len = mdn_ref64.sweep_case(k, d)
    ref = _inside_the_bound('K=%d D=%d' % (k, d), k, d, pred, target, seq_len)
    mask = ref['mask']
    # a rounding bound, not a tolerance: it stays a small multiple of roundoff on the loss's own scale
    assert ref['loss_bound'] <= 1e-4 * max(abs(ref['loss']), 1.0), (ref['loss_bound'], ref['loss'])
    variance32 = np.exp(np.float32(2) * np.take_along_axis(mdn_ref64.split(pred, k, d)[2], ref['component'][:, :, None, None], axis=2)[:, :, 0])
    assert np.all(np.abs(variance32.astype(np.float64) - ref['variance'])[mask] <= ref['variance_bound'][mask])


@pytest.mark.parametrize('name', ['far', 'dominant', 's_minus10', 's_plus10', 'minus_inf'])
def test_fp32_evaluations_of_the_range_cases_sit_inside_the_derived_bound(name):
    k, d, cases = mdn_ref64.range_cases()
    pred, target, seq_len = cases[name]
    ref = _inside_the_bound(name, k, d, pred, target, seq_len)
    assert np.isfinite(ref['loss']) and np.isfinite(ref['grad']).all() and np.isfinite(ref['grad_bound']).all()
    if name == 'far':                                     # what the bound says there: fp32 resolves q = -6e6 to about 0.5
        assert ref['frame_loss'][ref['mask']].min() > 1e5 and 0.01 < ref['frame_bound'][ref['mask']].max() < 10.0
    if name == 'dominant':
        assert np.sort(ref['responsibility'], axis=2)[:, :, -2][ref['mask']].max() < 1e-20
    if name == 'minus_inf':
        assert np.all(ref['grad'][:, :, :k][np.isneginf(pred[:, :, :k])] == 0.0)


def test_sweep_covers_every_kernel_regime():
    rows = sorted(k * d for k, d in mdn_ref64.SWEEP)
    for edge in (64, 128, 256, 512, mdn_ref64.REG_MAX):
        assert edge in rows and edge + 1 in rows, edge
    assert mdn_ref64.MAX_ROW in rows and max(k for k, _ in mdn_ref64.SWEEP) == mdn_ref64.MAX_COMPONENTS
    small = [d for k, d in mdn_ref64.SWEEP if k * d <= mdn_ref64.REG_MAX]
    assert mdn_ref64.SMALL_D in small and mdn_ref64.SMALL_D + 1 in small
    assert (mdn_ref64.MAX_COMPONENTS, mdn_ref64.MAX_ROW) == (_lib.MG_MDN_MAX_COMPONENTS, _lib.MG_MDN_MAX_ROW) == (64, 16384)


# ------------------------------------------------------------------------------------------------------------ the C ABI, host side
def test_mdn_entry_points_validate_their_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.mg_masked_mdn_workspace_bytes(4, 100, 8, 3) >= 4 * 7 * 4
    assert lib.mg_masked_mdn_workspace_bytes(4, 100, 16, 1024) >= 4 * 25 * 4

    def call(pred=16, ldp=56, col0=0, target=16, ldt=3, b=2, t=3, k=8, d=3, loss=16, grad=None, ldg=0, gcol0=0, ws=16, ws_bytes=1 << 20):
        return lib.mg_masked_mdn_f32(pred, ldp, col0, target, ldt, None, b, t, k, d, 0.0, 0, 1.0, 1.0, 0.0, loss, grad, ldg, gcol0, ws,
                                     ws_bytes, None)

    assert call(k=0) == -1 and 'K=0' in _lib.last_error()
    assert call(d=-3) == -1 and 'mg_masked_mdn_f32' in _lib.last_error()
    assert call(pred=None) == -1 and 'NULL' in _lib.last_error()
    assert call(target=None) == -1 and call(loss=None) == -1
    assert call(k=65, d=1, ldp=65 * 3) == -1 and 'cap of 64' in _lib.last_error()
    assert call(k=1, d=16385, ldp=2 * 16385 + 1, ldt=16385) == -1 and 'cap of 16384' in _lib.last_error()
    assert call(k=5, d=3277, ldp=5 * (1 + 2 * 3277), ldt=3277) == -1 and 'cap of 16384' in _lib.last_error()
    assert call(b=0) == -1 and call(t=0) == -1 and call(b=65536) == -1
    assert call(ldp=55) == -1 and 'ldp=55' in _lib.last_error()                    # the row stride must cover col0 + K (1 + 2 D)
    assert call(ldp=58, col0=3) == -1 and call(col0=-1) == -1
    assert call(ldt=2) == -1 and 'ldt=2' in _lib.last_error()
    assert call(grad=16, ldg=56, gcol0=1) == -1 and 'ldg=56' in _lib.last_error()
    assert call(ws=None) == -3 and call(ws_bytes=4) == -3                          # MG_EWORKSPACE
    with pytest.raises(ValueError):
        _lib.check(call(k=0), 'mg_masked_mdn_f32')

    def select(pred=16, ldp=56, col0=0, b=2, t=3, k=8, d=3, component=16, mean=16, variance=16):
        return lib.mg_mdn_select_f32(pred, ldp, col0, None, b, t, k, d, 0.0, 0, component, mean, variance, None)

    assert select(k=65, d=1, ldp=65 * 3) == -1 and 'cap of 64' in _lib.last_error()
    assert select(k=1, d=16385, ldp=2 * 16385 + 1) == -1 and 'cap of 16384' in _lib.last_error()
    assert select(mean=None) == -1 and select(ldp=55) == -1 and select(t=0) == -1 and select(col0=-1) == -1


# ------------------------------------------------------------------------------------------------------------------ host layers
def test_losses_mdn_refuses_bad_widths_dtypes_and_cpu_tensors():
    target = torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match=r'4 \* \(1 \+ 2 \* 3\) = 28'):
        losses.mdn(torch.zeros(2, 5, 27), target, n_components=4)
    with pytest.raises(ValueError):
        losses.mdn(torch.zeros(2, 5, 28), target, n_components=0)
    with pytest.raises(TypeError, match='float32'):
        losses.mdn(torch.zeros(2, 5, 28, dtype=torch.float64), target, n_components=4)
    with pytest.raises(TypeError, match='float32'):
        losses.mdn_select(torch.zeros(2, 5, 28, dtype=torch.bfloat16), 4, 3)
    with pytest.raises(ValueError):
        losses.mdn_select(torch.zeros(2, 5, 28), 4, 2)
    with pytest.raises(RuntimeError, match=r'The size of tensor a \(5\) must match the size of tensor b \(6\) at non-singleton dimension 1'):
        losses.mdn(torch.zeros(2, 5, 28), torch.zeros(2, 6, 3), n_components=4)
    with pytest.raises(_lib.MorganaHipError):                                       # the right shapes: refused for the device only
        losses.mdn(torch.zeros(2, 5, 28), target, torch.tensor([5, 2]), n_components=4)
    with pytest.raises(_lib.MorganaHipError):
        losses.mdn_select(torch.zeros(2, 5, 28), 4, 3)
    assert losses.mdn_width(4, 3) == 28 and losses.mdn_width(1, 1) == 3


def test_stream_table_knows_the_mixture_kind():
    st = models.Stream('lf0', 3, 'mdn', n_components=4, min_log_std=-3)
    assert st.is_mdn and st.is_delta and not st.is_categorical and st.output_key == 'normalised_lf0_deltas'
    assert (st.width, st.dim, st.n_components, st.min_log_std) == (28, 3, 4, -3.0)
    assert models.Stream('lf0', 3, 'mdn').width == 7                                 # one component: a Gaussian with a predicted variance
    for other in (models.Stream('lf0', 3), models.Stream('vuv', 1, 'sigmoid_bce'), models.Stream('phone', 40, 'ce'),
                  models.Stream('lf0', 3, losses.mse)):
        assert other.width == other.dim and not other.is_mdn
    for model in (models.LSTMAcousticModel(num_layers=1), models.GRUF0Model(), models.VAEF0Model()):   # the shipped tables are unchanged
        assert all(st.width == st.dim and not st.is_mdn for st in model.streams)
    with pytest.raises(ValueError, match='not a differentiable function of the weights'):
        models.Stream('lf0', 3, 'mdn', n_components=4, trajectory_weight=1.)
    with pytest.raises(ValueError, match='not a differentiable function of the weights'):
        models.Stream('lf0', 3, 'mdn', n_components=4, trajectory_loss=losses.mse)
    with pytest.raises(ValueError, match='n_components >= 1'):
        models.Stream('lf0', 3, 'mdn', n_components=0)
    with pytest.raises(ValueError, match="belong to an 'mdn' stream"):
        models.Stream('lf0', 3, 'mse', n_components=4)
    with pytest.raises(ValueError, match="belong to an 'mdn' stream"):
        models.Stream('vuv', 1, 'sigmoid_bce', min_log_std=-3.)


def test_stream_model_refuses_a_fused_mixture_loss_and_sizes_its_stack():
    streams = [models.Stream('lf0', 3, 'mdn', n_components=4), models.Stream('vuv', 1, 'sigmoid_bce')]
    layers = utils.SequentialWithRecurrent(nn.Linear(609, 16), nn.Sigmoid(), nn.Linear(16, sum(st.width for st in streams)), precision='fp32')
    with pytest.raises(ValueError, match='the one-pass multi-stream kernel has no MDN term'):
        models.StreamModel(layers, streams, fused_loss=True)
    model = models.StreamModel(layers, streams, fused_loss=False)
    assert [st.width for st in model.streams] == [28, 1]
    sources = model.normaliser_sources()
    assert sources['lf0'].use_deltas and 'vuv' not in sources
    mixture = models.GRUF0Model(n_components=4, min_log_std=-5.)
    last = [p for p in mixture.parameters()][-2:]
    assert tuple(last[0].shape) == (28, 64) and tuple(last[1].shape) == (28,)
    assert mixture.streams[0].is_mdn and mixture.streams[0].min_log_std == -5. and mixture.streams[0].metric[0] == 'LF0_RMSE_Hz'
    plain = models.GRUF0Model()
    assert tuple([p for p in plain.parameters()][-1].shape) == (3,) and plain.streams[0].loss == 'mse'
    assert sorted(plain.state_dict()) == sorted(mixture.state_dict())
    with pytest.raises(ValueError, match='not a differentiable function of the weights'):
        models.GRUF0Model(n_components=4, trajectory_weight=1.)
