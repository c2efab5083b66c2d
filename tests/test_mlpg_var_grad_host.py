"""The variance gradient of MLPG without a GPU: the dense float64 reference of tests/mlpg_var_grad_ref64.py against central differences
of the oracle's MLPG, its scale invariant, the conditioning of the cases the GPU tests run, the argument checks of
mg_mlpg_grad_mv_f32 (the library loads without a device), the refusals of the host layers and the 'gaussian' stream's loss and table."""
import ctypes

import numpy as np
import pytest
import torch

import mdn_ref64
import mlpg_var_grad_ref64 as ref
from morgana_amd import _lib, losses, models, ops
from morgana_amd.viz import synthesis
from oracle import ref_cpu

FD_STEP = 1e-5          # relative step of the central differences
# their own error, relative to the scale of the reference's floor: truncation h^2 / 6 |f'''| var^3 - the third logarithmic derivative
# of a rational function of the variances, taken as up to 10^3 of the term sizes - plus rounding 2^-52 |L| / h: both under 1e-7
FD_ALLOWANCE = 1e-7


def _input_sensitivity(windows, length, padding, tau, mu_tau, mu, grad):
    """First-order effect on dL/dvar of one system of relative 2^-24 perturbations of every float32-formed tau and mu tau (the kernel
    rounds 1 / var and mu / var to float32, the oracle does not): sum over the inputs of |change| under a one-at-a-time relative step
    through the dense system."""
    base = ref.system_grads(windows, length, padding, tau, mu_tau, mu, grad)[1]
    total = np.zeros_like(base)
    step = 2.0 ** -24
    for array in (tau, mu_tau):
        for idx in np.ndindex(array.shape):
            moved = array.copy()
            moved[idx] *= 1.0 + step
            args = (moved, mu_tau, mu, grad) if array is tau else (tau, moved, mu, grad)
            total += np.abs(ref.system_grads(windows, length, padding, *args)[1] - base)
    return total


@pytest.mark.parametrize('length', [1, 5, 6, 7])
@pytest.mark.parametrize('windows,padding', [('default', 0), ('default', 2), ('default', 3), ('5pt', 4)])
def test_reference_equals_central_differences_of_the_oracle(windows, padding, length):
    """L = sum(g * mlpg(means, variances)) on the float64 oracle; dL/dvar element by element from central differences with a relative
    step.  The reference forms 1 / var and mu / var in float32 as the kernel does, the oracle in float64: the bound is the central
    differences' own allowance plus the first-order effect of those roundings (``_input_sensitivity``)."""
    rng = np.random.RandomState(100 * length + padding)
    wins = ref.WINDOWS[windows]
    bsz, t, dim = 2, 7, 2
    width = len(wins) * dim
    seq_len = np.array([t, length])
    means = rng.standard_normal((bsz, t, width)).astype(np.float32)
    variances = (rng.uniform(0.2, 0.6, (bsz, t, width)) ** 2).astype(np.float32)
    grad_out = rng.standard_normal((bsz, t, dim))
    grad_out[1, length:] = 0.0
    means64, var64 = means.astype(np.float64), variances.astype(np.float64)

    def objective(v):
        return float((grad_out * ref_cpu.mlpg(means64, v, wins, padding_size=padding, seq_len=seq_len)).sum())

    want = np.zeros((bsz, t, width))
    for b in range(bsz):
        for f in range(int(seq_len[b])):
            for col in range(width):
                up, down = var64.copy(), var64.copy()
                h = FD_STEP * var64[b, f, col]
                up[b, f, col] += h
                down[b, f, col] -= h
                want[b, f, col] = (objective(up) - objective(down)) / (2 * h)
    got = ref.grads_ref(grad_out, means, variances, wins, padding, seq_len)
    tau, mu_tau, mu = ref.kernel_inputs(means, variances)
    limit = FD_ALLOWANCE * got['scale']
    for b in range(bsz):
        n = int(seq_len[b])
        for d in range(dim):
            cols = np.arange(len(wins)) * dim + d
            limit[b, :n, cols] += _input_sensitivity(wins, n, padding, tau[b, :n, cols], mu_tau[b, :n, cols], mu[b, :n, cols],
                                                     grad_out[b, :n, d])
    err = np.abs(got['grad_variances'] - want)
    valid = limit > 0
    print('windows %s padding %d length %d: max |difference| %.3e (max |want| %.3e), worst difference / bound %.3f' % (
        windows, padding, length, err.max(), np.abs(want).max(), (err[valid] / limit[valid]).max()))
    assert np.abs(want).max() > 0
    assert (err <= limit).all()
    assert not got['grad_variances'][1, length:].any() and not got['grad_means'][1, length:].any()
    # the trajectory the reference solves on the way is the oracle's (float32-formed inputs: 1e-6)
    base = ref_cpu.mlpg(means, variances, wins, padding_size=padding, seq_len=seq_len)
    assert np.abs(got['trajectory'] - base).max() <= 1e-6 * np.abs(base).max()


@pytest.mark.parametrize('name', sorted(ref.VAR_CASES))
def test_variance_gradient_is_scale_invariant(name):
    """The trajectory depends only on ratios of precisions: sum over (f, w) of var * dL/dvar = 0 for every system - up to the float32
    forming of tau (the reference differentiates through the rounded 1 / var: 2^-23 of the sum of |var dL/dvar|) and the floor."""
    _, _, variances, windows, _, _, want = ref.case(name)
    n_win = len(windows)
    bsz, t, width = variances.shape
    dim = width // n_win
    weighted = (variances.astype(np.float64) * want['grad_variances']).reshape(bsz, t, n_win, dim)
    total, absolute = weighted.sum(axis=(1, 2)), np.abs(weighted).sum(axis=(1, 2))
    floor = ref.SOLVE_FLOOR * (variances.astype(np.float64) * want['scale']).reshape(bsz, t, n_win, dim).sum(axis=(1, 2))
    limit = 2.0 ** -22 * absolute + floor
    print('%s: max |sum var dL/dvar| %.3e against sum |var dL/dvar| %.3e' % (name, np.abs(total).max(), absolute.max()))
    assert absolute.max() > 0
    assert (np.abs(total) <= limit).all()


@pytest.mark.parametrize('name', sorted(ref.VAR_CASES))
def test_gpu_cases_are_well_conditioned(name):
    """64 cond(P) 2^-52 < 1e-9 for every system of every GPU case: what makes the 1e-9 floor of the float64 comparison honest."""
    for masked in (True, False):
        _, means, variances, _, _, _, want = ref.case(name, masked)
        if name == 'wide_spread':
            lo, hi = np.exp(2 * ref.WIDE_LOG_STD[0]), np.exp(2 * ref.WIDE_LOG_STD[1])
            assert variances.max() / variances.min() > 30
        else:
            lo, hi = 0.04, 0.36
        assert lo * (1 - 1e-6) <= variances.min() and variances.max() <= hi * (1 + 1e-6)
        print('%s (%s): cond(P) <= %.1f' % (name, 'masked' if masked else 'seq_len=None', want['cond'].max()))
        assert ref.COND_FACTOR * want['cond'].max() < ref.SOLVE_FLOOR
        assert np.isfinite(want['grad_variances']).all() and np.abs(want['grad_variances']).max() > 0
        assert np.abs(want['grad_means']).max() > 0


def test_mg_mlpg_grad_mv_validates_its_arguments_without_a_gpu():
    lib = _lib.load()
    fake = 1 << 20                                        # never dereferenced: every call below returns before a launch
    win_l, win_u, win_c = ops._window_arrays(ref.DEFAULT_WINDOWS)

    def call(grad_out=fake, means=fake, variances=fake, b=2, t=5, d=3, n_win=3, l=win_l, u=win_u, c=win_c, padding=2, grad_means=fake,
             grad_variances=fake, ws=fake, ws_bytes=1 << 30):
        return lib.mg_mlpg_grad_mv_f32(grad_out, means, variances, None, b, t, d, n_win, l, u, c, padding, grad_means, grad_variances, 0,
                                       ws, ws_bytes, None)

    for null in ('grad_out', 'means', 'variances', 'grad_means', 'grad_variances', 'l', 'u', 'c'):
        assert call(**{null: None}) == -1 and 'mg_mlpg_grad_mv_f32: null argument' in _lib.last_error(), null
    for n_win in (0, 5):
        assert call(n_win=n_win) == -1 and 'windows supported, got %d' % n_win in _lib.last_error()
    wide_l, wide_u = (ctypes.c_int * 3)(0, 3, 1), (ctypes.c_int * 3)(0, 2, 1)       # l + u + 1 = 6 coefficients
    assert call(l=wide_l, u=wide_u) == -1 and 'window 1 (l=3, u=2) is wider than 5' in _lib.last_error()
    assert call(b=0) == -1 and 'bad shape (B=0' in _lib.last_error()
    assert call(t=0) == -1 and call(d=0) == -1 and call(padding=-1) == -1
    # two sets of the forward's planes; too small a workspace is MG_EWORKSPACE, before any launch
    forward = lib.mg_mlpg_workspace_bytes(2, 5, 3, 2, 3, win_l, win_u)
    need = lib.mg_mlpg_grad_mv_workspace_bytes(2, 5, 3, 2, 3, win_l, win_u)
    assert need == 2 * forward == 2 * (2 + 2) * (5 + 4) * 6 * 8
    assert lib.mg_mlpg_grad_mv_workspace_bytes(0, 5, 3, 2, 3, win_l, win_u) == 0
    assert lib.mg_mlpg_grad_mv_workspace_bytes(2, 5, 3, 2, 3, None, win_u) == 0
    assert call(ws_bytes=need - 1) == _lib.MG_EWORKSPACE and 'workspace of %d bytes needed' % need in _lib.last_error()
    assert call(ws_bytes=forward) == _lib.MG_EWORKSPACE
    assert call(ws=None) == _lib.MG_EWORKSPACE
    with pytest.raises(ValueError, match='mg_mlpg_grad_mv_f32'):
        _lib.check(call(b=0), 'mg_mlpg_grad_mv_f32')


def test_host_layers_refuse_what_they_cannot_do():
    g, mu = torch.zeros(2, 5, 1), torch.zeros(2, 5, 3)
    with pytest.raises(_lib.MorganaHipError, match='no CPU fallback'):
        ops.mlpg_backward_mv(g, mu, torch.ones(2, 5, 3), ref.DEFAULT_WINDOWS)
    for shape in ((3,), (2, 3)):
        with pytest.raises(ValueError, match=r'expand them to \(B, T, W\*D\)'):
            ops.mlpg_backward_mv(g, mu, torch.ones(shape), ref.DEFAULT_WINDOWS)
    with pytest.raises(ValueError, match='means'):
        ops.mlpg_backward_mv(g, torch.zeros(2, 5, 2), torch.ones(2, 5, 3), ref.DEFAULT_WINDOWS)
    # the keyword: False is the refusal of before, with a pointer to the new path; True wants per-frame variances
    with pytest.raises(ValueError, match='variance_grad=True'):
        synthesis.mlpg_trajectory(mu, torch.ones(2, 5, 3, requires_grad=True))
    with pytest.raises(ValueError, match='normaliser constants'):
        synthesis.mlpg_trajectory(mu, torch.ones(3, requires_grad=True), variance_grad=False)
    for shape in ((3,), (2, 3)):
        with pytest.raises(ValueError, match=r'expand them to\s+\(B, T, W\*D\)'):
            synthesis.mlpg_trajectory(mu, torch.ones(shape, requires_grad=True), variance_grad=True)
    with pytest.raises(TypeError, match='device tensors'):
        synthesis.mlpg_trajectory(mu, np.ones((2, 5, 3), np.float32), variance_grad=True)
    with pytest.raises(_lib.MorganaHipError, match='no CPU fallback'):
        synthesis.mlpg_trajectory(mu, torch.ones(2, 5, 3, requires_grad=True), variance_grad=True)


def test_gaussian_stream_table():
    st = models.Stream('lf0', 3, 'gaussian')
    assert st.width == 6 and st.is_delta and st.is_gaussian and not st.is_mdn
    assert st.output_key == 'normalised_lf0_deltas' and not st.differentiable_trajectory and st.min_log_std is None
    trained = models.Stream('lf0', 3, 'gaussian', min_log_std=-3., trajectory_weight=1., gv_weight=0.5, gv_log=False)
    assert trained.trains_trajectory and trained.trains_gv and trained.differentiable_trajectory and trained.min_log_std == -3.
    assert models.Stream('lf0', 3, 'gaussian', trajectory_loss=losses.mse).trajectory_loss is losses.mse
    with pytest.raises(ValueError, match="n_components belongs to an 'mdn' stream"):
        models.Stream('lf0', 3, 'gaussian', n_components=2)
    with pytest.raises(ValueError, match='negative'):
        models.Stream('lf0', 3, 'gaussian', trajectory_weight=-1.)
    # the refusals of the other kinds stand
    with pytest.raises(ValueError, match="belong to an 'mdn' stream: a 'mse' stream has no mixture"):
        models.Stream('lf0', 3, 'mse', min_log_std=-3.)
    with pytest.raises(ValueError, match="selected mean of an 'mdn' stream"):
        models.Stream('lf0', 3, 'mdn', n_components=2, trajectory_weight=1.)
    with pytest.raises(ValueError, match="selected mean of an 'mdn' stream"):
        models.Stream('lf0', 3, 'mdn', n_components=1, gv_weight=1.)
    layers = torch.nn.Linear(4, 6)
    with pytest.raises(ValueError, match='fused_loss=True cannot score the stream.* lf0 with a Gaussian likelihood'):
        models.StreamModel(layers, [st], fused_loss=True)
    assert models.StreamModel(layers, [st], fused_loss=False).streams[0] is st
    with pytest.raises(ValueError, match='per-frame variances have no differentiable trajectory'):
        model = models.StreamModel(layers, [st], fused_loss=False)
        model.normalisers = {'lf0': None}
        model._trajectory('lf0', torch.zeros(1, 2, 3), differentiable=True, norm_variance=torch.ones(1, 2, 3))


def test_gruf0_predict_variance():
    plain, off = models.GRUF0Model(), models.GRUF0Model(predict_variance=False)
    assert [(st.name, st.dim, st.loss, st.width) for st in plain.streams] == [(st.name, st.dim, st.loss, st.width) for st in off.streams]
    assert {k: tuple(v.shape) for k, v in plain.state_dict().items()} == {k: tuple(v.shape) for k, v in off.state_dict().items()}
    model = models.GRUF0Model(predict_variance=True, trajectory_weight=1., gv_weight=0.5, min_log_std=-4.)
    (st,) = model.streams
    assert st.loss == 'gaussian' and st.width == 6 and st.trajectory_weight == 1. and st.gv_weight == 0.5 and st.min_log_std == -4.
    assert tuple(model.layers[12].weight.shape) == (6, 64)
    assert list(model.state_dict()) == list(plain.state_dict())
    with pytest.raises(ValueError, match='predict_variance=True .* n_components=2'):
        models.GRUF0Model(predict_variance=True, n_components=2)
    # without delta parameters there is no trajectory to score, as for the other kinds
    model = models.GRUF0Model(generate=False, predict_variance=True, gv_weight=1.)
    model.mode = 'train'
    features = {'n_frames': torch.tensor([2]), 'normalised_lf0_deltas': torch.zeros(1, 2, 3)}
    with pytest.raises(RuntimeError, match="gv_weight=1.*normaliser 'lf0' has no delta parameters"):
        model.loss(features, {'lf0_gaussian': torch.zeros(1, 2, 6)})


@pytest.mark.parametrize('min_log_std', [None, -0.5])
def test_gaussian_nll_is_the_mdn_of_one_component(min_log_std):
    """losses.gaussian's per-element term in float64 on the CPU, averaged as losses.mse averages, against tests/mdn_ref64.py at K = 1
    with a zero logit (log_softmax of one logit is 0): values and gradients to float64 rounding."""
    rng = np.random.RandomState(3)
    bsz, t, dim = 3, 11, 4
    seq_len = np.array([11, 6, 1])
    target = rng.standard_normal((bsz, t, dim))
    mean = target + 0.7 * rng.standard_normal((bsz, t, dim))
    log_std = -0.5 + 0.8 * rng.standard_normal((bsz, t, dim))
    pred = torch.tensor(np.concatenate([mean, log_std], axis=2), dtype=torch.float64, requires_grad=True)
    term = losses.gaussian_nll(pred, torch.tensor(target), min_log_std=min_log_std)
    assert term.dtype == torch.float64 and tuple(term.shape) == (bsz, t, dim)
    mask = torch.tensor(np.arange(t)[None, :] < seq_len[:, None])[..., None]
    loss = ((term * mask).sum(dim=1) / torch.tensor(seq_len, dtype=torch.float64)[:, None]).mean()
    loss.backward()
    as_mdn = np.concatenate([np.zeros((bsz, t, 1)), mean, log_std], axis=2)
    want = mdn_ref64.mdn(as_mdn, target, seq_len, n_components=1, min_log_std=min_log_std)
    print('loss %.12f, mdn_ref64 %.12f' % (loss.item(), want['loss']))
    assert abs(loss.item() - want['loss']) <= 1e-12 * abs(want['loss'])
    got_grad = pred.grad.numpy() * mask.numpy()
    assert np.abs(got_grad - want['grad'][:, :, 1:]).max() <= 1e-12 * np.abs(want['grad']).max()
    if min_log_std is not None:
        assert (log_std < min_log_std).any() and not got_grad[:, :, dim:][log_std < min_log_std].any()
    with pytest.raises(ValueError, match='2 D'):
        losses.gaussian_nll(torch.zeros(1, 2, 5), torch.zeros(1, 2, 3))
    with pytest.raises(ValueError, match='2 D'):
        losses.gaussian(torch.zeros(1, 2, 5), torch.zeros(1, 2, 3))
    with pytest.raises(_lib.MorganaHipError, match='no CPU fallback'):
        losses.gaussian(torch.zeros(1, 2, 6), torch.zeros(1, 2, 3))
