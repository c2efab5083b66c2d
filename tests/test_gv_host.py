"""losses.gv without a GPU: the long-double restatement (tests/gv_ref64.py) against torch float64 autograd and central differences,
the honesty of its derived bounds on the inputs the GPU test uses, the offset column that tells a sum of raw squares from the
two-pass variance, the host-side argument validation of the C entry points, and the refusals of models.Stream and the models."""
import ctypes

import numpy as np
import pytest
import torch

import gv_ref64
from morgana_amd import _lib, losses, models


def _chunk():
    return _lib.load().mg_gv_chunk_frames()


def _torch_gv(pred, tgt, seq_len, log, eps):
    """The definition composed of torch float64 ops: var(unbiased=False) per utterance, autograd for the gradient."""
    x = torch.tensor(np.asarray(pred, np.float64), requires_grad=True)
    y = torch.tensor(np.asarray(tgt, np.float64))
    b, t, d = x.shape
    n = gv_ref64.valid_frames(seq_len, b, t)
    total = 0.
    for i in range(b):
        vp, vt = x[i, :n[i]].var(dim=0, unbiased=False), y[i, :n[i]].var(dim=0, unbiased=False)
        delta = torch.log(vp + eps) - torch.log(vt + eps) if log else vp - vt
        total = total + (delta ** 2).sum()
    loss = total / (b * d)
    loss.backward()
    return loss.item(), x.grad.numpy()


# ------------------------------------------------------------------------------------------------- the restatement against autograd
@pytest.mark.parametrize('log', [True, False])
def test_restatement_equals_torch_float64_autograd(log):
    rng = np.random.RandomState(3)
    pred, tgt = rng.standard_normal((3, 7, 2)).astype(np.float32), rng.standard_normal((3, 7, 2)).astype(np.float32)
    for seq_len in ([7, 4, 2], None):
        ref = gv_ref64.gv(pred, tgt, seq_len, log=log, grad_scale=1.0)
        want_loss, want_grad = _torch_gv(pred, tgt, seq_len, log, 1e-6)
        print('log=%s seq_len=%s: loss %.3e, gradient %.3e apart' % (log, seq_len, abs(ref['loss'] - want_loss),
                                                                    np.abs(ref['grad'] - want_grad).max()))
        assert abs(ref['loss'] - want_loss) <= 1e-12 * max(1.0, abs(want_loss))
        assert np.abs(ref['grad'] - want_grad).max() <= 1e-12 * max(1.0, np.abs(want_grad).max())
        assert np.all(ref['grad'][~ref['mask']] == 0.0)
    scaled = gv_ref64.gv(pred, tgt, [7, 4, 2], log=log, grad_scale=-0.5)
    assert np.allclose(scaled['grad'], -0.5 * gv_ref64.gv(pred, tgt, [7, 4, 2], log=log)['grad'], rtol=1e-15, atol=0)


@pytest.mark.parametrize('log', [True, False])
def test_restatement_gradient_equals_central_differences(log):
    rng = np.random.RandomState(4)
    pred, tgt = rng.standard_normal((2, 6, 3)).astype(np.float32), rng.standard_normal((2, 6, 3)).astype(np.float32)
    seq_len = [6, 4]
    grad = gv_ref64.gv(pred, tgt, seq_len, log=log)['grad']
    h = 2.0 ** -7                                                # exact in float32 next to values of order 1
    for b, t, d in ((0, 0, 0), (0, 5, 2), (1, 3, 1), (1, 5, 0)):
        up, down = pred.copy(), pred.copy()
        up[b, t, d] += h
        down[b, t, d] -= h
        step = float(up[b, t, d]) - float(down[b, t, d])
        fd = (gv_ref64.gv(up, tgt, seq_len, log=log)['loss'] - gv_ref64.gv(down, tgt, seq_len, log=log)['loss']) / step
        assert abs(fd - grad[b, t, d]) <= 2e-3 * max(np.abs(grad).max(), 1e-3), (b, t, d, fd, grad[b, t, d])
    assert grad[1, 5, 0] == 0.0                                  # a pad frame


def test_restatement_semantics():
    rng = np.random.RandomState(1)
    pred, tgt = rng.standard_normal((3, 7, 5)).astype(np.float32), rng.standard_normal((3, 7, 5)).astype(np.float32)
    full = gv_ref64.gv(pred, tgt)
    assert full['loss'] == gv_ref64.gv(pred, tgt, [7, 7, 7])['loss'] == gv_ref64.gv(pred, tgt, [9, 7, 100])['loss']
    empty = gv_ref64.gv(pred, tgt, [7, 0, 2])
    assert np.isnan(empty['loss']) and np.isnan(empty['grad'][1]).all() and np.isfinite(empty['grad'][[0, 2]]).all()
    one = gv_ref64.gv(pred, tgt, [7, 1, 2])
    assert np.isfinite(one['loss']) and np.all(one['grad'][1] == 0.0) and np.all(one['v_pred'][1] == 0.0)
    poisoned = pred.copy()
    poisoned[1, 5, 2] = np.nan                                   # a pad frame of utterance 1: never read
    a, b = gv_ref64.gv(pred, tgt, [7, 4, 2]), gv_ref64.gv(poisoned, tgt, [7, 4, 2])
    assert a['loss'] == b['loss'] and np.array_equal(a['grad'], b['grad'])
    constant = pred.copy()
    constant[:, :, 3] = 2.5
    v, bound = gv_ref64.variance_bound(constant, [7, 4, 2])
    assert np.all(v[:, 3] == 0.0) and np.all(bound[:, 3] == 0.0)


# ----------------------------------------------------------------------------------------------------------- the bounds are honest
@pytest.mark.parametrize('log', [True, False])
@pytest.mark.parametrize('kind', gv_ref64.SEQ_LENS)
@pytest.mark.parametrize('d', [1, 5, 60, 67])
def test_another_summation_order_lies_inside_the_bounds(d, kind, log):
    """The two-pass definition on the GPU test's float32 inputs, accumulated in float64 in another order and rounded to float32 once as
    the kernel rounds (gv_ref64.other_order), is inside the derived bounds: they leave room for a correct evaluation.  (An evaluation
    whose arithmetic is float32 throughout is NOT inside them and is not meant to be: the bounds allow one float32 rounding.)"""
    chunk = _chunk()
    pred, tgt = gv_ref64.case(chunk, d)
    seq_len = gv_ref64.seq_len_case(kind, chunk)
    ref = gv_ref64.gv(pred, tgt, seq_len, log=log, grad_scale=0.75)
    loss, grad = gv_ref64.other_order(pred, tgt, seq_len, log=log, grad_scale=0.75)
    gv_ref64.report('D=%d seq_len=%s log=%s' % (d, kind, log), ref, loss, grad)
    assert np.isfinite(ref['loss']) and ref['loss'] > 0 and np.abs(ref['grad']).max() > 0
    assert ref['loss_float64'] <= 1e-2 * ref['loss_rounding']                 # the float64 term is a correction, not the bound
    assert abs(float(loss) - ref['loss']) <= ref['loss_bound']
    assert np.all(np.abs(grad.astype(np.float64) - ref['grad']) <= ref['grad_bound'])
    assert np.all(grad[~ref['mask']] == 0.0)


def test_offset_column_tells_raw_squares_from_two_pass():
    """Column 0 of the offset case sits at 16384 with standard deviation 2^-6.  E[x^2] - E[x]^2 in float64 misses the loss bound
    there, by orders of magnitude, while the two-pass evaluation in another order is inside it: the GPU test on this input cannot
    be passed by a kernel that sums raw squares."""
    chunk = _chunk()
    pred, tgt = gv_ref64.offset_case(chunk)
    assert abs(pred[:, :, 0].mean() - 16384) < 1 and 0.5 * 2.0 ** -6 < tgt[:, :, 0].std() < 2.0 ** -5
    for log in (True, False):
        ref = gv_ref64.gv(pred, tgt, log=log)
        loss, grad = gv_ref64.other_order(pred, tgt, log=log)
        raw = gv_ref64.raw_squares_loss(pred, tgt, log=log)
        gv_ref64.report('offset log=%s' % log, ref, loss, grad)
        print('   sum of raw squares in float64: loss off by %.3e = %.1f x the bound' % (abs(raw - ref['loss']),
                                                                                       abs(raw - ref['loss']) / ref['loss_bound']))
        assert abs(float(loss) - ref['loss']) <= ref['loss_bound']
        assert np.all(np.abs(grad.astype(np.float64) - ref['grad']) <= ref['grad_bound'])
        if log:
            assert abs(raw - ref['loss']) > 100 * ref['loss_bound']
    # per column, the variance itself: the raw-squares value of column 0 is off by far more than its bound
    v, bound = gv_ref64.variance_bound(tgt)
    seg = tgt.astype(np.float64)
    raw_v = (seg ** 2).mean(axis=1) - seg.mean(axis=1) ** 2
    assert np.all(np.abs(raw_v[:, 0] - v[:, 0]) > 100 * bound[:, 0])
    assert np.all(np.abs(raw_v[:, 2:] - v[:, 2:]) <= bound[:, 2:])


# ------------------------------------------------------------------------------------------------------------------ the C entry points
def test_gv_entry_points_validate_their_arguments_without_a_gpu():
    lib = _lib.load()
    chunk = lib.mg_gv_chunk_frames()
    assert chunk > 0
    assert lib.mg_gv_workspace_bytes(3, 7, 5) >= 2 * 3 * 2 * 5 * 8
    assert lib.mg_gv_workspace_bytes(3, chunk + 1, 5) > lib.mg_gv_workspace_bytes(3, chunk, 5) >= 2 * 3 * 2 * 5 * 8
    assert lib.mg_gv_workspace_bytes(0, 7, 5) == 0 and lib.mg_gv_workspace_bytes(3, 7, -1) == 0 and lib.mg_gv_workspace_bytes(3, 0, 5) == 0
    assert lib.mg_gv_workspace_bytes(3, 7, _lib.MG_GV_MAX_D + 1) == 0
    p, y, loss, state, ws = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20       # never dereferenced: every call below is refused on the host
    names = ('pred', 'psb', 'pst', 'psd', 'tgt', 'tsb', 'tst', 'tsd', 'seq_len', 'B', 'T', 'D', 'log', 'eps', 'loss', 'state', 'v_pred',
             'v_tgt', 'workspace', 'workspace_bytes', 'stream')
    ok = (p, 35, 5, 1, y, 35, 5, 1, None, 3, 7, 5, 1, 1e-6, loss, state, None, None, ws, 1 << 12, None)

    def fwd(**changed):
        args = dict(zip(names, ok))
        args.update(changed)
        return lib.mg_gv_f32(*[args[n] for n in names])

    assert fwd(pred=None) == _lib.MG_EINVAL and 'mg_gv_f32' in _lib.last_error() and 'NULL' in _lib.last_error()
    assert fwd(loss=None) == _lib.MG_EINVAL and 'NULL' in _lib.last_error()
    assert fwd(state=None) == _lib.MG_EINVAL
    assert fwd(tgt=None, loss=None, state=None) == _lib.MG_EINVAL and 'v_pred' in _lib.last_error()
    for dim in ('B', 'T', 'D'):
        assert fwd(**{dim: 0}) == _lib.MG_EINVAL and '%s=0' % dim in _lib.last_error()
        assert fwd(**{dim: -2}) == _lib.MG_EINVAL
    assert fwd(B=65536) == _lib.MG_EINVAL and '65535' in _lib.last_error()
    assert fwd(D=_lib.MG_GV_MAX_D + 1) == _lib.MG_EINVAL and 'MG_GV_MAX_D' in _lib.last_error()
    for stride in ('psb', 'pst', 'psd', 'tsb', 'tst', 'tsd'):
        assert fwd(**{stride: -1}) == _lib.MG_EINVAL and 'stride' in _lib.last_error()
    assert fwd(eps=-1e-6) == _lib.MG_EINVAL and 'eps' in _lib.last_error()
    assert fwd(pred=p + 2) == _lib.MG_EINVAL and 'aligned' in _lib.last_error()
    assert fwd(tgt=y + 1) == _lib.MG_EINVAL and fwd(state=state + 4) == _lib.MG_EINVAL and fwd(workspace=ws + 4) == _lib.MG_EINVAL
    assert fwd(workspace=None) == _lib.MG_EWORKSPACE and 'workspace' in _lib.last_error()
    assert fwd(workspace_bytes=16) == _lib.MG_EWORKSPACE and 'got 16' in _lib.last_error()
    with pytest.raises(_lib.MorganaHipError):
        _lib.check(fwd(workspace_bytes=0), 'mg_gv_f32')
    with pytest.raises(ValueError):
        _lib.check(fwd(T=0), 'mg_gv_f32')

    g, grad = 6 << 20, 7 << 20
    bnames = ('grad_loss', 'state', 'pred', 'psb', 'pst', 'psd', 'seq_len', 'B', 'T', 'D', 'grad', 'stream')
    bok = (g, state, p, 35, 5, 1, None, 3, 7, 5, grad, None)

    def bwd(**changed):
        args = dict(zip(bnames, bok))
        args.update(changed)
        return lib.mg_gv_bwd_f32(*[args[n] for n in bnames])

    for name in ('grad_loss', 'state', 'pred', 'grad'):
        assert bwd(**{name: None}) == _lib.MG_EINVAL and 'mg_gv_bwd_f32' in _lib.last_error() and 'NULL' in _lib.last_error()
    for shape in ((0, 7, 5), (3, 0, 5), (3, 7, 0), (-1, 7, 5)):
        assert bwd(**dict(zip('BTD', shape))) == _lib.MG_EINVAL and 'bad shape' in _lib.last_error()
    assert bwd(B=65536) == _lib.MG_EINVAL and '65535' in _lib.last_error()
    assert bwd(pst=-5) == _lib.MG_EINVAL and 'stride' in _lib.last_error()
    assert bwd(grad=grad + 1) == _lib.MG_EINVAL and 'aligned' in _lib.last_error()
    assert bwd(state=state + 4) == _lib.MG_EINVAL
    assert _lib.SIGNATURES['mg_gv_f32'][1][1:4] == [ctypes.c_int64] * 3 == _lib.SIGNATURES['mg_gv_f32'][1][5:8]
    assert _lib.SIGNATURES['mg_gv_f32'][1][12:14] == [ctypes.c_int, ctypes.c_double]
    assert _lib.SIGNATURES['mg_gv_chunk_frames'] == (ctypes.c_int, [])


def test_gv_has_no_cpu_fallback_and_checks_its_operands():
    x, y = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4)
    with pytest.raises(_lib.MorganaHipError, match='no CPU fallback'):
        losses.gv(x, y)
    with pytest.raises(_lib.MorganaHipError, match='no CPU fallback'):
        losses.gv(x, y, torch.tensor([3, 2], dtype=torch.int32), log=False)
    with pytest.raises(_lib.MorganaHipError, match='no CPU fallback'):
        losses.global_variance(x)
    with pytest.raises(ValueError, match=r'\(2, 3, 5\)'):
        losses.gv(x, torch.zeros(2, 3, 5))
    with pytest.raises(ValueError, match=r'\(2, 3\)'):
        losses.gv(torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(ValueError):
        losses.global_variance(torch.zeros(2, 3))


# ------------------------------------------------------------------------------------------------------- Stream(gv_weight=...) and models
def _table(model):
    return [(st.name, st.dim, st.loss, st.metric, st.voicing, st.is_delta, st.output_key) for st in model.streams]


def test_stream_validation():
    with pytest.raises(ValueError, match="'ce' stream has no MLPG trajectory"):
        models.Stream('phone', 40, 'ce', gv_weight=0.5)
    with pytest.raises(ValueError, match="'sigmoid_bce' stream has no MLPG trajectory"):
        models.Stream('vuv', 1, 'sigmoid_bce', gv_weight=0.5)
    with pytest.raises(ValueError, match="global-variance loss.*'mdn' stream is not a differentiable"):
        models.Stream('lf0', 3, 'mdn', n_components=2, gv_weight=0.5)
    with pytest.raises(ValueError, match='gv_weight must not be negative'):
        models.Stream('lf0', 3, 'mse', gv_weight=-1.)
    varied = models.Stream('lf0', 3, 'mse', gv_weight=0.5, gv_log=False)
    assert varied.gv_weight == 0.5 and varied.gv_log is False and varied.trains_gv and not varied.trains_trajectory
    assert varied.differentiable_trajectory and varied.trajectory_weight == 0.
    plain = models.Stream('lf0', 3)
    assert plain.gv_weight == 0. and plain.gv_log is True and not plain.trains_gv and not plain.differentiable_trajectory
    both = models.Stream('lf0', 3, trajectory_weight=1., gv_weight=0.25)
    assert both.trains_gv and both.trains_trajectory
    layers = torch.nn.Linear(4, 3)
    with pytest.raises(ValueError, match='fused_loss=True cannot score the stream.* lf0 with a global-variance loss'):
        models.StreamModel(layers, [varied], fused_loss=True)
    assert models.StreamModel(layers, [varied], fused_loss=False).streams[0] is varied
    with pytest.raises(ValueError, match='fused_loss=True'):
        models.LSTMAcousticModel(num_layers=1, hidden_dim=8, post_dim=8, gv_weight=1.)
    with pytest.raises(ValueError, match='mdn'):
        models.GRUF0Model(n_components=4, gv_weight=1.)
    # weight 0 builds the table of today
    for cls, kwargs in ((models.GRUF0Model, {}), (models.VAEF0Model, {}), (models.LSTMAcousticModel, dict(num_layers=1, hidden_dim=8, post_dim=8))):
        without, zero = cls(**kwargs), cls(gv_weight=0., **kwargs)
        assert _table(without) == _table(zero)
        assert all(st.gv_weight == 0. and not st.trains_gv for st in zero.streams)
        assert [k for k in without.state_dict()] == [k for k in zero.state_dict()]
    acoustic = models.LSTMAcousticModel(num_layers=1, hidden_dim=8, post_dim=8, fused_loss=False, gv_weight=2.)
    assert [(st.name, st.gv_weight) for st in acoustic.streams] == [('lf0', 2.), ('vuv', 0.), ('mcep', 2.), ('bap', 2.)]
    assert [st.gv_weight for st in models.VAEF0Model(gv_weight=0.5).streams] == [0.5]


def test_a_gv_weight_without_delta_parameters_names_the_normaliser():
    model = models.GRUF0Model(generate=False, gv_weight=1.)
    features = {'n_frames': torch.tensor([2]), 'normalised_lf0_deltas': torch.zeros(1, 2, 3)}
    outputs = {'normalised_lf0_deltas': torch.zeros(1, 2, 3)}
    model.mode = 'train'
    with pytest.raises(RuntimeError, match="gv_weight=1.*normaliser 'lf0' has no delta parameters"):
        model.loss(features, outputs)
