"""The gradient of MLPG without a GPU: the dense float64 reference of tests/mlpg_grad_ref64.py against finite differences of the
oracle's MLPG, the conditioning of the cases the GPU tests run, the argument checks of mg_mlpg_grad_f32 (the library loads without a
device) and the validation of trajectory losses in the stream table."""
import ctypes

import numpy as np
import pytest
import torch

import mlpg_grad_ref64 as ref
from morgana_amd import _lib, models, ops
from morgana_amd.viz import synthesis
from oracle import ref_cpu


def test_the_reference_windows_are_the_package_defaults():
    for (l, u, c), (rl, ru, rc) in zip(synthesis.DEFAULT_WINDOWS, ref.DEFAULT_WINDOWS):
        assert (l, u, tuple(c)) == (rl, ru, rc)


@pytest.mark.parametrize('length', [1, 2, 9])
@pytest.mark.parametrize('windows,padding', [('default', 0), ('default', 7), ('5pt', 4)])
def test_reference_equals_finite_differences_of_the_oracle(windows, padding, length):
    """g^T (dx / dmu) with dx / dmu column by column from unit steps of oracle.ref_cpu.mlpg on float64 inputs: exact up to rounding,
    x being linear in mu.  The variances are powers of two inside [0.2^2, 0.6^2], so that the float32 reciprocal the reference (and
    the kernel) forms is the float64 one the oracle forms; two utterances, the second cut to ``length``, per-frame variances."""
    rng = np.random.RandomState(10 * length + padding)
    wins = ref.WINDOWS[windows]
    bsz, t, dim = 2, 9, 2
    width = len(wins) * dim
    seq_len = np.array([t, length])
    means = rng.standard_normal((bsz, t, width))
    variances = rng.choice([0.0625, 0.125, 0.25], size=(bsz, t, width))
    grad_out = rng.standard_normal((bsz, t, dim))
    grad_out[1, length:] = 0.0
    base = ref_cpu.mlpg(means, variances, wins, padding_size=padding, seq_len=seq_len)
    want = np.zeros((bsz, t, width))
    for b in range(bsz):
        for f in range(int(seq_len[b])):
            for col in range(width):
                stepped = means.copy()
                stepped[b, f, col] += 1.0
                column = ref_cpu.mlpg(stepped, variances, wins, padding_size=padding, seq_len=seq_len) - base
                want[b, f, col] = float((grad_out * column).sum())
    got, cond = ref.grad_means_ref(grad_out, variances.astype(np.float32), wins, padding, seq_len)
    err = np.abs(got - want).max() / np.abs(want).max()
    print('windows %s padding %d length %d: relative difference %.3e, cond(P) <= %.1f' % (windows, padding, length, err, cond.max()))
    assert err < 1e-10
    assert not got[1, length:].any()


@pytest.mark.parametrize('layout', ref.VAR_LAYOUTS)
@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_gpu_cases_are_well_conditioned(name, layout):
    """64 cond(P) 2^-52 < 1e-9 for every system of every GPU case: what makes the 1e-9 floor of the float64 comparison honest."""
    for masked in ((True, False) if name == 'no_padding' else (True,)):
        grad_out, variances, windows, padding, seq_len, want, cond = ref.case(name, layout, masked)
        assert 0.04 - 1e-7 <= variances.min() and variances.max() <= 0.36 + 1e-7
        print('%s / %s: cond(P) <= %.1f' % (name, layout, cond.max()))
        assert ref.COND_FACTOR * cond.max() < ref.SOLVE_FLOOR
        assert np.isfinite(want).all() and np.abs(want).max() > 0


def test_mg_mlpg_grad_validates_its_arguments_without_a_gpu():
    lib = _lib.load()
    fake = 1 << 20                                        # never dereferenced: every call below returns before a launch
    win_l, win_u, win_c = ops._window_arrays(ref.DEFAULT_WINDOWS)

    def call(grad_out=fake, variances=fake, b=2, t=5, d=3, n_win=3, l=win_l, u=win_u, c=win_c, padding=2, grad_means=fake, ws=fake,
             ws_bytes=1 << 30):
        return lib.mg_mlpg_grad_f32(grad_out, variances, 0, None, b, t, d, n_win, l, u, c, padding, grad_means, 0, ws, ws_bytes, None)

    for null in ('grad_out', 'variances', 'grad_means', 'l', 'u', 'c'):
        assert call(**{null: None}) == -1 and 'mg_mlpg_grad_f32: null argument' in _lib.last_error(), null
    for n_win in (0, 5):
        assert call(n_win=n_win) == -1 and 'windows supported, got %d' % n_win in _lib.last_error()
    wide_l, wide_u = (ctypes.c_int * 3)(0, 3, 1), (ctypes.c_int * 3)(0, 2, 1)       # l + u + 1 = 6 coefficients
    assert call(l=wide_l, u=wide_u) == -1 and 'window 1 (l=3, u=2) is wider than 5' in _lib.last_error()
    assert call(b=0) == -1 and 'bad shape (B=0' in _lib.last_error()
    assert call(t=0) == -1 and call(d=0) == -1 and call(padding=-1) == -1
    # the forward's workspace is the backward's: too small a one is MG_EWORKSPACE, before any launch
    need = lib.mg_mlpg_workspace_bytes(2, 5, 3, 2, 3, win_l, win_u)
    assert need == (2 + 2) * (5 + 4) * 6 * 8
    assert call(ws_bytes=need - 1) == _lib.MG_EWORKSPACE and 'workspace of %d bytes needed' % need in _lib.last_error()
    assert call(ws=None) == _lib.MG_EWORKSPACE
    with pytest.raises(ValueError, match='mg_mlpg_grad_f32'):
        _lib.check(call(b=0), 'mg_mlpg_grad_f32')


def test_host_layers_refuse_what_they_cannot_do():
    with pytest.raises(_lib.MorganaHipError, match='no CPU fallback'):
        ops.mlpg_backward(torch.zeros(2, 5, 1), torch.ones(3), ref.DEFAULT_WINDOWS)
    with pytest.raises(TypeError, match='device tensors'):
        synthesis.mlpg_trajectory(np.zeros((2, 5, 3), np.float32), torch.ones(3))
    with pytest.raises(ValueError, match='variances'):
        synthesis.mlpg_trajectory(torch.zeros(2, 5, 3), torch.ones(3, requires_grad=True))


def _table(model):
    return [(st.name, st.dim, st.loss, st.metric, st.voicing, st.is_delta, st.output_key) for st in model.streams]


def test_stream_validation():
    with pytest.raises(ValueError, match="'ce' stream has no MLPG trajectory"):
        models.Stream('phone', 40, 'ce', trajectory_weight=0.5)
    with pytest.raises(ValueError, match="'sigmoid_bce' stream has no MLPG trajectory"):
        models.Stream('vuv', 1, 'sigmoid_bce', trajectory_weight=0.5)
    with pytest.raises(ValueError, match='negative'):
        models.Stream('lf0', 3, 'mse', trajectory_weight=-1.)
    weighted = models.Stream('lf0', 3, 'mse', trajectory_weight=0.5)
    assert weighted.trajectory_weight == 0.5 and weighted.trajectory_loss is None and weighted.is_delta
    plain = models.Stream('lf0', 3)
    assert plain.trajectory_weight == 0. and plain.trajectory_loss is None
    layers = torch.nn.Linear(4, 3)
    with pytest.raises(ValueError, match='fused_loss=True cannot score the stream.* lf0 with a trajectory loss'):
        models.StreamModel(layers, [weighted], fused_loss=True)
    assert models.StreamModel(layers, [weighted], fused_loss=False).streams[0] is weighted
    with pytest.raises(ValueError, match='fused_loss=True'):
        models.LSTMAcousticModel(num_layers=1, hidden_dim=8, post_dim=8, trajectory_weight=1.)
    # weight 0 builds the table of today
    for cls, kwargs in ((models.GRUF0Model, {}), (models.VAEF0Model, {}), (models.LSTMAcousticModel, dict(num_layers=1, hidden_dim=8, post_dim=8))):
        without, zero = cls(**kwargs), cls(trajectory_weight=0., **kwargs)
        assert _table(without) == _table(zero)
        assert all(st.trajectory_weight == 0. and not st.trains_trajectory for st in zero.streams)
        assert [k for k in without.state_dict()] == [k for k in zero.state_dict()]
    acoustic = models.LSTMAcousticModel(num_layers=1, hidden_dim=8, post_dim=8, fused_loss=False, trajectory_weight=2.)
    assert [(st.name, st.trajectory_weight) for st in acoustic.streams] == [('lf0', 2.), ('vuv', 0.), ('mcep', 2.), ('bap', 2.)]


def test_a_trajectory_weight_without_delta_parameters_names_the_normaliser():
    """``generate=False`` (or normalisers without delta parameters): there is no trajectory, and ``loss`` says which normaliser lacks
    what, at the first call."""
    model = models.GRUF0Model(generate=False, trajectory_weight=1.)
    features = {'n_frames': torch.tensor([2]), 'normalised_lf0_deltas': torch.zeros(1, 2, 3)}
    outputs = {'normalised_lf0_deltas': torch.zeros(1, 2, 3)}
    model.mode = 'train'
    with pytest.raises(RuntimeError, match="trajectory_weight=1.*normaliser 'lf0' has no delta parameters"):
        model.loss(features, outputs)
