"""losses.sequence_loss without a GPU: the float64 restatement (tests/seqloss_ref64.py) against the reference's recorded numbers
inside the derived bounds, the wrapper's contract and checks, the host-side argument validation of the C entry points, and the
callable loss of models.Stream."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
import torch.nn as nn

import seqloss_ref64
from morgana_amd import _lib, losses, models, utils


# ------------------------------------------------------------------------------------- the restatement against the reference's numbers
def test_golden_file_holds_the_cases(golden):
    g = golden(seqloss_ref64.GOLDEN)
    assert tuple(g['cases']) == seqloss_ref64.GOLDEN_CASES
    assert 'l1_full__seq_len' not in g and all(name + '__seq_len' in g for name in seqloss_ref64.GOLDEN_CASES if name != 'l1_full')
    assert g['nll__pred'].shape == (3, 7, 10) and g['nll__feature_loss'].shape == (3, 7, 5)
    assert g['l1_long__feature_loss'].shape == (2, 70, 33) and g['l1_d1__feature_loss'].shape == (3, 7, 1)
    assert np.array_equal(g['l1_full__pred'], g['l1_ragged__pred']) and np.array_equal(g['l1_full__target'], g['l1_ragged__target'])


@pytest.mark.parametrize('name', seqloss_ref64.GOLDEN_CASES)
def test_restatement_against_the_golden_cases(golden, name):
    _, _, seq_len, feature_loss, loss, grad_feature, _ = seqloss_ref64.golden_case(golden(seqloss_ref64.GOLDEN), name)
    ref = seqloss_ref64.seq_mean(feature_loss, seq_len)
    loss_err = abs(loss - ref['loss'])
    grad_err = np.abs(grad_feature.astype(np.float64) - ref['grad'])
    print('%s: loss err %.3e (bound %.3e), worst gradient err %.3f of 2^-24 |g|'
          % (name, loss_err, ref['golden_loss_bound'], float((grad_err / np.maximum(np.abs(ref['grad']), 1e-300)).max() / seqloss_ref64.U)))
    assert loss_err <= ref['golden_loss_bound']
    assert np.all(grad_err <= ref['golden_grad_bound'])
    assert np.all(grad_feature[~ref['mask']] == 0.0)


def test_restatement_semantics():
    rng = np.random.RandomState(1)
    x = rng.standard_normal((3, 7, 5)).astype(np.float32)
    full = seqloss_ref64.seq_mean(x, None)
    assert full['loss'] == seqloss_ref64.seq_mean(x, [7, 7, 7])['loss'] == seqloss_ref64.seq_mean(x, [9, 7, 100])['loss']
    assert abs(full['loss'] - x.astype(np.float64).mean()) <= 1e-15
    empty = seqloss_ref64.seq_mean(x, [7, 0, 1])
    assert np.isnan(empty['loss']) and np.isnan(empty['grad'][1]).all() and np.isfinite(empty['grad'][[0, 2]]).all()
    assert np.isnan(seqloss_ref64.seq_mean(x, [7, -3, 1])['loss'])
    poisoned = x.copy()
    poisoned[1, 5, 2] = np.nan                                   # a pad frame of utterance 1
    assert np.isnan(seqloss_ref64.seq_mean(poisoned, [7, 4, 1])['loss'])
    ragged = seqloss_ref64.seq_mean(x, [7, 4, 1], grad_scale=0.5)
    assert ragged['grad'][1, 3, 0] == 0.5 / (4 * 3 * 5) and ragged['grad'][1, 4, 0] == 0.0 and ragged['grad'][2, 0, 4] == 0.5 / 15


# ------------------------------------------------------------------------------------------------------------- the wrapper's contract
def test_sequence_loss_keeps_name_doc_and_signature():
    @losses.sequence_loss
    def l1(predictions, targets):
        """Absolute error of every frame and feature."""
        return torch.abs(predictions - targets)

    assert l1.__name__ == 'l1' and l1.__doc__ == 'Absolute error of every frame and feature.'
    assert l1.__wrapped__.__name__ == 'l1'
    spec = inspect.getfullargspec(l1)
    assert spec.args == ['predictions', 'targets', 'seq_len'] and spec.defaults == (None,)
    assert spec.varargs is None and spec.varkw is None and not spec.kwonlyargs


def test_sequence_loss_checks_the_feature_loss():
    x, y = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4)
    with pytest.raises(ValueError, match=r'\(2, 3\)'):                       # the rank that was given is named
        losses.sequence_loss(lambda p, t: (p - t).sum(dim=-1))(x, y)
    with pytest.raises(ValueError, match=r'\(2, 3, 4, 1\)'):
        losses.sequence_loss(lambda p, t: (p - t).unsqueeze(-1))(x, y)
    with pytest.raises(TypeError, match='float64'):
        losses.sequence_loss(lambda p, t: (p - t).double())(x, y)
    with pytest.raises(TypeError, match='float16'):
        losses.sequence_loss(lambda p, t: (p - t).half())(x, y)
    with pytest.raises(TypeError, match='float'):
        losses.sequence_loss(lambda p, t: 1.0)(x, y)
    plain = losses.sequence_loss(lambda p, t: p - t)
    with pytest.raises(ValueError, match=r'\(3,\)'):
        plain(x, y, torch.tensor([3, 2, 1]))
    with pytest.raises(ValueError, match=r'\(2, 1\)'):
        plain(x, y, torch.tensor([[3], [2]]))
    with pytest.raises(TypeError, match='float32'):
        plain(x, y, torch.tensor([3.0, 2.0]))


def test_sequence_loss_has_no_cpu_fallback():
    x, y = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4)
    plain = losses.sequence_loss(lambda p, t: p - t)
    with pytest.raises(_lib.MorganaHipError, match='no CPU fallback'):
        plain(x, y)
    with pytest.raises(_lib.MorganaHipError, match='no CPU fallback'):
        plain(x, y, torch.tensor([3, 2], dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------------ the C entry points
def test_seq_mean_entry_points_validate_their_arguments_without_a_gpu():
    """mg_seq_mean_f32 / mg_seq_mean_bwd_f32: the host side refuses null pointers, shapes that are not positive and a workspace that
    is too small before any launch (the library's codes and a message), as every other entry point does."""
    lib = _lib.load()
    chunk = lib.mg_seq_mean_chunk()
    assert chunk > 0 and chunk % 1024 == 0
    assert lib.mg_seq_mean_workspace_bytes(3, 7, 5) >= 3 * 8
    assert lib.mg_seq_mean_workspace_bytes(64, chunk + 1, 1) >= 64 * 2 * 8 > lib.mg_seq_mean_workspace_bytes(64, chunk, 1) >= 64 * 8
    assert lib.mg_seq_mean_workspace_bytes(0, 7, 5) == 0 and lib.mg_seq_mean_workspace_bytes(3, 7, -1) == 0
    x, loss, ws = 1 << 20, 2 << 20, 3 << 20                    # never dereferenced: every call below is refused on the host
    ok = (x, 35, 5, 1, None, 3, 7, 5, loss, ws, 1 << 12, None)

    def fwd(**changed):
        names = ('x', 'stride_b', 'stride_t', 'stride_d', 'seq_len', 'B', 'T', 'D', 'loss', 'workspace', 'workspace_bytes', 'stream')
        args = dict(zip(names, ok))
        args.update(changed)
        return lib.mg_seq_mean_f32(*[args[n] for n in names])

    assert fwd(x=None) == _lib.MG_EINVAL and 'mg_seq_mean_f32' in _lib.last_error() and 'NULL' in _lib.last_error()
    assert fwd(loss=None) == _lib.MG_EINVAL
    for dim in ('B', 'T', 'D'):
        assert fwd(**{dim: 0}) == _lib.MG_EINVAL and '%s=0' % dim in _lib.last_error()
        assert fwd(**{dim: -2}) == _lib.MG_EINVAL
    assert fwd(B=65536) == _lib.MG_EINVAL and '65535' in _lib.last_error()
    assert fwd(stride_t=-5) == _lib.MG_EINVAL and 'stride' in _lib.last_error()
    assert fwd(x=x + 2) == _lib.MG_EINVAL and 'aligned' in _lib.last_error()
    assert fwd(workspace=None) == _lib.MG_EWORKSPACE and 'workspace' in _lib.last_error()
    assert fwd(workspace_bytes=16) == _lib.MG_EWORKSPACE and 'got 16' in _lib.last_error()
    with pytest.raises(_lib.MorganaHipError):
        _lib.check(fwd(workspace_bytes=0), 'mg_seq_mean_f32')
    with pytest.raises(ValueError):
        _lib.check(fwd(T=0), 'mg_seq_mean_f32')

    g, grad = 1 << 20, 2 << 20
    assert lib.mg_seq_mean_bwd_f32(None, None, 3, 7, 5, grad, None) == _lib.MG_EINVAL and 'mg_seq_mean_bwd_f32' in _lib.last_error()
    assert lib.mg_seq_mean_bwd_f32(g, None, 3, 7, 5, None, None) == _lib.MG_EINVAL
    for shape in ((0, 7, 5), (3, 0, 5), (3, 7, 0), (-1, 7, 5)):
        assert lib.mg_seq_mean_bwd_f32(g, None, *shape, grad, None) == _lib.MG_EINVAL and 'bad shape' in _lib.last_error()
    assert lib.mg_seq_mean_bwd_f32(g, None, 65536, 7, 5, grad, None) == _lib.MG_EINVAL
    assert lib.mg_seq_mean_bwd_f32(g, None, 3, 7, 5, grad + 1, None) == _lib.MG_EINVAL and 'aligned' in _lib.last_error()
    assert tuple(_lib.SIGNATURES['mg_seq_mean_bwd_f32']) == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p])
    assert _lib.SIGNATURES['mg_seq_mean_f32'][1][1:4] == [ctypes.c_int64] * 3


# ------------------------------------------------------------------------------------------------------------ Stream(loss=callable)
def _layers(width):
    return utils.SequentialWithRecurrent(nn.Linear(609, 8), nn.Sigmoid(), nn.Linear(8, width), precision='fp32')


def test_stream_with_a_callable_loss_is_a_delta_stream():
    l1 = losses.sequence_loss(lambda p, y: torch.abs(p - y))
    custom, plain = models.Stream('mcep', 6, loss=l1), models.Stream('mcep', 6, 'mse')
    assert custom.is_delta and not custom.is_categorical
    assert custom.output_key == plain.output_key == 'normalised_mcep_deltas'
    for kind, is_delta, key in (('mse', True, 'normalised_lf0_deltas'), ('sigmoid_bce', False, 'lf0'), ('ce', False, 'lf0_logits')):
        st = models.Stream('lf0', 3, kind)                      # nothing changes for the string kinds
        assert st.is_delta == is_delta and st.output_key == key and st.is_categorical == (kind == 'ce')
    model = models.StreamModel(_layers(9), [models.Stream('lf0', 3, 'mse'), custom])
    sources = model.normaliser_sources()
    assert sources['mcep'].use_deltas and type(sources['mcep']) is type(sources['lf0'])
    assert model._target({'normalised_mcep_deltas': 'y'}, custom) == 'y'


def test_stream_model_refuses_fused_loss_with_a_callable_stream():
    l1 = losses.sequence_loss(lambda p, y: torch.abs(p - y))
    streams = [models.Stream('lf0', 3, 'mse'), models.Stream('mcep', 6, loss=l1)]
    with pytest.raises(ValueError, match='mcep'):
        models.StreamModel(_layers(9), streams, fused_loss=True)
    models.StreamModel(_layers(9), streams, fused_loss=False)
    models.StreamModel(_layers(9), [models.Stream('lf0', 3, 'mse'), models.Stream('mcep', 6, 'mse')], fused_loss=True)
