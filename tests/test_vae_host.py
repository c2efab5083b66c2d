"""CPU-only checks of the latent-conditioned model surface (BaseVAE, KLD_standard_normal, VAEF0Model) and of the C-ABI entry points
of csrc/vae.hip: the API exists, the contract mirrors the reference's BaseVAE, CPU tensors raise, and bad arguments are refused on the
host before any launch."""
import torch
import torch.nn as nn
import pytest

from morgana_amd import _lib, base_models, functional as F_hip, losses, models, ops, utils


class _TinyVAE(base_models.BaseVAE):
    def __init__(self):
        super(_TinyVAE, self).__init__(z_dim=4, kld_weight=0.5)
        self.enc = nn.Linear(3, 8)
        self.dec = nn.Linear(4, 2)

    def encode(self, features):
        out = self.enc(features['x'])
        return out[:, :4], out[:, 4:]

    def decode(self, latent, features):
        return {'y': self.dec(latent)}

    def loss(self, features, output_features):
        return losses.KLD_standard_normal(output_features['mean'], output_features['log_variance'])


def test_api_exists():
    assert issubclass(base_models.BaseVAE, base_models.BaseSPSS)
    assert callable(losses.KLD_standard_normal)
    assert issubclass(models.VAEF0Model, base_models.BaseVAE)
    for name in ('vae_sample', 'vae_sample_backward', 'kld_standard_normal', 'kld_standard_normal_backward', 'gather_concat_latent',
                 'rows_add_per_item', 'rows_sum_per_item'):
        assert callable(getattr(ops, name)), name
    for name in ('SampleFn', 'KLDFn', 'LatentConcatFn'):
        assert issubclass(getattr(F_hip, name), torch.autograd.Function), name


def test_base_vae_contract():
    model = _TinyVAE()
    assert model.z_dim == 4 and model.kld_weight == 0.5
    assert 'kld' in model.metrics['all'] and 'loss' in model.metrics['all']
    bare = base_models.BaseVAE()
    assert bare.z_dim == 16 and bare.kld_weight == 1.
    with pytest.raises(NotImplementedError):
        bare.encode({})
    with pytest.raises(NotImplementedError):
        bare.decode(None, {})
    # predict without a latent decodes the zero vector (batch size from the first feature)
    captured = {}

    def decode(latent, features):
        captured['latent'] = latent
        return {}
    model.decode = decode
    model.predict({'x': torch.zeros(5, 3)})
    assert tuple(captured['latent'].shape) == (5, 4) and not captured['latent'].any()
    given = torch.ones(5, 4)
    model.predict({'x': torch.zeros(5, 3), 'latent': given})
    assert captured['latent'] is given


def test_vae_f0_model_state_dict_keys():
    model = models.VAEF0Model()
    keys = set(model.state_dict())
    gru = models.GRUF0Model()
    assert {k for k in keys if k.startswith('layers.')} == set(gru.state_dict())
    assert model.state_dict()['layers.0.weight'].shape == (256, 609 + 16)
    assert keys - set(gru.state_dict()) == {
        'encoder.0.layer.weight_ih_l0', 'encoder.0.layer.weight_hh_l0', 'encoder.0.layer.bias_ih_l0', 'encoder.0.layer.bias_hh_l0',
        'encoder_projection.0.weight', 'encoder_projection.0.bias'}
    assert model.state_dict()['encoder.0.layer.weight_ih_l0'].shape == (3 * 64, 3)
    assert model.state_dict()['encoder_projection.0.weight'].shape == (32, 64)
    small = models.VAEF0Model(z_dim=8, encoder_hidden=32)
    assert small.state_dict()['encoder_projection.0.weight'].shape == (16, 32)
    assert small.state_dict()['layers.0.weight'].shape == (256, 609 + 8)
    assert 'kld' in model.metrics['all'] and 'LF0_RMSE_Hz' in model.metrics['all']


def test_cpu_tensors_raise():
    mean, logvar = torch.zeros(4, 3), torch.zeros(4, 3)
    with pytest.raises(_lib.MorganaHipError):
        losses.KLD_standard_normal(mean, logvar)
    with pytest.raises(_lib.MorganaHipError):
        _TinyVAE().sample(mean, logvar)
    with pytest.raises(_lib.MorganaHipError):
        _TinyVAE()({'x': torch.zeros(2, 3)})
    with pytest.raises(_lib.MorganaHipError):
        ops.gather_concat_latent(torch.zeros(4, 8), None, torch.zeros(4, 2), torch.zeros(2, 3), 2)
    with pytest.raises(_lib.MorganaHipError):
        utils.concat_frame_features(torch.zeros(2, 3, 4), torch.zeros(2, 3, 1), torch.zeros(2, 5))


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    # sampler: null pointers, row strides narrower than Z
    assert lib.mg_vae_sample_f32(None, 4, 16, 4, 8, 4, 1, 0, None, 16, 16, None) == -1 and 'mg_vae_sample_f32' in _lib.last_error()
    assert lib.mg_vae_sample_f32(16, 3, 16, 4, 8, 4, 1, 0, None, 16, 16, None) == -1 and 'ldm=3' in _lib.last_error()
    assert lib.mg_vae_sample_f32(16, 4, 16, 4, 0, 4, 1, 0, None, 16, 16, None) == 0             # nothing to draw: no launch
    assert lib.mg_vae_sample_bwd_f32(16, 16, 16, 2, 8, 4, 16, 16, None) == -1 and 'ldv=2' in _lib.last_error()
    assert lib.mg_vae_sample_bwd_f32(16, 16, 16, 4, 8, 0, 16, 16, None) == -1
    # KLD: at least one row, strides
    assert lib.mg_kld_standard_normal_f32(16, 4, 16, 4, 0, 4, 16, None) == -1 and 'rows=0' in _lib.last_error()
    assert lib.mg_kld_standard_normal_f32(16, 4, 16, 1, 3, 4, 16, None) == -1 and 'ldv=1' in _lib.last_error()
    assert lib.mg_kld_standard_normal_bwd_f32(None, 16, 4, 16, 4, 3, 4, 16, 16, None) == -1
    # latent concat: extra exactly when C > 0, ldo wide enough, rows per item > 0, bf16 alignment and padding
    assert lib.mg_gather_concat_latent_f32(16, None, None, 16, 16, 8, 4, 2, 3, 4, 9, None) == -1 and 'extra' in _lib.last_error()
    assert lib.mg_gather_concat_latent_f32(16, None, 16, 16, 16, 8, 4, 2, 3, 4, 8, None) == -1 and 'ldo=8' in _lib.last_error()
    assert lib.mg_gather_concat_latent_f32(16, None, 16, 16, 16, 8, 4, 2, 3, 0, 9, None) == -1 and 'rows_per_item=0' in _lib.last_error()
    assert lib.mg_gather_concat_latent_f32(16, None, 16, 16, 16, 0, 4, 2, 3, 4, 9, None) == 0          # no rows: no launch
    assert lib.mg_gather_concat_latent_bf16(16, None, 16, 16, 16, 8, 4, 2, 3, 4, 12, None) == -1 and 'multiple of 8' in _lib.last_error()
    assert lib.mg_gather_concat_latent_bf16(16, None, 16, 16, 24, 8, 4, 2, 3, 4, 16, None) == -1 and '16-byte aligned' in _lib.last_error()
    # per-item row add / row sum
    assert lib.mg_rows_add_per_item_f32(16, 4, 8, 8, 16, 8, 4, None) == -1 and 'ldp=4' in _lib.last_error()
    assert lib.mg_rows_add_per_item_f32(16, 8, 8, 8, 16, 8, 0, None) == -1
    assert lib.mg_rows_sum_per_item(16, 4, 0, None, 0, 2, 4, 8, 16, 8, None) == -1 and 'ldg=4' in _lib.last_error()
    assert lib.mg_rows_sum_per_item(16, 8, 0, 16, 4, 2, 4, 8, 16, 8, None) == -1 and 'ldh=4' in _lib.last_error()
    assert lib.mg_rows_sum_per_item(16, 8, 1, None, 0, 70000, 4, 8, 16, 8, None) == -1 and '65535' in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(lib.mg_rows_sum_per_item(None, 8, 0, None, 0, 2, 4, 8, 16, 8, None), 'mg_rows_sum_per_item')


def test_latent_concat_shape_is_refused_before_the_device():
    class _Up(object):
        shape = (2, 5, 4)
    with pytest.raises(RuntimeError):
        utils.UpsampledConcat(_Up(), torch.zeros(2, 5, 1), torch.zeros(3, 4))
