"""Latent-conditioned models on the HIP path (csrc/vae.hip, base_models.BaseVAE, models.VAEF0Model): the sampler against a host
restatement of its Philox / Box-Muller mapping, the KLD and the latent-conditioned first layer against torch on the CPU, the shipped
VAE F0 model in every precision, and the training loop graphed against eager."""
import ctypes
import json
import math
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from morgana_amd import _lib, data, experiment_builder, losses, models, ops, synthetic, utils
from morgana_amd import functional as F_hip

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SEED = 0x0123456789ABCDEF


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)


def _counter(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def _philox(counter, key):
    c, k, out = (ctypes.c_uint32 * 4)(*counter), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
    _lib.load().mg_philox4x32_10(c, k, out)
    return [int(v) for v in out]


def _host_noise(n, seed, site, ctr):
    """The mapping include/morgana_hip.h documents for mg_vae_sample_f32, in float64 on the host."""
    u = lambda w: float((w >> 8) | 1) * 2.0 ** -24
    out = np.empty(4 * ((n + 3) // 4))
    for q in range((n + 3) // 4):
        x, y, z, w = _philox([q & 0xFFFFFFFF, q >> 32, ctr & 0xFFFFFFFF, (site ^ (ctr >> 32)) & 0xFFFFFFFF],
                             [seed & 0xFFFFFFFF, seed >> 32])
        r0, r1 = math.sqrt(-2.0 * math.log(u(x))), math.sqrt(-2.0 * math.log(u(z)))
        out[4 * q:4 * q + 4] = (r0 * math.cos(2 * math.pi * u(y)), r0 * math.sin(2 * math.pi * u(y)),
                                r1 * math.cos(2 * math.pi * u(w)), r1 * math.sin(2 * math.pi * u(w)))
    return out[:n]


# ------------------------------------------------------------------------------------------------------------------------ sampler
def test_sampler_matches_host_restatement_on_column_views():
    rng = np.random.RandomState(5)
    rows, zd = 37, 13
    stats = torch.from_numpy(rng.randn(rows, 2 * zd).astype(np.float32)).to(DEV)        # [mean | logvar] of one encoder output
    mean, logvar = stats[:, :zd], stats[:, zd:]
    ctr = 5 + (3 << 32)
    z, eps = ops.vae_sample(mean, logvar, SEED, ops.SAMPLE_SITE, _counter(ctr))
    want_eps = _host_noise(rows * zd, SEED, ops.SAMPLE_SITE, ctr).reshape(rows, zd)
    np.testing.assert_allclose(eps.cpu().numpy(), want_eps, rtol=1e-6, atol=1e-6)
    s64 = stats.cpu().double()
    want_z = s64[:, :zd] + torch.exp(0.5 * s64[:, zd:]) * eps.cpu().double()
    assert rel_err(z.cpu().numpy(), want_z.numpy()) < 1e-6


def test_sampler_statistics_and_counters():
    n_rows = (1 << 22) // 16
    zeros = torch.zeros(n_rows, 16, device=DEV)
    z, eps = ops.vae_sample(zeros, zeros, SEED, ops.SAMPLE_SITE, _counter(11))
    assert torch.equal(z, eps)
    e = eps.double()
    assert abs(e.mean().item()) < 3e-3 and abs(e.var().item() - 1.0) < 3e-3
    assert torch.isfinite(e).all()
    small = torch.zeros(64, 16, device=DEV)
    a = ops.vae_sample(small, small, SEED, ops.SAMPLE_SITE, _counter(11))[1]
    assert torch.equal(a, eps[:64])                                                         # same counter, same draw
    assert not torch.equal(a, ops.vae_sample(small, small, SEED, ops.SAMPLE_SITE, _counter(12))[1])
    assert not torch.equal(a, ops.vae_sample(small, small, SEED, ops.SAMPLE_SITE + 1, _counter(11))[1])
    assert not torch.equal(a, ops.vae_sample(small, small, SEED ^ 1, ops.SAMPLE_SITE, _counter(11))[1])


def test_sample_fn_forward_backward_vs_torch(monkeypatch):
    monkeypatch.setattr(ops, 'dropout_draw', lambda device: _counter(21))
    rng = np.random.RandomState(6)
    stats = torch.from_numpy(rng.randn(9, 2, 32).astype(np.float32)).to(DEV).requires_grad_(True)
    mean, logvar = stats[..., :16], stats[..., 16:]
    z = F_hip.SampleFn.apply(mean, logvar)
    _, eps = ops.vae_sample(mean.detach(), logvar.detach(), ops.dropout_seed(), ops.SAMPLE_SITE, _counter(21))
    up = torch.from_numpy(rng.randn(9, 2, 16).astype(np.float32))
    z.backward(up.to(DEV))
    ref = stats.detach().cpu().requires_grad_(True)
    want = ref[..., :16] + torch.exp(0.5 * ref[..., 16:]) * eps.cpu()
    want.backward(up)
    assert rel_err(z.detach().cpu().numpy(), want.detach().numpy()) < 1e-6
    assert rel_err(stats.grad.cpu().numpy(), ref.grad.numpy()) < 1e-6


def test_graph_replay_draws_new_noise():
    mean = torch.zeros(8, 16, device=DEV)
    ops.dropout_state(DEV)
    F_hip.SampleFn.apply(mean, mean)                                  # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        z = F_hip.SampleFn.apply(mean, mean)
    graph.replay()
    first = z.clone()
    graph.replay()
    second = z.clone()
    torch.cuda.synchronize()
    assert not torch.equal(first, second)


# ------------------------------------------------------------------------------------------------------------------------ KLD
@pytest.mark.parametrize('shape', [(1, 1), (7, 16), (5, 9, 33), (257, 16)])
def test_kld_vs_torch(shape):
    rng = np.random.RandomState(sum(shape))
    m = rng.randn(*shape).astype(np.float32)
    lv = (0.7 * rng.randn(*shape)).astype(np.float32)
    mean, logvar = torch.from_numpy(m).to(DEV).requires_grad_(True), torch.from_numpy(lv).to(DEV).requires_grad_(True)
    kld = losses.KLD_standard_normal(mean, logvar)
    (1.7 * kld).backward()
    rm, rlv = torch.from_numpy(m).double().requires_grad_(True), torch.from_numpy(lv).double().requires_grad_(True)
    want = torch.mean(-0.5 * torch.sum(1 + rlv - rm ** 2 - torch.exp(rlv), dim=-1))
    (1.7 * want).backward()
    assert kld.shape == () and abs(kld.item() - want.item()) <= 1e-6 * abs(want.item())
    assert rel_err(mean.grad.cpu().numpy(), rm.grad.numpy()) < 1e-6
    assert rel_err(logvar.grad.cpu().numpy(), rlv.grad.numpy()) < 1e-6
    again = losses.KLD_standard_normal(mean.detach(), logvar.detach())
    assert torch.equal(again, kld.detach())                                                 # one fixed reduction order


def test_kld_reads_column_views_in_place():
    rng = np.random.RandomState(8)
    stats = torch.from_numpy(rng.randn(33, 24).astype(np.float32)).to(DEV).requires_grad_(True)
    kld = losses.KLD_standard_normal(stats[:, :12], stats[:, 12:])
    kld.backward()
    ref = stats.detach().cpu().double().requires_grad_(True)
    want = torch.mean(-0.5 * torch.sum(1 + ref[:, 12:] - ref[:, :12] ** 2 - torch.exp(ref[:, 12:]), dim=-1))
    want.backward()
    assert abs(kld.item() - want.item()) <= 1e-6 * abs(want.item())
    assert rel_err(stats.grad.cpu().numpy(), ref.grad.numpy()) < 1e-6


# ----------------------------------------------------------------------------------------------- latent-conditioned first layer
def test_latent_row_kernels_vs_torch():
    rng = np.random.RandomState(9)
    p = torch.from_numpy(rng.randn(3 * 7 + 2, 24).astype(np.float32)).to(DEV)
    u = torch.from_numpy(rng.randn(3, 24).astype(np.float32)).to(DEV)
    want = p.cpu().clone()
    want[:21] += u.cpu().repeat_interleave(7, dim=0)
    ops.rows_add_per_item(p, u, 21, 7)
    np.testing.assert_allclose(p.cpu().numpy(), want.numpy(), rtol=1e-6, atol=1e-6)
    g = torch.from_numpy(rng.randn(5 * 11, 70).astype(np.float32)).to(DEV)
    h = torch.rand(5 * 11, 70, device=DEV)
    s = ops.rows_sum_per_item(g, 5, 11)
    np.testing.assert_allclose(s.cpu().numpy(), g.cpu().double().view(5, 11, 70).sum(1).numpy(), rtol=1e-5, atol=1e-5)
    sh = ops.rows_sum_per_item(g, 5, 11, h=h)
    want_h = (g.cpu().double() * h.cpu().double() * (1 - h.cpu().double())).view(5, 11, 70).sum(1)
    np.testing.assert_allclose(sh.cpu().numpy(), want_h.numpy(), rtol=1e-5, atol=1e-5)
    gb = g.to(torch.bfloat16)
    sb = ops.rows_sum_per_item(gb, 5, 11, n=64)
    np.testing.assert_allclose(sb.cpu().numpy(), gb[:, :64].cpu().double().view(5, 11, 64).sum(1).numpy(), rtol=1e-5, atol=1e-5)


def _torch_upsample(lab, dur, t):
    out = torch.zeros(lab.shape[0], t, lab.shape[2], dtype=lab.dtype)
    for b in range(lab.shape[0]):
        rep = torch.repeat_interleave(lab[b], dur[b].reshape(-1), dim=0)
        out[b, :rep.shape[0]] = rep
    return out


def _torch_gru(gru, x, seq_len):
    packed = nn.utils.rnn.pack_padded_sequence(x, seq_len, batch_first=True, enforce_sorted=False)
    out, h_n = gru(packed)
    out, _ = nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=x.shape[1])
    return out, h_n


def _batch(seed, b=4, frames=(40, 90)):
    return synthetic.make_acoustic_batch(b, frames, streams=(('lf0', 3, 'mse'),), seed=seed)


def _cpu(feats):
    return {k: torch.from_numpy(v) for k, v in feats.items() if isinstance(v, np.ndarray)}


TOLS = {'fp32': (1e-4, 1e-3), 'bf16x3': (1e-4, 1e-3), 'bf16': (2e-2, 5e-2)}      # (output, gradients), max-normalised


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16'])
def test_latent_conditioned_stack_vs_torch(precision):
    feats = _batch(31)
    f, c, zd, t = 600, 9, 16, feats['normalised_counters'].shape[1]
    torch.manual_seed(2)
    stack = utils.SequentialWithRecurrent(nn.Linear(f + c + zd, 256), nn.Sigmoid(),
                                          utils.RecurrentCuDNNWrapper(nn.GRU(256, 64, batch_first=True)), nn.Linear(64, 3),
                                          precision=precision).to(DEV)
    ref_lin0, ref_gru, ref_lin1 = nn.Linear(f + c + zd, 256), nn.GRU(256, 64, batch_first=True), nn.Linear(64, 3)
    for mod, ref in ((stack[0], ref_lin0), (stack[2].layer, ref_gru), (stack[3], ref_lin1)):
        ref.load_state_dict({k: v.cpu() for k, v in mod.state_dict().items()})
    rng = np.random.RandomState(3)
    z_np = rng.randn(4, zd).astype(np.float32)
    w_np = rng.randn(4, t, 3).astype(np.float32)

    d = data.to_device(feats, DEV)
    z = torch.from_numpy(z_np).to(DEV).requires_grad_(True)
    up = utils.upsample_to_repetitions(d['normalised_lab'], d['dur'], max_len=t, fused=True)
    x = utils.concat_frame_features(up, d['normalised_counters'], z)
    assert isinstance(x, utils.UpsampledConcat) and x.shape == (4, t, f + c + zd)
    out, _ = stack(x, seq_len=d['n_frames'], max_len=t)
    (out * torch.from_numpy(w_np).to(DEV)).sum().backward()

    cf = _cpu(feats)
    rz = torch.from_numpy(z_np).requires_grad_(True)
    rx = torch.cat((_torch_upsample(cf['normalised_lab'], cf['dur'], t), cf['normalised_counters'], rz[:, None, :].expand(4, t, zd)), -1)
    h, _ = _torch_gru(ref_gru, torch.sigmoid(ref_lin0(rx)), cf['n_frames'])
    want = ref_lin1(h)
    (want * torch.from_numpy(w_np)).sum().backward()

    tol_out, tol_grad = TOLS[precision]
    assert rel_err(out.detach().cpu().numpy(), want.detach().numpy()) < tol_out
    assert rel_err(z.grad.cpu().numpy(), rz.grad.numpy()) < tol_grad
    for mod, ref in ((stack[0], ref_lin0), (stack[2].layer, ref_gru), (stack[3], ref_lin1)):
        for (name, prm), (_, rprm) in zip(mod.named_parameters(), ref.named_parameters()):
            assert rel_err(prm.grad.cpu().numpy(), rprm.grad.numpy()) < tol_grad, name


def test_latent_concat_materialised_is_differentiable():
    feats = _batch(32)
    d = data.to_device(feats, DEV)
    t = feats['normalised_counters'].shape[1]
    z = torch.randn(4, 5, device=DEV, requires_grad=True)
    up = utils.upsample_to_repetitions(d['normalised_lab'], d['dur'], max_len=t, fused=True)
    x = utils.concat_frame_features(up, d['normalised_counters'], z).materialise()
    w = torch.randn(x.shape, device=DEV)
    (x * w).sum().backward()
    cf = _cpu(feats)
    want = torch.cat((_torch_upsample(cf['normalised_lab'], cf['dur'], t), cf['normalised_counters'],
                      z.detach().cpu()[:, None, :].expand(4, t, 5)), -1)
    assert torch.equal(x.detach().cpu(), want)
    np.testing.assert_allclose(z.grad.cpu().numpy(), w[..., -5:].sum(1).cpu().numpy(), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------------ VAEF0Model
def _torch_vae_f0(model, feats, eps, latent=None):
    """BaseVAE.forward of VAEF0Model restated in torch on the CPU (modules copied from ``model``): returns (loss, prediction, the
    restated modules by the model's parameter names)."""
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    zd, hid = model.z_dim, model.encoder[0].layer.hidden_size
    enc = nn.GRU(3, hid, batch_first=True)
    enc.load_state_dict({k[len('encoder.0.layer.'):]: v for k, v in sd.items() if k.startswith('encoder.0.layer.')})
    proj = nn.Linear(hid, 2 * zd)
    proj.load_state_dict({'weight': sd['encoder_projection.0.weight'], 'bias': sd['encoder_projection.0.bias']})
    lin = {i: nn.Linear(*sd['layers.%d.weight' % i].shape[::-1]) for i in (0, 9, 12)}
    for i, m in lin.items():
        m.load_state_dict({'weight': sd['layers.%d.weight' % i], 'bias': sd['layers.%d.bias' % i]})
    grus = {}
    for i, n_in in ((3, 256), (5, 64), (7, 64)):
        grus[i] = nn.GRU(n_in, 64, batch_first=True)
        grus[i].load_state_dict({k[len('layers.%d.layer.' % i):]: v for k, v in sd.items() if k.startswith('layers.%d.layer.' % i)})
    cf = _cpu(feats)
    t = cf['normalised_counters'].shape[1]
    n_frames = cf['n_frames']
    _, h_n = _torch_gru(enc, cf['normalised_lf0_deltas'], n_frames)
    stats = proj(h_n[0])
    mean, logvar = stats[:, :zd], stats[:, zd:]
    z = mean + torch.exp(0.5 * logvar) * eps if latent is None else latent
    x = torch.cat((_torch_upsample(cf['normalised_lab'], cf['dur'], t), cf['normalised_counters'], z[:, None, :].expand(z.shape[0], t, zd)), -1)
    h = torch.sigmoid(lin[0](x))
    for i in (3, 5, 7):
        h, _ = _torch_gru(grus[i], h, n_frames)
    pred = lin[12](torch.sigmoid(lin[9](h)))
    mask = (torch.arange(t)[None, :] < n_frames[:, None]).float()[..., None]
    mse = ((pred - cf['normalised_lf0_deltas']) ** 2 * mask).sum(1) / n_frames[:, None].float()
    kld = torch.mean(-0.5 * torch.sum(1 + logvar - mean ** 2 - torch.exp(logvar), dim=-1))
    loss = mse.mean() + model.kld_weight * kld
    named = {'encoder.0.layer.' + k: v for k, v in enc.named_parameters()}
    named.update({'encoder_projection.0.' + k: v for k, v in proj.named_parameters()})
    for i, m in lin.items():
        named.update({'layers.%d.%s' % (i, k): v for k, v in m.named_parameters()})
    for i, m in grus.items():
        named.update({'layers.%d.layer.%s' % (i, k): v for k, v in m.named_parameters()})
    return loss, pred, named


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16'])
def test_vae_f0_model_vs_torch(precision, monkeypatch):
    monkeypatch.setattr(ops, 'dropout_draw', lambda device: _counter(77))
    feats = _batch(41)
    torch.manual_seed(4)
    model = models.VAEF0Model(kld_weight=0.3, precision=precision).to(DEV)
    d = data.to_device(feats, DEV)
    loss, out = model(d)
    loss.backward()
    assert set(('latent', 'mean', 'log_variance', 'normalised_lf0_deltas')) <= set(out)
    _, eps = ops.vae_sample(out['mean'].detach(), out['log_variance'].detach(), ops.dropout_seed(), ops.SAMPLE_SITE, _counter(77))
    want_loss, want_pred, named = _torch_vae_f0(model, feats, eps.cpu())
    want_loss.backward()
    tol_out, tol_grad = TOLS[precision]
    assert abs(loss.item() - want_loss.item()) <= tol_out * abs(want_loss.item())
    assert rel_err(out['normalised_lf0_deltas'].detach().cpu().numpy(), want_pred.detach().numpy()) < tol_out
    for name, prm in model.named_parameters():
        assert rel_err(prm.grad.cpu().numpy(), named[name].grad.numpy()) < tol_grad, name

    # predict: the decoder alone, on the given latent or on zeros
    with torch.no_grad():
        given = torch.from_numpy(np.random.RandomState(1).randn(4, 16).astype(np.float32))
        pred_given = model.predict(dict(d, latent=given.to(DEV)))['normalised_lf0_deltas']
        pred_zero = model.predict(d)['normalised_lf0_deltas']
        _, want_given, _ = _torch_vae_f0(model, feats, None, latent=given)
        _, want_zero, _ = _torch_vae_f0(model, feats, None, latent=torch.zeros(4, 16))
    assert rel_err(pred_given.cpu().numpy(), want_given.numpy()) < tol_out
    assert rel_err(pred_zero.cpu().numpy(), want_zero.numpy()) < tol_out


# -------------------------------------------------------------------------------------------------------------- the training loop
def test_experiment_builder_graphed_equals_eager(tmp_path):
    base = _batch(51, b=8, frames=(60, 100))
    batches = []
    for i in range(5):
        b = dict(base)
        b['normalised_lf0_deltas'] = (base['normalised_lf0_deltas'] * (1.0 + 0.1 * i)).astype(np.float32)
        batches.append(data.to_device(b, DEV))

    def train(use_graphs):
        torch.manual_seed(3)
        ops.dropout_state(DEV).zero_()
        builder = experiment_builder.ExperimentBuilder(models.VAEF0Model, dict(precision='bf16', dropout_prob=0.1), learning_rate=0.01,
                                                       device=DEV, use_graphs=use_graphs, graph_group=1)
        optimizer = builder.make_optimizer()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            history = [builder.train_epoch(batches, optimizer) for _ in range(2)]
        assert not [w for w in caught if 'captur' in str(w.message)], [str(w.message) for w in caught]
        params = {k: v.detach().clone() for k, v in builder.model.named_parameters()}
        return history, params, builder, ops.dropout_state(DEV).item()

    hist_e, params_e, _, draws_e = train(False)
    hist_g, params_g, builder, draws_g = train(True)
    assert builder._graph_cache.replayed_steps > 0, builder._graph_cache.stats()
    assert draws_g == draws_e > 0                              # every replay drew from the device counter, as the eager steps did
    assert hist_g == hist_e
    for name in params_e:
        assert torch.equal(params_g[name], params_e[name]), name

    valid_dir, test_dir = str(tmp_path / 'valid'), str(tmp_path / 'test')
    builder.valid_epoch(batches[:2], out_dir=valid_dir)
    builder.test_epoch(batches[:2], out_dir=test_dir)
    for out_dir in (valid_dir, test_dir):
        with open(os.path.join(out_dir, 'metrics.json')) as f:
            assert 'kld' in json.load(f)
