"""``morgana_amd.sampling`` on the device (csrc/sampling.hip): both samplers against the float64 restatement of their Philox mapping
and arithmetic (tests/sampling_ref64.py, which test_sampling_host.py pins to the reference), held to the fp32 bounds derived there;
the invariants of the two surfaces; gradients; the counter scheme; the uniform sphere law; graph replay; and a VAE's predict() fed
a sampled latent."""
import ctypes
import math

import numpy as np
import pytest
import torch

import sampling_ref64 as ref
from morgana_amd import _lib, data, models, ops, sampling, synthetic
from morgana_amd import functional as F_hip

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SEED = 0x0123456789ABCDEF
CTR = 5 + (3 << 32)


def _counter(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def _philox(counter, key):
    c, k, out = (ctypes.c_uint32 * 4)(*counter), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
    _lib.load().mg_philox4x32_10(c, k, out)
    return [int(v) for v in out]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _worst(got, want, bound):
    """max |got - want| / bound (0 / 0 counts as 0): <= 1 means every element is inside its bound."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


# ----------------------------------------------------------------------------------------------------------------------- sphere
# 3, 13, 65: Philox blocks straddle the rows; 256 / 257: the last row kept in registers and the first chunked one; 600: chunks
SPHERE_SHAPES = [(1, 1), (37, 3), (37, 13), (5, 65), (2, 256), (2, 257), (3, 600)]


@pytest.mark.parametrize('rows,d', SPHERE_SHAPES)
def test_sphere_equals_host_restatement(rows, d):
    rng = np.random.RandomState(100 + d)
    centre, radius = rng.standard_normal(d).astype(np.float32), np.float32(1.7)
    out, unit = ops.sphere_sample(_dev(centre), _dev([radius]), rows, SEED, ops.SPHERE_SITE, _counter(CTR))
    out, unit = out.cpu().numpy(), unit.cpu().numpy()
    assert out.shape == (rows, d) and unit.shape == (rows, d)
    want = ref.sphere(centre, radius, ref.normal_noise(rows, d, SEED, ops.SPHERE_SITE, CTR, _philox))
    worst_unit, worst_out = _worst(unit, want['unit'], want['unit_bound']), _worst(out, want['out'], want['out_bound'])
    print('sphere %dx%d: direction at %.3f of its bound, points at %.3f' % (rows, d, worst_unit, worst_out))
    assert worst_unit <= 1.0 and worst_out <= 1.0
    # the surface: |unit| = 1 and |out - centre| = radius in every row
    norm = np.sqrt((unit.astype(np.float64) ** 2).sum(-1))
    dist = np.sqrt(((out.astype(np.float64) - centre.astype(np.float64)) ** 2).sum(-1))
    print('   | |unit| - 1 | %.3g (bound %.3g), | |out - centre| - radius | %.3g' % (np.abs(norm - 1).max(), ref.rho_own(d),
                                                                                    np.abs(dist - radius).max()))
    assert (np.abs(norm - 1.0) <= ref.rho_own(d)).all()
    assert (np.abs(dist - float(radius)) <= ref.sphere_radius_bound(out, radius)).all()
    if d == 1:
        assert (np.abs(unit) == 1.0).all()
        assert np.array_equal(out, centre + radius * unit)                              # fp32: exactly centre +- radius


# -------------------------------------------------------------------------------------------------------------------- ellipsoid
@pytest.mark.parametrize('d', [2, 3, 16, 65, 130])
def test_ellipsoid_equals_host_restatement(d):
    rows = 7
    rng = np.random.RandomState(200 + d)
    radii = (0.5 + rng.rand(d)).astype(np.float32)
    out, factor = ops.ellipsoid_sample(_dev(radii), rows, SEED, ops.ELLIPSOID_SITE, _counter(CTR))
    out, factor = out.cpu().numpy(), factor.cpu().numpy()
    angles = ref.uniform_angles(rows, d, SEED, ops.ELLIPSOID_SITE, CTR, _philox)
    want = ref.ellipsoid(radii, angles)
    worst_f, worst_o = _worst(factor, want['factor'], want['factor_bound']), _worst(out, want['out'], want['out_bound'])
    print('ellipsoid %dx%d: factor at %.3f of its bound, points at %.3f' % (rows, d, worst_f, worst_o))
    assert worst_f <= 1.0 and worst_o <= 1.0
    # sum factor^2 = 1 is an identity of the construction: the restatement has it, and so must the kernel with equal radii
    r = np.float32(1.5)
    equal = ref.ellipsoid(np.full(d, r), angles)['out']
    np.testing.assert_allclose(np.sqrt((equal ** 2).sum(-1)), float(r), rtol=1e-13)
    out_r = ops.ellipsoid_sample(_dev(np.full(d, r)), rows, SEED, ops.ELLIPSOID_SITE, _counter(CTR))[0].cpu().numpy().astype(np.float64)
    dev_norm = np.abs(np.sqrt((out_r ** 2).sum(-1)) - float(r)).max()
    print('   | |out| - r | %.3g (bound %.3g)' % (dev_norm, float(r) * (ref.ellipsoid_norm_rho(d) + ref.U)))
    assert dev_norm <= float(r) * (ref.ellipsoid_norm_rho(d) + ref.U)
    # sample_angles' kernel draws the same angles: fp32 pi (2.8e-8 relative, below U) times the exact 2 u or u, one product: 2 U
    got = ops.ellipsoid_angles(rows, d, DEV, SEED, ops.ELLIPSOID_SITE, _counter(CTR)).cpu().numpy()
    assert got.shape == (rows, d - 1) and (np.abs(got - angles) <= 2 * ref.U * angles).all()


# -------------------------------------------------------------------------------------------------------------------- gradients
# columns: 13 -> four rows side by side in a wave; 40 -> one row a wave; 65 -> two workgroups; 300 rows: every wave sums several
@pytest.mark.parametrize('rows,d', [(37, 13), (300, 3), (70, 40), (5, 65)])
def test_sphere_gradients(rows, d, monkeypatch):
    monkeypatch.setattr(ops, 'dropout_draw', lambda device: _counter(CTR))
    rng = np.random.RandomState(300 + d)
    centre = _dev(rng.standard_normal(d)).requires_grad_(True)
    radius = _dev([1.3]).requires_grad_(True)
    up = rng.standard_normal((rows, d)).astype(np.float32)
    out = F_hip.SphereSampleFn.apply(centre, radius, rows)
    out.backward(_dev(up))
    fwd = ref.sphere(centre.detach().cpu().numpy(), np.float32(1.3), ref.normal_noise(rows, d, ops.dropout_seed(), ops.SPHERE_SITE, CTR, _philox))
    assert _worst(out.detach().cpu().numpy(), fwd['out'], fwd['out_bound']) <= 1.0
    want = ref.sphere_grads(up, fwd['unit'], fwd['unit_bound'])
    worst_c = _worst(centre.grad.cpu().numpy(), want['dcentre'], want['dcentre_bound'])
    worst_r = _worst(radius.grad.cpu().numpy(), want['dradius'], want['dradius_bound'])
    print('sphere grads %dx%d: dcentre at %.3f of its bound, dradius at %.3f' % (rows, d, worst_c, worst_r))
    assert centre.grad.shape == (d,) and radius.grad.shape == (1,)
    assert worst_c <= 1.0 and worst_r <= 1.0
    unit = ops.sphere_sample(centre.detach(), radius.detach(), rows, ops.dropout_seed(), ops.SPHERE_SITE, _counter(CTR))[1]
    first, second = ops.sphere_sample_backward(_dev(up), unit), ops.sphere_sample_backward(_dev(up), unit)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert torch.equal(first[0], centre.grad) and torch.equal(first[1], radius.grad)
    # a Python radius is staged once and gets no gradient; centre still does
    sampler = sampling.UniformSphereSurfaceSampler(centre.detach().clone().requires_grad_(True), 1.3)
    points = sampler.rsample((rows,))
    points.backward(_dev(up))
    assert torch.equal(points.detach(), out.detach()) and torch.equal(sampler.centre.grad, centre.grad)


@pytest.mark.parametrize('rows,d', [(37, 13), (300, 3), (70, 40), (3, 130)])
def test_ellipsoid_gradients(rows, d, monkeypatch):
    monkeypatch.setattr(ops, 'dropout_draw', lambda device: _counter(CTR))
    rng = np.random.RandomState(400 + d)
    radii = _dev(0.5 + rng.rand(d)).requires_grad_(True)
    up = rng.standard_normal((rows, d)).astype(np.float32)
    sampler = sampling.UniformEllipsoidSurfaceApproximateSampler(torch.zeros(d, device=DEV), radii)
    out = sampler.rsample((rows,))
    out.backward(_dev(up))
    fwd = ref.ellipsoid(radii.detach().cpu().numpy(), ref.uniform_angles(rows, d, ops.dropout_seed(), ops.ELLIPSOID_SITE, CTR, _philox))
    assert _worst(out.detach().cpu().numpy(), fwd['out'], fwd['out_bound']) <= 1.0
    want = ref.ellipsoid_grads(up, fwd['factor'], fwd['factor_bound'])
    worst = _worst(radii.grad.cpu().numpy(), want['dradii'], want['dradii_bound'])
    print('ellipsoid grads %dx%d: dradii at %.3f of its bound' % (rows, d, worst))
    assert radii.grad.shape == (d,) and worst <= 1.0
    factor = ops.ellipsoid_sample(radii.detach(), rows, ops.dropout_seed(), ops.ELLIPSOID_SITE, _counter(CTR))[1]
    first, second = ops.ellipsoid_sample_backward(_dev(up), factor), ops.ellipsoid_sample_backward(_dev(up), factor)
    assert torch.equal(first, second) and torch.equal(first, radii.grad)


# --------------------------------------------------------------------------------------------------------------------- counters
def test_counters_sites_and_seed():
    centre, radius, radii = torch.zeros(16, device=DEV), torch.ones(1, device=DEV), torch.ones(16, device=DEV)
    draws = {'sphere': lambda seed, site, ctr: ops.sphere_sample(centre, radius, 64, seed, site, _counter(ctr))[0],
             'ellipsoid': lambda seed, site, ctr: ops.ellipsoid_sample(radii, 64, seed, site, _counter(ctr))[0]}
    for name, draw in draws.items():
        site = ops.SPHERE_SITE if name == 'sphere' else ops.ELLIPSOID_SITE
        a = draw(SEED, site, 11)
        assert torch.equal(a, draw(SEED, site, 11)), name                               # same (seed, site, counter), same draw
        assert not torch.equal(a, draw(SEED, site, 12)), name
        assert not torch.equal(a, draw(SEED, site, 11 + (1 << 32))), name               # the counter's high word counts too
        assert not torch.equal(a, draw(SEED, site + 1, 11)), name
        assert not torch.equal(a, draw(SEED ^ 1, site, 11)), name
        assert not torch.equal(a, draw(SEED ^ (1 << 40), site, 11)), name
        assert not torch.equal(a, draw(SEED, ops.SAMPLE_SITE, 11)), name
    assert len({ops.SAMPLE_SITE, ops.SPHERE_SITE, ops.ELLIPSOID_SITE}) == 3
    # the sphere's noise IS the VAE sampler's at the same four numbers: one mapping, documented once
    zeros = torch.zeros(64, 16, device=DEV)
    eps = ops.vae_sample(zeros, zeros, SEED, ops.SPHERE_SITE, _counter(11))[1].double()
    unit = ops.sphere_sample(centre, radius, 64, SEED, ops.SPHERE_SITE, _counter(11))[1].double()
    assert (unit - eps / eps.norm(dim=-1, keepdim=True)).abs().max().item() <= ref.rho_own(16)

    samplers = (sampling.UniformSphereSurfaceSampler(centre, 2.0), sampling.UniformEllipsoidSurfaceApproximateSampler(centre, radii))
    state = ops.dropout_state(DEV)
    keep_seed = torch.initial_seed()
    try:
        for sampler in samplers:
            runs = []
            for seed in (5, 5, 6):
                torch.manual_seed(seed)
                state.zero_()
                runs.append((sampler.rsample((4,)), sampler.sample((4,))))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])   # torch.manual_seed: repeatable
            assert not torch.equal(runs[0][0], runs[2][0])
            assert not torch.equal(runs[0][0], runs[0][1])                                 # every call draws new noise
            assert runs[0][0].shape == (4, 16) and not runs[0][1].requires_grad
            assert sampler.rsample().shape == (16,) and sampler.rsample((2, 3)).shape == (2, 3, 16)
        assert samplers[1].sample_angles([2, 3]).shape == (2, 3, 15)
    finally:
        torch.manual_seed(keep_seed)


# ------------------------------------------------------------------------------------------------------------------- statistics
def test_sphere_statistics():
    """Properties of the uniform law on the unit sphere in D dimensions, not of the code: E x_c = 0, E x_c^2 = 1 / D (the squares sum
    to 1 and the coordinates are exchangeable), E x_c^4 = 3 / (D (D + 2)) (x_c^2 ~ Beta(1/2, (D - 1)/2)), so Var x_c^2 =
    2 (D - 1) / (D^2 (D + 2)).  Over n rows the two sample means have sigma = 1 / sqrt(D n) and sqrt(Var x_c^2 / n)."""
    rows, d = 1 << 18, 16
    out, unit = ops.sphere_sample(torch.zeros(d, device=DEV), torch.ones(1, device=DEV), rows, SEED, ops.SPHERE_SITE, _counter(7))
    assert torch.equal(out, unit) and torch.isfinite(out).all()
    x = out.double()
    mean, mean_sq = x.mean(0).cpu().numpy(), (x * x).mean(0).cpu().numpy()
    sigma = 1.0 / math.sqrt(d * rows)
    sigma_sq = math.sqrt(2.0 * (d - 1) / (d * d * (d + 2.0)) / rows)
    print('statistics: |mean| %.3g (5 sigma %.3g), |mean x^2 - 1/D| %.3g (5 sigma %.3g)'
          % (np.abs(mean).max(), 5 * sigma, np.abs(mean_sq - 1.0 / d).max(), 5 * sigma_sq))
    assert (np.abs(mean) <= 5 * sigma).all()
    assert (np.abs(mean_sq - 1.0 / d) <= 5 * sigma_sq).all()


# ------------------------------------------------------------------------------------------------------------------------ graph
@pytest.mark.parametrize('kind', ['sphere', 'ellipsoid'])
def test_graph_replay_draws_new_noise(kind):
    centre, r = torch.arange(16, dtype=torch.float32, device=DEV) / 8, 2.0
    sampler = (sampling.UniformSphereSurfaceSampler(centre, r) if kind == 'sphere'
               else sampling.UniformEllipsoidSurfaceApproximateSampler(centre, r))
    ops.dropout_state(DEV)
    sampler.rsample((8,))                                             # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        z = sampler.rsample((8,))
    graph.replay()
    first = z.clone()
    graph.replay()
    second = z.clone()
    torch.cuda.synchronize()
    assert first.shape == (8, 16) and not torch.equal(first, second)
    for points in (first, second):
        p = points.cpu().numpy()
        if kind == 'sphere':
            dist = np.sqrt(((p.astype(np.float64) - centre.cpu().numpy().astype(np.float64)) ** 2).sum(-1))
            assert (np.abs(dist - r) <= ref.sphere_radius_bound(p, r)).all()
        else:                                                          # equal radii; the centre is not added
            dist = np.sqrt((p.astype(np.float64) ** 2).sum(-1))
            assert (np.abs(dist - r) <= r * (ref.ellipsoid_norm_rho(16) + ref.U)).all()


# ------------------------------------------------------------------------------------------------------------------- end to end
def test_vae_predict_on_a_sampled_latent():
    feats = synthetic.make_acoustic_batch(4, (40, 90), streams=(('lf0', 3, 'mse'),), seed=41)
    torch.manual_seed(4)
    model = models.VAEF0Model(precision='fp32').to(DEV)
    assert model.z_dim == 16
    d = data.to_device(feats, DEV)
    sampler = sampling.UniformSphereSurfaceSampler(torch.zeros(16, device=DEV), 2.0)
    with torch.no_grad():
        latent = sampler.rsample((4,))
        pred = model.predict(dict(d, latent=latent))['normalised_lf0_deltas']
        pred_zero = model.predict(d)['normalised_lf0_deltas']
        pred_plain = model.predict(dict(d, latent=torch.from_numpy(latent.cpu().numpy()).to(DEV)))['normalised_lf0_deltas']
    assert latent.shape == (4, 16) and torch.isfinite(pred).all()
    assert not torch.equal(pred, pred_zero)
    assert torch.equal(pred, pred_plain)
