"""CPU-only checks of global gradient-norm clipping (optim.Adam(max_grad_norm=), csrc/clip.hip's host side): the float64
restatement against torch, the optimiser's seam path against clip_grad_norm_ + torch.optim.Adam, the slab-deferral switch, argument
validation of the new entry points and the two-rank mean semantics over gloo."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import clip_ref64
import helpers
from morgana_amd import _lib, experiment_builder, optim, synthetic
from oracle import ref_torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_clip(buffers, max_norm):
    """clip_grad_norm_ on float64 CPU copies of ``buffers`` -> (norm, [clipped])."""
    params = [torch.nn.Parameter(torch.zeros(b.shape, dtype=torch.float64)) for b in buffers]
    for p, b in zip(params, buffers):
        p.grad = torch.from_numpy(np.asarray(b, dtype=np.float64).copy())
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2, error_if_nonfinite=False)
    return float(norm), [p.grad.numpy() for p in params]


@pytest.mark.parametrize('case', ['bites', 'loose', 'zeros', 'inf', 'nan', 'huge'])
def test_clip_ref64_agrees_with_torch(case):
    rng = np.random.RandomState(5)
    buffers = [rng.standard_normal(n).astype(np.float32) for n in (301, 7, 64)]
    max_norm = 1000.0 if case == 'loose' else 0.75
    if case == 'zeros':
        buffers = [np.zeros_like(b) for b in buffers]
    elif case == 'inf':
        buffers[1][3] = np.inf
    elif case == 'nan':
        buffers[2][10] = np.nan
    elif case == 'huge':
        buffers = [b * np.float32(1e19) for b in buffers]           # squares beyond float32's range
    want_norm, want = _torch_clip(buffers, max_norm)
    norm, coef, got = clip_ref64.clip(buffers, max_norm)
    if case == 'nan':
        assert math.isnan(norm) and math.isnan(coef)
    else:
        assert norm == pytest.approx(want_norm, rel=1e-14)
    if case == 'inf':
        assert coef == 0.0
    if case == 'zeros':
        assert coef == 1.0
    if case == 'loose':
        assert coef == 1.0
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w, rtol=1e-14, atol=0.0, equal_nan=True)


def _fixed_grads(n_steps, shapes, seed=11):
    rng = np.random.RandomState(seed)
    # scales that put the norm on both sides of the threshold used below (1.0): steps 0, 2, 4 bite, 1 and 3 do not
    scales = [3.0, 1e-3, 40.0, 1e-2, 0.7]
    return [[(rng.standard_normal(s) * scales[i % len(scales)]).astype(np.float32) for s in shapes] for i in range(n_steps)]


def test_flat_adam_with_clipping_matches_torch():
    """Adam(max_grad_norm=c, kernel=<the oracle update>) over 5 steps of fixed gradients against clip_grad_norm_ + torch.optim.Adam in
    float64 - to the tolerance of test_host_logic.test_flat_adam_matches_torch_adam; two parameter groups share one norm."""
    shapes = [(12, 8), (8,), (5, 3), (1,)]
    rng = np.random.RandomState(2)
    init = [rng.uniform(-0.3, 0.3, size=s).astype(np.float32) for s in shapes]
    ours = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in init]
    ref = [torch.nn.Parameter(torch.from_numpy(a.astype(np.float64))) for a in init]
    groups = lambda ps: [{'params': ps[:2]}, {'params': ps[2:], 'lr': 0.005}]
    opt = optim.Adam(groups(ours), lr=0.02, weight_decay=1e-2, kernel=helpers.cpu_adam_kernel, max_grad_norm=1.0)
    opt_ref = torch.optim.Adam(groups(ref), lr=0.02, weight_decay=1e-2)
    norms = []
    for grads in _fixed_grads(5, shapes):
        opt.zero_grad()
        for p, q, g in zip(ours, ref, grads):
            p.grad.copy_(torch.from_numpy(g))
            q.grad = torch.from_numpy(g.astype(np.float64))
        want_norm = float(torch.nn.utils.clip_grad_norm_(ref, 1.0))
        opt_ref.step()
        opt.step()
        norm, coef = [float(v) for v in opt.grad_norms()[0]]
        norms.append(want_norm)
        assert norm == pytest.approx(want_norm, rel=1e-6)
        assert coef == pytest.approx(clip_ref64.coef(want_norm, 1.0), rel=1e-6)
    assert max(norms) > 1.0 > min(norms)                            # both sides of the threshold were taken
    for p, q in zip(ours, ref):
        np.testing.assert_allclose(p.detach().numpy(), q.detach().numpy(), rtol=1e-5, atol=1e-7)


def test_none_is_the_default_and_changes_nothing():
    a = torch.nn.Parameter(torch.ones(7))
    opt = optim.Adam([a], lr=0.01, kernel=helpers.cpu_adam_kernel)
    assert opt.max_grad_norm is None and opt.grad_norms() is None
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            optim.Adam([torch.nn.Parameter(torch.ones(3))], max_grad_norm=bad)


def test_clipping_switches_slab_deferral_off(monkeypatch):
    """The norm needs the finished gradient: ``defers_slabs()`` is False with clipping on, also in the fused loop on a device."""
    for clip, want in ((None, True), (2.0, False)):
        opt = optim.Adam([torch.nn.Parameter(torch.ones(4))], lr=0.01, fused_loop=True, max_grad_norm=clip)
        monkeypatch.setattr(opt, '_on_device', lambda: True)       # what it answers with its buffers on an MI355X
        assert opt.fused_loop and opt.defers_slabs() is want
    builder = experiment_builder.ExperimentBuilder(helpers.CpuF0Model, model_kwargs={'dims': (24, 16, 8, 1)}, device='cpu',
                                                   max_grad_norm=0.5)
    opt = builder.make_optimizer(kernel=helpers.cpu_adam_kernel)
    assert opt.max_grad_norm == 0.5 and opt.fused_loop and not opt.defers_slabs()
    assert experiment_builder.ExperimentBuilder(helpers.CpuF0Model, model_kwargs={'dims': (24, 16, 8, 1)},
                                                device='cpu').make_optimizer(kernel=helpers.cpu_adam_kernel).max_grad_norm is None


def test_graphed_step_refuses_a_clipping_optimiser_before_any_capture():
    """A clipped step runs as ordinary launches: GraphedTrainStep refuses it first thing (no device call, no capture)."""
    from morgana_amd import graphs
    model = helpers.init_small(helpers.CpuF0Model(dims=(24, 16, 8, 1)), seed=1)
    opt = optim.Adam(model.parameters(), lr=0.01, kernel=helpers.cpu_adam_kernel, max_grad_norm=1.0)
    with pytest.raises(RuntimeError, match='not captured'):
        graphs.GraphedTrainStep(model, opt, {}, warmup=0)
    assert graphs._capture_refusal(RuntimeError('x'))               # GraphedStepCache reads it as "keep this step eager"


def test_clip_entry_points_validate_their_arguments_without_a_gpu():
    lib = _lib.load()
    # the grid is a function of n alone: at most 1024 chunks, multiples of 1024 floats, at least 4096
    for n, chunk, blocks in ((1, 4096, 1), (4096, 4096, 1), (4097, 4096, 2), (1000003, 4096, 245), (4096 * 1024, 4096, 1024),
                             (4096 * 1024 + 1, 5120, 820), (17500000, 17408, 1006)):
        assert (lib.mg_grad_clip_chunk(n), lib.mg_grad_clip_blocks(n)) == (chunk, blocks), n
    assert lib.mg_grad_clip_chunk(0) == 0 and lib.mg_grad_clip_blocks(-5) == 0
    fake_g, fake_p, fake_o = 1 << 20, 1 << 21, 1 << 22              # never dereferenced: every call below is refused before a launch
    assert lib.mg_grad_sumsq_f32(fake_g, 0, fake_p, 0, 4, None) == -1 and 'n=0' in _lib.last_error()
    assert lib.mg_grad_sumsq_f32(None, 16, fake_p, 0, 4, None) == -1 and 'NULL' in _lib.last_error()
    assert lib.mg_grad_sumsq_f32(fake_g, 16, None, 0, 4, None) == -1
    assert lib.mg_grad_sumsq_f32(fake_g + 2, 16, fake_p, 0, 4, None) == -1 and 'aligned' in _lib.last_error()
    assert lib.mg_grad_sumsq_f32(fake_g, 16, fake_p, 4, 4, None) == -1 and 'do not fit' in _lib.last_error()
    assert lib.mg_grad_sumsq_f32(fake_g, 3 * 4096, fake_p, 2, 4, None) == -1 and 'do not fit' in _lib.last_error()
    assert lib.mg_grad_sumsq_f32(fake_g, 16, fake_p, -1, 4, None) == -1
    assert lib.mg_grad_sumsq_f32(fake_g, 16, fake_p, 0, _lib.MG_CLIP_MAX_PARTIALS + 1, None) == -1 and 'n_partials' in _lib.last_error()
    assert lib.mg_grad_clip_scale_f32(fake_g, 0, fake_p, 1, 1.0, 1.0, fake_o, None) == -1 and 'n=0' in _lib.last_error()
    assert lib.mg_grad_clip_scale_f32(None, 16, fake_p, 1, 1.0, 1.0, fake_o, None) == -1
    assert lib.mg_grad_clip_scale_f32(fake_g, 16, None, 1, 1.0, 1.0, fake_o, None) == -1
    assert lib.mg_grad_clip_scale_f32(fake_g, 16, fake_p, 0, 1.0, 1.0, fake_o, None) == -1 and 'n_partials' in _lib.last_error()
    for bad in (0.0, -2.0, float('nan')):
        assert lib.mg_grad_clip_scale_f32(fake_g, 16, fake_p, 1, 1.0, bad, fake_o, None) == -1 and 'max_norm' in _lib.last_error()
    for bad in (0.0, 1.5, float('nan')):
        assert lib.mg_grad_clip_scale_f32(fake_g, 16, fake_p, 1, bad, 1.0, fake_o, None) == -1 and 'inv_world' in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(-1, 'mg_grad_clip_scale_f32')


def _single_process_clipped(n_steps, max_norm):
    """One process on the whole batch: torch's own clip_grad_norm_ between backward and a step of the unclipped flat Adam."""
    torch.set_num_threads(1)
    model = helpers.init_small(helpers.CpuF0Model(dims=(24, 16, 8, 1)), seed=1)
    batch = ref_torch.to_torch(synthetic.make_batch(8, 50, lab_dim=24, frames_per_phone=5.0, seed=17))
    opt = optim.Adam(model.parameters(), lr=0.01, weight_decay=1e-3, kernel=helpers.cpu_adam_kernel)
    norms = []
    for _ in range(n_steps):
        opt.zero_grad()
        loss, _ = model(batch)
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(model.parameters()), max_norm)))
        opt.step()
    return opt.flat_buffers()['param'].numpy().copy(), norms


@pytest.mark.parametrize('max_norm', [0.05, 0.9])
def test_two_ranks_clip_the_mean_gradient(tmp_path, max_norm):
    """Two gloo ranks with half the batch each, under a threshold that bites, end at the parameters of one process with the whole
    batch: the norm is taken on the MEAN over ranks (a norm of the summed buffer would be twice as large and clip twice as hard).
    0.05 bites at every step by more than a factor of 2; 0.9 bites at the first two steps only (norms 1.26, 1.02, 0.79, 0.56), so a
    wrong coefficient changes the relative weight of the steps in Adam's moments, which a uniformly wrong one hardly does."""
    n_steps = 4
    out = str(tmp_path / 'clip.npz')
    rendezvous = 'file://' + str(tmp_path / 'rendezvous')
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MG_TEST_RENDEZVOUS=rendezvous, OMP_NUM_THREADS='1')
        procs.append(subprocess.Popen([sys.executable, os.path.join(REPO, 'tests', '_dist_clip_worker.py'), out, str(n_steps), str(max_norm)],
                                      env=env, cwd=REPO))
    for p in procs:
        assert p.wait(timeout=240) == 0
    got = np.load(out)
    want_flat, want_norms = _single_process_clipped(n_steps, max_norm)
    if max_norm == 0.05:
        assert min(want_norms) > 2 * max_norm                       # bites at every step, by a margin a factor of 2 would show
    else:
        assert want_norms[0] > max_norm > want_norms[-1] and 2 * want_norms[-1] > max_norm
    assert np.array_equal(got['replicas'][0], got['replicas'][1])   # both ranks arrived at the same coefficient
    np.testing.assert_allclose(got['norms'][:, 0], want_norms, rtol=1e-4)
    np.testing.assert_allclose(got['flat'], want_flat, rtol=1e-4, atol=1e-6)
