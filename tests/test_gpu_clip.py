"""Global gradient-norm clipping on the HIP path (csrc/clip.hip: mg_grad_sumsq_f32 + mg_grad_clip_scale_f32, optim.Adam(max_grad_norm=)):
the two kernels against the float64 restatement (tests/clip_ref64.py) inside a derived bound, special inputs, the optimiser against
clip_grad_norm_ + torch.optim.Adam in float64, and a whole training step - against a float64 torch model, against the unclipped
step, through the step cache (which keeps clipped steps on ordinary launches) and behind a world-1 RCCL exchange.

The bound on the norm: the kernel accumulates exact squares in float64 (error a few 2^-53 n, far below one fp32 rounding) and rounds
sqrt(sum) once to fp32, so |norm - fp32(norm64)| <= 2^-23 norm64 allows one fp32 rounding of the final value on either side.  The
coefficient is formed from the float64 norm and rounded once; against clip_ref64 evaluated on the REPORTED (fp32-rounded) norm that
is the same one-rounding bound.  The scaled buffer is a single fp32 multiply: bit-equal to float32(before) * float32(coef)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import clip_ref64
from morgana_amd import data, graphs, models, ops, optim, synthetic, utils
from morgana_amd import functional as F_hip
from oracle import ref_torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ONE_ROUNDING = 2.0 ** -23
RTOL = 1e-4                                   # the project's fp32 parity figure
_CHUNK = 4096                                 # chunk of every buffer below 4 Mi floats (mg_grad_clip_chunk; asserted in the sweep)
_EDGE = 3 * _CHUNK                            # chunk * blocks at three workgroups
SIZES = (1, 3, 255, 256, 257, 4099, _EDGE - 1, _EDGE + 1, 1000003)


def _clip(buffers, max_norm, inv_world=1.0):
    """Both launches over device ``buffers`` (in place) -> (norm, coef) as reported, float32, and the partials."""
    blocks = [ops.grad_clip_blocks(b.numel())[1] for b in buffers]
    partials = torch.full((sum(blocks),), -1.0, dtype=torch.float64, device=DEV)
    out = torch.full((2,), -1.0, dtype=torch.float32, device=DEV)
    off = 0
    for b, nb in zip(buffers, blocks):
        ops.grad_sumsq(b, partials, off)
        off += nb
    for i, b in enumerate(buffers):
        ops.grad_clip_scale(b, partials, inv_world, max_norm, out if i == 0 else None)
    norm, coef = out.cpu().numpy()
    return norm, coef, partials.cpu().numpy()


def _view(values, lead):
    """``values`` on the device as a view that starts ``lead`` floats into a larger allocation, guard values on both sides."""
    n = values.size
    whole = torch.full((lead + n + 5,), 7.0, dtype=torch.float32, device=DEV)
    whole[lead:lead + n] = torch.from_numpy(values)
    return whole, whole[lead:lead + n]


def _check(values_list, max_norm, leads=None, inv_world=1.0):
    """Norm, coefficient and scaled buffers of one clip over ``values_list`` against clip_ref64 and the bounds of the module docstring."""
    leads = leads or [0] * len(values_list)
    held = [_view(v, lead) for v, lead in zip(values_list, leads)]
    norm, coef, _ = _clip([h[1] for h in held], max_norm, inv_world)
    want_norm = clip_ref64.norm64(*values_list) * inv_world
    print('n=%s leads=%s: norm %.9g (float64 %.17g, err / bound %.3f), coef %.9g' % (
        [v.size for v in values_list], leads, norm, want_norm, abs(float(norm) - float(np.float32(want_norm))) / (ONE_ROUNDING * want_norm), coef))
    assert abs(float(norm) - float(np.float32(want_norm))) <= ONE_ROUNDING * want_norm
    want_coef = clip_ref64.coef(float(norm), max_norm)                   # on the kernel's own reported (mean) norm
    assert abs(float(coef) - float(np.float32(want_coef))) <= ONE_ROUNDING * want_coef
    for (whole, view), v, lead in zip(held, values_list, leads):
        got = whole.cpu().numpy()
        np.testing.assert_array_equal(got[lead:lead + v.size], v * np.float32(coef))       # one fp32 multiply: bit-equal
        assert (got[:lead] == 7.0).all() and (got[lead + v.size:] == 7.0).all()           # nothing outside the view was touched
    return norm, coef


@pytest.mark.parametrize('n', SIZES)
def test_kernels_against_float64_inside_one_rounding(n):
    """Vector tail, a single element, workgroup and chunk edges; the buffer at a 16-byte boundary and 4 / 12 bytes behind one."""
    assert ops.grad_clip_blocks(n)[0] == _CHUNK and ops.grad_clip_blocks(_EDGE) == (_CHUNK, 3)
    values = np.random.RandomState(n).standard_normal(n).astype(np.float32)
    max_norm = 0.5 * clip_ref64.norm64(values)                           # bites: coef about 0.5
    for lead in (0, 1, 3):
        norm, coef = _check([values], max_norm, [lead])
        assert 0.49 < coef < 0.51


def test_chunks_above_the_minimum():
    """Past 4 Mi floats the chunk grows (5120 floats at 4 Mi + 1, 820 workgroups): the other grid path, at a misaligned start."""
    n = 4096 * 1024 + 1
    assert ops.grad_clip_blocks(n) == (5120, 820)
    values = np.random.RandomState(7).standard_normal(n).astype(np.float32)
    _check([values], 100.0, [1])


def test_values_whose_squares_overflow_float32():
    values = (np.random.RandomState(1).choice([-1.0, 1.0], size=5001) * 1e19).astype(np.float32)
    norm, coef = _check([values], 1.0)
    assert np.isfinite(norm) and norm > 1e20 and 0.0 < coef < 1e-20


def test_all_zero_gradient_is_left_alone():
    values = np.zeros(4099, np.float32)
    values[5] = -0.0
    whole, view = _view(values, 1)
    norm, coef, _ = _clip([view], 0.25)
    assert norm == 0.0 and coef == 1.0
    got = whole.cpu().numpy()[1:1 + 4099]
    assert not got.any() and np.signbit(got[5]) and not np.signbit(got[4])


def test_norm_just_under_and_just_over_the_threshold():
    values = np.random.RandomState(3).standard_normal(4099).astype(np.float32)
    n64 = clip_ref64.norm64(values)
    buf = torch.from_numpy(values).to(DEV)
    norm, coef, _ = _clip([buf], n64 * (1.0 + 2.0 ** -20) + 2e-6)       # under: the coefficient is exactly 1 and nothing moves
    assert coef == 1.0 and np.array_equal(buf.cpu().numpy(), values)
    norm, coef = _check([values], n64 * (1.0 - 2.0 ** -20))             # over, by less than torch's own fp32 norm could tell
    assert coef < 1.0 and coef >= np.float32(1.0 - 2.0 ** -19)


def test_one_inf_gives_coefficient_zero():
    values = np.random.RandomState(4).standard_normal(4099).astype(np.float32)
    values[1234] = np.inf
    buf = torch.from_numpy(values).to(DEV)
    norm, coef, _ = _clip([buf], 1.0)
    assert np.isposinf(norm) and coef == 0.0
    with np.errstate(invalid='ignore'):
        want = values * np.float32(0.0)                                 # zeros with the signs kept, NaN where the inf was: as torch
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    finite = np.arange(values.size) != 1234                             # (the sign of a NaN is nobody's promise)
    assert np.array_equal(np.signbit(got[finite]), np.signbit(want[finite])) and np.isnan(got[1234]) and np.isnan(got).sum() == 1


def test_one_nan_gives_nan_gradients():
    values = np.random.RandomState(5).standard_normal(4099).astype(np.float32)
    values[4098] = np.nan                                               # in the scalar tail
    buf = torch.from_numpy(values).to(DEV)
    norm, coef, _ = _clip([buf], 1.0)
    assert np.isnan(norm) and np.isnan(coef)
    assert np.isnan(buf.cpu().numpy()).all()                            # NaN != 1: the scale launch still writes


def test_two_groups_share_one_norm():
    rng = np.random.RandomState(6)
    a, b = rng.standard_normal(5000).astype(np.float32), (rng.standard_normal(13) * 30.0).astype(np.float32)
    norm, coef = _check([a, b], 2.0, [0, 3])
    assert norm > clip_ref64.norm64(a) and norm > clip_ref64.norm64(b)
    # 1 / world scales the norm, not the buffer: a sum over 4 ranks whose mean is under the threshold is left alone
    both = clip_ref64.norm64(a, b)
    _, coef = _check([a, b], 0.3 * both, inv_world=0.25)
    assert coef == 1.0
    _, coef = _check([a, b], 0.2 * both, inv_world=0.25)
    assert 0.79 < coef < 0.81


def test_two_runs_are_bit_equal():
    values = np.random.RandomState(8).standard_normal(1000003).astype(np.float32)
    runs = []
    for _ in range(2):
        buf = torch.from_numpy(values).to(DEV)
        norm, coef, partials = _clip([buf], 10.0)
        runs.append((np.float32(norm).tobytes(), np.float32(coef).tobytes(), partials.tobytes(), buf.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------------------------ optimiser
def test_optimiser_against_torch_in_float64():
    """Five steps of fixed gradients, two parameter groups, the threshold taken on both sides: parameters against clip_grad_norm_ +
    torch.optim.Adam on CPU float64 (the tolerance of test_gpu_parity.test_adam_and_ema_vs_oracle), ``grad_norms()`` against the
    float64 norm of each step's gradient."""
    rng = np.random.RandomState(0)
    shapes = [(10007,), (33, 7), (5,)]
    init = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    ours = [nn.Parameter(torch.from_numpy(a.copy()).to(DEV)) for a in init]
    ref = [nn.Parameter(torch.from_numpy(a.astype(np.float64))) for a in init]
    groups = lambda ps: [{'params': ps[:1]}, {'params': ps[1:], 'lr': 0.003}]
    opt = optim.Adam(groups(ours), lr=0.01, weight_decay=1e-2, max_grad_norm=1.0)
    opt_ref = torch.optim.Adam(groups(ref), lr=0.01, weight_decay=1e-2)
    bitten = []
    for scale in (3.0, 1e-4, 40.0, 1e-3, 0.7):
        grads = [(rng.standard_normal(s) * scale).astype(np.float32) for s in shapes]
        opt.zero_grad()
        for p, q, g in zip(ours, ref, grads):
            p.grad.copy_(torch.from_numpy(g))
            q.grad = torch.from_numpy(g.astype(np.float64))
        torch.nn.utils.clip_grad_norm_(ref, 1.0)
        opt_ref.step()
        opt.step()
        norm, coef = opt.grad_norms()[0].cpu().numpy()
        want = clip_ref64.norm64(*grads)
        assert abs(float(norm) - float(np.float32(want))) <= ONE_ROUNDING * want
        assert abs(float(coef) - float(np.float32(clip_ref64.coef(float(norm), 1.0)))) <= ONE_ROUNDING * clip_ref64.coef(float(norm), 1.0)
        bitten.append(coef < 1.0)
    assert bitten == [True, False, True, False, True]
    for p, q in zip(ours, ref):
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().numpy(), rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------------------------------------------------ whole step
DIMS = dict(lab=20, counters=4, d1=24, hid=16, post=16, out=3)       # the layer widths of golden G13
N_STEPS = 5


class _TinyGRUF0(models.StreamModel):
    """models.GRUF0Model's stack and stream table on small widths (the class itself fixes 256 / 64 / 64)."""

    def __init__(self):
        d = DIMS
        gru = lambda n_in: utils.RecurrentCuDNNWrapper(nn.GRU(n_in, d['hid'], batch_first=True), precision='fp32')
        layers = utils.SequentialWithRecurrent(
            nn.Linear(d['lab'] + d['counters'], d['d1']), nn.Sigmoid(), nn.Dropout(p=0.),
            gru(d['d1']), nn.Dropout(p=0.), gru(d['hid']), nn.Dropout(p=0.), gru(d['hid']), nn.Dropout(p=0.),
            nn.Linear(d['hid'], d['post']), nn.Sigmoid(), nn.Dropout(p=0.), nn.Linear(d['post'], d['out']), precision='fp32')
        from morgana_amd import metrics
        streams = [models.Stream('lf0', d['out'], 'mse', ('LF0_RMSE_Hz', metrics.LF0Distortion, 'voiced_trajectory'))]
        models.StreamModel.__init__(self, layers, streams, fused_upsample=True, fused_loss=False, generate=False)


class _Float64GRUF0(nn.Module):
    """The same stack in plain torch on the CPU, float64, with the reference's wrapper, upsampling and masked MSE (oracle/ref_torch.py);
    same state_dict keys."""

    def __init__(self):
        super().__init__()
        d = DIMS
        gru = lambda n_in: ref_torch.GRUWrapper(nn.GRU(n_in, d['hid'], batch_first=True))
        self.layers = nn.ModuleList([
            nn.Linear(d['lab'] + d['counters'], d['d1']), nn.Sigmoid(), nn.Identity(), gru(d['d1']), nn.Identity(), gru(d['hid']),
            nn.Identity(), gru(d['hid']), nn.Identity(), nn.Linear(d['hid'], d['post']), nn.Sigmoid(), nn.Identity(),
            nn.Linear(d['post'], d['out'])])

    def forward(self, feats):
        n_frames = feats['n_frames']
        x = torch.cat((ref_torch.upsample_to_repetitions(feats['normalised_lab'], feats['dur']), feats['normalised_counters']), dim=-1)
        x = self.layers[1](self.layers[0](x))
        for idx in (3, 5, 7):
            x, _ = self.layers[idx](x, n_frames)
        pred = self.layers[12](self.layers[10](self.layers[9](x)))
        return ref_torch.mse(pred, feats['normalised_lf0_deltas'], n_frames)


def _state():
    d = DIMS
    return synthetic.gru_f0_state(seed=2121, input_dim=d['lab'] + d['counters'], d1=d['d1'], hidden=d['hid'], post=d['post'],
                                  output_dim=d['out'])


def _batch_np():
    """B = 4, T = 37, ragged: the first seed whose longest utterance has 37 frames and whose shortest is shorter."""
    for seed in range(100):
        feats = synthetic.make_acoustic_batch(4, (11, 37), lab_dim=DIMS['lab'], counters_dim=DIMS['counters'], streams=(('lf0', DIMS['out'], 'mse'),),
                                              frames_per_phone=5.0, seed=seed)
        if feats['n_frames'].max() == 37 and feats['n_frames'].min() < 30:
            return feats
    raise AssertionError('no seed gives T = 37')


def _fresh(max_grad_norm, **kw):
    model = _TinyGRUF0().to(DEV)
    own = model.state_dict()
    for key, value in _state().items():
        own[key].copy_(torch.from_numpy(value))
    return model, optim.Adam(model.parameters(), lr=0.01, fused_loop=True, max_grad_norm=max_grad_norm, **kw)


def _eager_run(max_grad_norm, feats, **kw):
    """N_STEPS of the fused loop as ordinary launches -> (losses, flat buffers, per-step (norm, coef))."""
    model, opt = _fresh(max_grad_norm, **kw)
    losses, norms = [], []
    for _ in range(N_STEPS):
        opt.zero_grad()
        loss, _ = model(feats)
        F_hip.backward(loss)
        opt.step()
        losses.append(loss.item())
        if max_grad_norm is not None:
            norms.append(opt.grad_norms()[0].cpu().numpy().copy())
    flat = opt.flat_buffers()
    return losses, {k: flat[k].clone() for k in ('param', 'exp_avg', 'exp_avg_sq')}, norms


_SHARED = {}


def _shared():
    """Computed once for the whole-step tests and left unchanged: the batch, the first gradient's norm (which sets a threshold that
    bites at every step), the eager clipped run and the float64 torch run with the same clipping."""
    if not _SHARED:
        feats_np = _batch_np()
        feats = data.to_device(feats_np, DEV)
        ref = ref_torch.load_state(_Float64GRUF0().double(), {k: v.astype(np.float64) for k, v in _state().items()})
        feats64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in ref_torch.to_torch(feats_np).items() if isinstance(v, torch.Tensor)}
        loss = ref(feats64)
        loss.backward()
        first_norm = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), 1e30))
        ref.zero_grad()
        threshold = 0.02 * first_norm                                    # the loss falls slowly over five steps: this bites at all of them
        opt_ref = torch.optim.Adam(ref.parameters(), lr=0.01)
        ref_losses, ref_norms = [], []
        for _ in range(N_STEPS):
            opt_ref.zero_grad()
            loss = ref(feats64)
            loss.backward()
            ref_norms.append(float(torch.nn.utils.clip_grad_norm_(ref.parameters(), threshold)))
            opt_ref.step()
            ref_losses.append(loss.item())
        _SHARED.update(feats=feats, threshold=threshold, ref_losses=ref_losses, ref_norms=ref_norms, eager=_eager_run(threshold, feats))
    return _SHARED


def test_whole_step_against_float64_torch():
    """Five clipped steps of the fused loop against the float64 torch model under clip_grad_norm_ + torch.optim.Adam: the loss curve
    (whose later points are functions of the clipped updates before them) and each step's pre-clip norm at the fp32 parity figure -
    the norm is, like the loss, a sum over every frame and element of fp32-rounded terms, so it carries the same figure.  Parameters
    are not compared element by element: Adam's update lr m / (sqrt(v) + eps) turns the fp32 rounding of a gradient element near
    zero into a change of up to lr per step, which no relative figure bounds; their effect is in the loss curve."""
    s = _shared()
    losses, flat, norms = s['eager']
    assert min(s['ref_norms']) > 2 * s['threshold']                      # the threshold bit at every step
    print('losses', losses, 'float64', s['ref_losses'], 'norms', [float(n[0]) for n in norms], 'float64', s['ref_norms'])
    np.testing.assert_allclose(losses, s['ref_losses'], rtol=RTOL)
    np.testing.assert_allclose([n[0] for n in norms], s['ref_norms'], rtol=RTOL)
    for n, want in zip(norms, s['ref_norms']):
        assert abs(float(n[1]) - clip_ref64.coef(float(n[0]), s['threshold'])) <= ONE_ROUNDING


def test_step_cache_keeps_clipped_steps_on_ordinary_launches():
    """A clipped step is not captured into a HIP graph: ``GraphedTrainStep`` refuses it before any capture begins, and
    ``GraphedStepCache`` (``ExperimentBuilder(use_graphs=True)``) then runs every such step as ordinary launches - the same five steps as
    the eager loop, bit for bit, one warning."""
    import warnings
    s = _shared()
    losses_e, flat_e, _ = s['eager']
    model, opt = _fresh(s['threshold'])
    with pytest.raises(RuntimeError, match='not captured'):
        graphs.GraphedTrainStep(model, opt, s['feats'], warmup=0)
    cache = graphs.GraphedStepCache(model, opt)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        losses_c = [cache.step(s['feats'])[0].item() for _ in range(N_STEPS)]
    assert losses_c == losses_e
    assert cache.stats()['eager'] == N_STEPS and cache.stats()['replayed'] == 0 and cache.stats()['graphs'] == 0
    assert len([w for w in caught if 'cannot be captured' in str(w.message)]) == 1
    for key in ('param', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(opt.flat_buffers()[key], flat_e[key]), key


def test_threshold_that_never_bites_equals_no_clipping():
    """max_grad_norm=1e30 against None: the coefficient is exactly 1 and the gradient is not written, so the two runs differ only in
    where split-M slabs are summed (clipping declines the deferral) - loss curves within the fp32 parity figure."""
    s = _shared()
    loose, flat_l, norms = _eager_run(1e30, s['feats'])
    plain, flat_p, _ = _eager_run(None, s['feats'])
    assert all(float(n[1]) == 1.0 and float(n[0]) > 0.0 for n in norms)
    np.testing.assert_allclose(loose, plain, rtol=RTOL)
    assert float((flat_l['param'] - flat_p['param']).abs().max() / flat_p['param'].abs().max()) < RTOL


def test_clip_follows_the_exchange_on_a_world1_rccl_group(tmp_path):
    """exchange_always=True on a world-1 RCCL group (the all-reduce over one rank is the identity, 1 / world = 1): the clip runs
    behind the exchange in ``step``, and the results equal the run without a group."""
    import os
    import torch.distributed as dist
    s = _shared()
    losses_e, flat_e, norms_e = s['eager']
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    torch.cuda.set_device(0)
    dist.init_process_group(backend='nccl', init_method='file://' + str(tmp_path / 'rendezvous'), rank=0, world_size=1)
    try:
        model, opt = _fresh(s['threshold'], exchange_always=True)
        assert opt.exchanging()
        losses_m, flat_m, norms_m = _eager_run(s['threshold'], s['feats'], exchange_always=True)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert losses_m == losses_e
    assert np.array_equal(np.stack(norms_m), np.stack(norms_e))
    for key in ('param', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(flat_m[key], flat_e[key]), key
