"""Write-through stores of the phone-rate step's launches (csrc/common.h: mg_wt_mask, mg_store_wt) against plain write-back stores
(MG_TUNE_AB = 85): the cache policy of a store changes no byte, so every output of every launch is EQUAL bit for bit
(``-m gpu``, MI355X).  Each test runs one call twice - the default form, then with mg_set_tuning(7, 85) - on a few thousand
table rows: 4 864 (whole tiles) and 5 003 (no multiple of 32, 192 or 256: the partial last tile, where the sink-row stores and
the row guards decide what is written)."""
import numpy as np
import pytest
import torch

import morgana_amd.functional as F_hip
from morgana_amd import _lib, data, graphs, models, ops, optim, synthetic

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ROWS = (4864, 5003)
BETAS, EPS_ADAM, LR = (0.9, 0.999), 1e-8, 0.01
NAN_BITS = 0x7fc1
GUARD = 8


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def both_forms(call):
    """call() in the default form and with plain stores everywhere; every tensor of a result is cloned (workspaces are reused)."""
    lib = _lib.load()

    def keep(x):
        if torch.is_tensor(x):
            return x.clone()
        if isinstance(x, (tuple, list)):
            return tuple(keep(v) for v in x)
        return x

    got = keep(call())
    _lib.check(lib.mg_set_tuning(7, 85), 'mg_set_tuning')
    try:
        want = keep(call())
    finally:
        _lib.check(lib.mg_set_tuning(7, 0), 'mg_set_tuning')
    torch.cuda.synchronize()
    return got, want


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


def _layer1(m, seed):
    rng = np.random.RandomState(seed)
    k, n = 600, 512
    a = ops.cast_pad_bf16(dev(rng.uniform(0, 1, (m, k)).astype(np.float32)))
    (w_bf,), _ = ops.cast_params_bf16([dev(rng.uniform(-0.1, 0.1, (n, k)).astype(np.float32))], want_plain=True, want_t=())
    bias = dev(rng.uniform(-0.1, 0.1, n).astype(np.float32))
    return a, k, w_bf, bias, n


@pytest.mark.parametrize('m', ROWS)
def test_layer1_forward(m):
    """ops.phone_front with the first layer in its grid (phone_front_gemm_kernel: H1 written through) and ops.linear_fwd_bf16 (the GEMM
    as a launch of its own keeps plain stores in both forms: that half only holds the two launches against each other)."""
    a, k, w_bf, bias, n = _layer1(m, m)
    rng = np.random.RandomState(m + 1)
    b, p, t, extra = 48, 80, 200, ops.PHONE_RATE_EXTRA
    dur = dev(rng.randint(1, 5, size=(b, p)).astype(np.int64))
    seq = dev(np.minimum(dur.sum(1).cpu().numpy(), t).astype(np.int64))
    target = dev(rng.standard_normal(b * t).astype(np.float32))
    assert ops.phone_front_ok(b, p, t, extra)
    got, want = both_forms(lambda: ops.phone_front(dur, target, seq, t, extra, linear=(a, k, w_bf, bias, n, ops.ACT_SIGMOID)))
    assert len(got) == len(want) == 7
    for i in (0, 1, 2, 3, 4, 6):                    # rows, mapped rows, segments, ybar, weight, H1 (5 is the workspace: scratch behind the partials)
        assert bits_equal(got[i], want[i]), i
    r = b * p
    n_partial = (r + 15) // 16 + extra // 4
    assert bits_equal(got[5].view(torch.float32)[:n_partial], want[5].view(torch.float32)[:n_partial])
    assert got[6].shape == (m, n) and bool(got[6].float().abs().sum() > 0)
    y, y_plain = both_forms(lambda: ops.linear_fwd_bf16(a, None, m, k, w_bf, bias, n, ops.ACT_SIGMOID))
    assert bits_equal(y, y_plain) and bits_equal(y, got[6])


def _slabs_equal(got, want, used):
    (gs, g_n, g_st), (ws, w_n, w_st) = got, want
    assert (g_n, g_st) == (w_n, w_st) and g_n > 0
    gs, ws = gs.view(torch.float32), ws.view(torch.float32)
    for i in range(g_n):
        assert torch.equal(gs[i * g_st:i * g_st + used].view(torch.int32), ws[i * w_st:i * w_st + used].view(torch.int32)), i


@pytest.mark.parametrize('m', ROWS)
def test_layer1_weight_gradient_slabs(m):
    """ops.linear_wgrad_slabs_bf16 at (m, 512, 600) with a 640-wide operand (wgrad_big_kernel<5>): every slab over its n k + n floats.
    PLACEHOLDER: this launch did not gain from write-through stores and carries no switch, so both runs are the same code; the case
    stays for the day the staged 16-byte slab epilogue is tried."""
    n, k, lda = 512, 600, 640
    rng = np.random.RandomState(m + 2)
    dy = ops.cast_pad_bf16(dev((rng.standard_normal((m, n)) * 0.05).astype(np.float32)))
    a = torch.zeros((m, lda), dtype=torch.bfloat16, device=DEV)
    a[:, :k] = dev(rng.uniform(-1, 1, (m, k)).astype(np.float32)).to(torch.bfloat16)
    got, want = both_forms(lambda: ops.linear_wgrad_slabs_bf16(dy, a, None, m, n, k))
    _slabs_equal(got, want, n * k + n)


@pytest.mark.parametrize('m', ROWS)
def test_wgrad_dgrad_pair(m):
    """ops.linear_wgrad_dgrad_bf16 (128 <-> 512): dX and the slabs of the shared grid."""
    n, k = 128, 512
    rng = np.random.RandomState(m + 3)
    (_,), (wt,) = ops.cast_params_bf16([dev(rng.uniform(-0.1, 0.1, (n, k)).astype(np.float32))], want_plain=True, want_t=(0,))
    h = ops.cast_pad_bf16(dev(rng.uniform(0.05, 0.95, (m, k)).astype(np.float32)))
    dy = ops.cast_pad_bf16(dev((rng.standard_normal((m, n)) * 0.01).astype(np.float32)))
    got, want = both_forms(lambda: ops.linear_wgrad_dgrad_bf16(dy, h, m, n, k, wt))
    _slabs_equal(got[:3], want[:3], n * k + n)
    assert bits_equal(got[3], want[3]) and bool(got[3].float().abs().sum() > 0)


def test_l2tail_rows():
    """ops.f0_l2tail_rows at 4 864 rows (one 32-row tile per wave): dZ2, the prediction, the loss and the gradient sums.
    PLACEHOLDER: the launch lost with write-through stores and carries no switch; both runs are the same code."""
    m = 4864
    rng = np.random.RandomState(11)
    h1 = ops.cast_pad_bf16(dev(rng.uniform(0.05, 0.95, (m, 512)).astype(np.float32)))
    (w2_bf,), _ = ops.cast_params_bf16([dev(rng.uniform(-0.08, 0.08, (128, 512)).astype(np.float32))])
    b2 = dev(rng.uniform(-0.1, 0.1, 128).astype(np.float32))
    w3, b3 = dev(rng.uniform(-0.2, 0.2, (32, 128)).astype(np.float32)), dev(rng.uniform(-0.1, 0.1, 32).astype(np.float32))
    w4, b4 = dev(rng.uniform(-0.3, 0.3, (1, 32)).astype(np.float32)), dev(rng.uniform(-0.1, 0.1, 1).astype(np.float32))
    ybar = dev(rng.standard_normal(m).astype(np.float32))
    weight = dev((rng.uniform(0, 1, m) * (rng.uniform(0, 1, m) > 0.1) / m).astype(np.float32))

    def call():
        grads = torch.full((32 * 128 + 32 + 32 + 1 + 1,), float('nan'), device=DEV)
        pred, loss, dz2 = ops.f0_l2tail_rows(h1, w2_bf, b2, w3, b3, w4, b4, ybar, weight, grads)
        return pred, loss, dz2, grads

    got, want = both_forms(call)
    for i, (g, w) in enumerate(zip(got, want)):
        assert bits_equal(g, w), i
    assert bool(torch.isfinite(got[3][:4162]).all()) and bool(got[2].float().abs().sum() > 0)


# ---- ops.adam_step_plan: the 'narrow_four_ragged' and 'shadows_wide' shapes of tests/test_gpu_adam_plan.py ----------------------------
_MIX = [(0, 24, 40, 'both'), (1000, 7, 9, 'dst'), (1100, 16, 8, 'dst_t'), (1300, 24, 40, 'pair'), (2300, 5, 13, 'pair_dst'),
        (2400, 12, 10, 'pair_t'), (2600, 3, 70, 'both'), (2900, 9, 9, 'both')]
ADAM_CASES = {
    'narrow_four_ragged': dict(n=1000, sources=[(0, 201, 2, 204), (201, 238, 15, 240), (439, 163, 16, 164), (602, 298, 17, 300)],
                               shadows=[(201, 14, 17, 'both'), (602, 10, 29, 'pair'), (900, 10, 10, 'dst')]),
    'shadows_wide': dict(n=4000, sources=[(0, 1000, 5, 1000), (3100, 300, 3, 300)], shadows=_MIX),
}


def _sentinel_buffer(rows, ld):
    whole = torch.full((GUARD + rows * ld + GUARD,), NAN_BITS, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    return whole, whole[GUARD:GUARD + rows * ld].view(rows, ld)


def _adam_run(spec, seed):
    n = spec['n']
    rng = np.random.RandomState(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 0.1).astype(np.float32)
    m = (rng.standard_normal(n) * 0.01).astype(np.float32)
    v = rng.uniform(1e-4, 1e-2, n).astype(np.float32)
    sources, wholes = [], []
    for begin, count, n_slabs, stride in spec['sources']:
        view = dev((rng.standard_normal((n_slabs, stride)) * 0.05).astype(np.float32))
        sources.append((begin, count, view, n_slabs, stride))
    entries = []
    for offset, rows, cols, kind in spec['shadows']:
        pair = kind.startswith('pair')
        ldd, ldt = ops.pad_ld(cols) * (2 if pair else 1), ops.pad_ld(rows) * (2 if pair else 1)
        d = _sentinel_buffer(rows, ldd) if kind in ('both', 'dst', 'pair', 'pair_dst') else None
        t = _sentinel_buffer(cols, ldt) if kind in ('both', 'dst_t', 'pair', 'pair_t') else None
        entries.append((offset, rows, cols, d[1] if d else None, t[1] if t else None, pair))
        wholes += [x[0] for x in (d, t) if x is not None]
    bufs = [dev(x) for x in (p, g, m, v)]
    scalars = torch.tensor(ops.adam_scalars(LR, BETAS, 3), dtype=torch.float32, device=DEV)
    ops.adam_step_plan(bufs[0], bufs[1], bufs[2], bufs[3], BETAS, EPS_ADAM, 1e-2, scalars, 0.5, slab_srcs=sources, shadows=entries, clear_grad=True)
    return tuple(bufs) + tuple(w.view(torch.int16) for w in wholes)


@pytest.mark.parametrize('name', sorted(ADAM_CASES))
def test_adam_step_plan(name):
    """Parameters, moments, the cleared gradient and the bf16 copies with their sentinel padding and guard elements.
    PLACEHOLDER: the update kernel lost with write-through stores and carries no switch; both runs are the same code."""
    spec = ADAM_CASES[name]
    got, want = both_forms(lambda: _adam_run(spec, seed=len(name) + spec['n']))
    assert len(got) == len(want) > 4
    for i, (g, w) in enumerate(zip(got, want)):
        assert bits_equal(g, w), (name, i)
    assert not bool(got[1].any())
    assert any(bool((w == NAN_BITS).any()) and bool((w != NAN_BITS).any()) for w in got[4:])      # copies written, padding kept


def test_graphed_train_step():
    """Three replays of graphs.GraphedTrainStep on a (128, 400) batch - 4 096 + 1 024 table rows, the phone-rate step (a (96, 200)
    batch has 1 536 table rows, under the 2 048 from which ops.phone_rate_table_ok takes that step): losses, prediction and the
    optimiser's flat buffers."""
    feats = data.to_device(synthetic.make_batch(128, 400, seed=9), DEV)
    data.add_bf16_table(feats)

    def run():
        model = models.F0Model(precision='bf16').to(DEV)
        own = model.state_dict()
        for key, value in synthetic.f0_model_state().items():
            own[key].copy_(torch.from_numpy(value))
        opt = optim.Adam(model.parameters(), lr=0.01, fused_loop=True)
        _lib.CALL_LOG = []
        try:
            step = graphs.GraphedTrainStep(model, opt, feats, warmup=2)
            log = list(_lib.CALL_LOG)
        finally:
            _lib.CALL_LOG = None
        losses = torch.stack([step().clone().reshape(()) for _ in range(3)])
        pred = next(iter(step.output.values())) if isinstance(step.output, dict) else step.output
        flat = opt.flat_buffers()
        return (losses, pred.clone()) + tuple(flat[k].clone() for k in sorted(flat) if torch.is_tensor(flat[k])), log

    lib = _lib.load()
    got, log = run()
    assert 'mg_phone_front_linear_fwd_bf16' in log and 'mg_linear_wgrad_dgrad_bf16' in log, 'the phone-rate step must engage'
    _lib.check(lib.mg_set_tuning(7, 85), 'mg_set_tuning')
    try:
        want, _ = run()
    finally:
        _lib.check(lib.mg_set_tuning(7, 0), 'mg_set_tuning')
    assert len(got) == len(want) >= 5
    for i, (g, w) in enumerate(zip(got, want)):
        assert bits_equal(g, w), i
    assert bool(torch.isfinite(got[0]).all())


@pytest.mark.parametrize('m', ROWS)
def test_pair_plane_layer1_forward(m):
    """bf16x3: ops.phone_front_x3 with the front in its grid (phone_front_gemm_kernel on pair planes: both planes of H1 written
    through) - the front's results and the [hi | lo] pair of H1."""
    rng = np.random.RandomState(m + 5)
    k, n = 600, 512
    a = ops.split_pair(dev(rng.uniform(0, 1, (m, k)).astype(np.float32)))
    w = ops.split_pair(dev(rng.uniform(-0.1, 0.1, (n, k)).astype(np.float32)))
    bias = dev(rng.uniform(-0.1, 0.1, n).astype(np.float32))
    b, p, t, extra = 48, 80, 200, ops.PHONE_RATE_EXTRA
    dur = dev(rng.randint(1, 5, size=(b, p)).astype(np.int64))
    seq = dev(np.minimum(dur.sum(1).cpu().numpy(), t).astype(np.int64))
    target = dev(rng.standard_normal(b * t).astype(np.float32))
    got, want = both_forms(lambda: ops.phone_front_x3((dur, target, seq, t, extra), (a, k, w, bias, n, ops.ACT_SIGMOID)))
    assert len(got) == len(want) == 7
    for i in (0, 1, 2, 3, 4, 6):
        assert bits_equal(got[i], want[i]), i
    assert got[6].shape == (m, 2 * n) and bool(got[6][:, :n].float().abs().sum() > 0) and bool(got[6][:, n:].float().abs().sum() > 0)


@pytest.mark.parametrize('m', ROWS)
def test_pair_plane_wgrad_dgrad_pair(m):
    """bf16x3: ops.linear_wgrad_dgrad_x3 (the shared grid on pair planes): the slabs, the dZ1 pair and the column sums."""
    n, k = 128, 512
    rng = np.random.RandomState(m + 6)
    h1p = ops.split_pair(dev((rng.rand(m, k) * 0.8 + 0.1).astype(np.float32)))
    dz2p = ops.split_pair(dev((rng.standard_normal((m, n)) * 1e-3).astype(np.float32)))
    w2tp = ops.split_pair(dev((rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)), transpose=True)
    got, want = both_forms(lambda: ops.linear_wgrad_dgrad_x3(dz2p, h1p, m, n, k, w2tp))
    _slabs_equal(got[:3], want[:3], n * k)
    assert bits_equal(got[3], want[3]) and bool(got[3].float().abs().sum() > 0)
    assert got[5] == want[5] > 0
    assert bits_equal(got[4].view(torch.float32)[:got[5] * k], want[4].view(torch.float32)[:want[5] * k])
