"""The kernels of the bf16 phone-rate training step (bench.py C2: mg_phone_front_linear_fwd_bf16, mg_f0_l2tail_rows_slabs_bf16,
mg_linear_wgrad_dgrad[_expand]_bf16, mg_linear_wgrad_slabs_bf16; the update's plan kernel has tests/test_gpu_adam_plan.py) held to the
float64 restatement of tests/phone_step_ref64.py ELEMENT BY ELEMENT: every assertion is ratio(device, Bounded reference) <= 1
(``-m gpu``, MI355X).  Where the reference's bound is zero - ``exact`` operands, and every bf16 output that is not ambiguous - that
is bit equality with float64 arithmetic.  One launch per test, through morgana_amd.ops; the ``wide`` cases of the backward launches
take the DEVICE's own outputs of the launch before as operands (dZ2 from the layers 2-4 pass, dZ1 from the pair grid).

Shapes, and the launch arithmetic they come from:
* layers 2-4 pass, rows form: a wave takes a 32-row tile, 4 waves a workgroup, at most 256 workgroups (l2tail_blocks) - M = 1 (one
  lane live), 31 / 33 (ragged tile / a second wave), 129 (a second workgroup), 4127 (33 workgroups, ragged, the smallest rows the
  backward's slab kernels take), 32 805 (1026 tiles on 1024 waves: waves 0 and 1 of workgroup 0 take a SECOND tile, 32 768 + 37 rows,
  so the stores issued "at the top of the next iteration" and the ragged last tile both happen on a second trip).
* frames form: (B, T) = (7, 9365) = 65 555 rows >= 65 536 takes ``rev = 1`` (tiles walked from the end) with a ragged last tile; (3, 11).
* pair grid: mg_wgrad_big_plan + mg_launch_wgrad_dgrad_pair, restated in phone_step_ref64.pair_plan: m = 4096 -> 64 splits of 64 rows
  (all used), 4127 -> 72 splits of 64 rows (65 used, 7 EMPTY), 8209 -> 88 of 96 rows (86 used, 2 empty).  (The plan's 48 splits of 96
  rows are doubled to 96 for a one-tile-wide dY before the chunk is formed; the returned n_slabs is asserted against the restatement.)
* layer-1 weight gradient: (4127, 512, 600), (4097, 512, 640), (4127, 512, 609) -> the half-width plan wgrad_big_kernel<5>: 32 splits
  of 160 rows, 26 used, 6 EMPTY.  The last 1024 rows of A are zero (the table's extra rows) with nonzero dZ1: only db1 carries them.
Slab buffers are poisoned with NaN before the call: an empty split must WRITE its zeros.

If an ``exact`` case differed on every interior element, the suspect would be the assumption that the matrix cores keep 24
significant bits below the largest addend of an accumulate step (phone_step_ref64's docstring), not a kernel; a difference on some
elements only (an edge, a tile, a split) is a kernel defect."""
import functools

import numpy as np
import pytest
import torch

import phone_step_ref64 as ref
from morgana_amd import _lib, ops
from parity_report import note
from recurrent_ref64 import ratio

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32 = np.float32
N_TAIL = ref.N_TAIL                                   # 4161 gradients; the loss follows


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bf(x):
    """A host array of bf16 VALUES as a bf16 device tensor (the conversion is exact)."""
    return dev(np.asarray(x, dtype=F32)).to(torch.bfloat16)


def host(t):
    return t.float().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _held(got, want, label):
    """ratio(device, reference) <= 1, recorded; on failure says how many elements are out and where the first one is."""
    got = host(got).reshape(want.v.shape)
    r = note(ratio(got, want), label, bound=1.0)
    print('%-86s observed / bound = %.4g' % (label, r))
    if r > 1.0:
        bad = ~(np.abs(got.astype(np.float64) - want.v) <= want.e)
        first = tuple(int(i) for i in np.argwhere(bad)[0]) if bad.ndim else ()
        raise AssertionError('%s: observed / bound = %.4g; %d of %d elements out, first at %s: got %.9g want %.9g +- %.3g'
                             % (label, r, int(bad.sum()), bad.size, first, got[first], want.v[first], np.asarray(want.e)[first]))


def _shares(label, shares, capped=()):
    """Prints the reference's ambiguous shares; ``capped``: the ones an ``exact`` case promises to keep rare (the reference alone)."""
    for key in capped:
        assert shares[key] <= 1e-3, (label, key, shares[key])
    print('%-86s ambiguous shares: %s' % (label, ', '.join('%s %.2e' % kv for kv in sorted(shares.items()))))


def _tail_operands(c):
    return [dev(c[k]) for k in ('w3', 'b3', 'w4', 'b4', 'ybar', 'weight')]


def _check_tail(label, pred, loss, dz2, grads, want, exact=False):
    g = host(grads)
    _held(pred, want['pred'], label + ' pred')
    _held(loss.reshape(()), want['loss'], label + ' loss')
    _held(dz2[:, :128], want['dz2'], label + ' dZ2')
    _held(g[:4096], want['dw3'], label + ' dW3')
    _held(g[4096:4128], want['db3'], label + ' db3')
    _held(g[4128:4160], want['dw4'], label + ' dW4')
    _held(g[4160], want['db4'], label + ' db4')
    _shares(label, want['shares'], ('h2',) if exact else ())


# ------------------------------------------------------------------------------------------------------------ layers 2-4, rows form
@functools.lru_cache(maxsize=4)
def _l2_case(kind, m):
    return (ref.exact_l2tail if kind == 'exact' else ref.wide_l2tail)(m)


def _l2_ref(kind, m, gs):
    c = _l2_case(kind, m)
    return ref.l2tail_rows(c['h1'], c['w2'], c['b2'], c['w3'], c['b3'], c['w4'], c['b4'], c['ybar'], c['weight'], gs, exact=(kind == 'exact'))


L2_CASES = [(m, 1.0) for m in (1, 31, 33, 129, 4127, 32805)] + [(m, gs) for m in (33, 4127) for gs in ref.GRAD_SCALES[1:]]


@pytest.mark.parametrize('kind', ['exact', 'wide'])
@pytest.mark.parametrize('m,gs', L2_CASES)
def test_l2tail_rows(m, gs, kind):
    """ops.f0_l2tail_rows: pred, loss, dZ2, dW3, db3, dW4, db4 within the reference's bounds; a second run into a differently
    pre-filled gradient buffer (the first is pre-filled with NaN) is bit-equal."""
    c = _l2_case(kind, m)
    h1, w2, b2 = bf(c['h1']), bf(c['w2']), dev(c['b2'])
    tail = _tail_operands(c)
    grads = torch.full((N_TAIL + 1,), float('nan'), device=DEV)
    pred, loss, dz2 = ops.f0_l2tail_rows(h1, w2, b2, *tail, grads, grad_scale=gs)
    assert loss.data_ptr() == grads[N_TAIL:].data_ptr()
    _check_tail('l2tail_rows %s M=%d gs=%.3g' % (kind, m, gs), pred, loss, dz2, grads, _l2_ref(kind, m, gs), kind == 'exact')
    grads2 = torch.full_like(grads, 7.0)
    pred2, loss2, dz2_2 = ops.f0_l2tail_rows(h1, w2, b2, *tail, grads2, grad_scale=gs)
    assert torch.equal(pred, pred2) and torch.equal(dz2, dz2_2) and torch.equal(grads, grads2)


# ------------------------------------------------------------------------------------------------------------ layers 2-4, frames form
@pytest.mark.parametrize('b,t,kind,gs', [(7, 9365, 'exact', 1.0), (3, 11, 'exact', 1.0), (3, 11, 'wide', 0.125)])
def test_l2tail_frames(b, t, kind, gs):
    """ops.f0_l2tail (seq_len form): ragged lengths with one utterance of length 1 and one of full length; 65 555 rows walk the tiles
    from the end (rev = 1) with a ragged last tile.  Frames past an utterance's length have dZ2 == 0 exactly."""
    m = b * t
    c = (ref.exact_l2tail if kind == 'exact' else ref.wide_l2tail)(m, 7)
    rng = np.random.RandomState(b * t)
    sl = rng.randint(2, t + 1, size=b).astype(np.int64)
    sl[0], sl[1], sl[-1] = t, 1, t - 3
    grads = torch.full((N_TAIL + 1,), float('nan'), device=DEV)
    w3, b3, w4, b4, tgt, _ = _tail_operands(c)
    pred, loss, dz2 = ops.f0_l2tail(bf(c['h1']), bf(c['w2']), dev(c['b2']), w3, b3, w4, b4, tgt, dev(sl), b, t, grads, grad_scale=gs)
    want = ref.l2tail_frames(c['h1'], c['w2'], c['b2'], c['w3'], c['b3'], c['w4'], c['b4'], c['ybar'], sl, b, t, gs, exact=(kind == 'exact'))
    _check_tail('l2tail_frames %s (%d, %d) gs=%.3g' % (kind, b, t, gs), pred, loss, dz2, grads, want, kind == 'exact')
    dead = (np.arange(t)[None, :] >= sl[:, None]).reshape(-1)
    assert dead.any() and not host(dz2)[dead].any()


# ------------------------------------------------------------------------------------------------------------ the 128-wide tail
@pytest.mark.parametrize('m,gs', [(1, 1.0), (33, 1.0 / 3.0), (4127, 0.125)])
def test_tail_rows(m, gs):
    """ops.f0_tail_rows (tail_bf16.hip, the fallback of the fused pass) from the H2 it is given, against the same chain."""
    c = ref.tail_h2(m)
    grads = torch.full((N_TAIL + 1,), float('nan'), device=DEV)
    pred, loss, dz2 = ops.f0_tail_rows(bf(c['h2']), *_tail_operands(c), grads, grad_scale=gs)
    want = ref.tail_rows(c['h2'], c['w3'], c['b3'], c['w4'], c['b4'], c['ybar'], c['weight'], gs)
    _check_tail('tail_rows M=%d gs=%.3g' % (m, gs), pred, loss, dz2, grads, want)


# ------------------------------------------------------------------------------------------------------------ expansion, deferred forms
def test_expansion_and_deferred_forms():
    """M = 4127 rows (3103 table rows + 1024 extra), 5000 frames whose map reaches the extra rows.  f0_l2tail_rows_expand: the repeated
    prediction is pred[rows] exactly, the loss is the reference's plus the constant term within its bound, gradients and dZ2 bit-equal to
    f0_l2tail_rows.  defer=True finished by finish_deferred_tail, and as riders of linear_wgrad_dgrad_bf16(tail=...): bit-equal to
    the undeferred call, and the pair's own outputs bit-equal to the call without riders."""
    m, frames, gs = 4127, 5000, 1.0 / 3.0
    n_table, extra = m - 1024, 1024
    c = _l2_case('exact', m)
    rng = np.random.RandomState(5)
    rows_np = np.sort(np.concatenate([rng.randint(0, n_table, frames - 600), rng.randint(n_table, m, 598), [n_table, m - 1]])).astype(np.int32)
    partials_np = rng.uniform(0, 1e-3, (n_table + 15) // 16 + extra // 4).astype(F32)
    rows, partials = dev(rows_np), dev(partials_np)
    h1, w2, b2 = bf(c['h1']), bf(c['w2']), dev(c['b2'])
    tail_ops = _tail_operands(c)

    def fresh():
        return torch.full((N_TAIL + 1,), float('nan'), device=DEV)

    grads_u = fresh()
    pred_u, loss_u, dz2_u = ops.f0_l2tail_rows(h1, w2, b2, *tail_ops, grads_u, grad_scale=gs)
    want = _l2_ref('exact', m, gs)
    grads_x = fresh()
    got_pred, got_loss, dz2_x = ops.f0_l2tail_rows_expand(h1, w2, b2, *tail_ops, grads_x, rows, (partials, n_table, extra), grad_scale=gs)
    want_x = ref.expand_loss(host(pred_u), rows_np, want['loss'], partials_np)
    assert np.array_equal(host(got_pred), want_x['pred'])                         # the prediction, repeated: exact
    _held(got_loss.reshape(()), want_x['loss'], 'expand: loss + constant term')
    assert got_loss.item() != loss_u.item()
    assert torch.equal(dz2_x, dz2_u) and torch.equal(grads_x[:N_TAIL], grads_u[:N_TAIL])
    want_loss = got_loss.clone()
    # deferred, finished by its own launch
    grads_d = fresh()
    pred_d, _, dz2_d, tail = ops.f0_l2tail_rows_expand(h1, w2, b2, *tail_ops, grads_d, rows, (partials, n_table, extra), grad_scale=gs, defer=True)
    pred_d.fill_(float('nan'))
    assert torch.isnan(grads_d).all()
    ops.finish_deferred_tail(tail)
    assert torch.equal(pred_d, got_pred) and torch.equal(grads_d, grads_x) and torch.equal(dz2_d, dz2_u)
    # deferred, finished as riders of the pair grid
    wt = bf(np.ascontiguousarray(c['w2'].T))
    assert ops.wgrad_slabs_ok(m, 128, 512, 512, 128)
    slab_w, ns_w, st_w, dx_w = ops.linear_wgrad_dgrad_bf16(dz2_u, h1, m, 128, 512, wt)
    slab_w = slab_w.view(torch.float32)[:ns_w * st_w].clone()
    grads_r = fresh()
    pred_r, loss_r, dz2_r, tail = ops.f0_l2tail_rows_expand(h1, w2, b2, *tail_ops, grads_r, rows, (partials, n_table, extra), grad_scale=gs, defer=True)
    pred_r.fill_(float('nan'))
    slab_r, ns_r, st_r, dx_r = ops.linear_wgrad_dgrad_bf16(dz2_r, h1, m, 128, 512, wt, tail=tail)
    assert torch.equal(pred_r, got_pred) and torch.equal(grads_r, grads_x) and loss_r.item() == want_loss.item()
    assert (ns_r, st_r) == (ns_w, st_w) and torch.equal(dx_r, dx_w) and torch.equal(slab_r.view(torch.float32)[:ns_r * st_r], slab_w)


# ------------------------------------------------------------------------------------------------------------ pair grid
def _poisoned_slab(m, n, k):
    nbytes = int(_lib.load().mg_linear_wgrad_workspace_bytes(m, n, k))
    return torch.full(((nbytes + 3) // 4,), float('nan'), dtype=torch.float32, device=DEV).view(torch.uint8)


@functools.lru_cache(maxsize=4)
def _device_chain(m):
    """The device's own dZ2 (layers 2-4 pass) and dZ1 (pair grid) of the ``wide`` operands at m rows, with those operands."""
    c = _l2_case('wide', m)
    h1 = bf(c['h1'])
    grads = torch.empty((N_TAIL + 1,), device=DEV)
    _, _, dz2 = ops.f0_l2tail_rows(h1, bf(c['w2']), dev(c['b2']), *_tail_operands(c), grads)
    slab, n_slabs, stride, dz1 = ops.linear_wgrad_dgrad_bf16(dz2, h1, m, 128, 512, bf(np.ascontiguousarray(c['w2'].T)))
    return c, host(dz2), host(dz1)


@pytest.mark.parametrize('kind', ['exact', 'wide'])
@pytest.mark.parametrize('m', [4096, 4127, 8209])
def test_pair_grid(m, kind):
    """ops.linear_wgrad_dgrad_bf16: the fp32 sum of the slabs (ops.slab_reduce) against dW2 | db2 - EQUAL to float64 on exact operands
    - and dZ1 against bf16((dZ2 W2) H1 (1 - H1)), equal wherever it is not ambiguous.  n_slabs as the restated plan; the slabs of
    empty splits are zero although the buffer held NaN."""
    if kind == 'exact':
        c = ref.exact_pair(m)
        dz2_np, h1_np, w2_np = c['dz2'], c['h1'], c['w2']
    else:
        c, dz2_np, _ = _device_chain(m)
        h1_np, w2_np = c['h1'], c['w2']
    n, k = 128, 512
    assert ops.wgrad_slabs_ok(m, n, k, 512, 128)
    slab, n_slabs, stride, dz1 = ops.linear_wgrad_dgrad_bf16(bf(dz2_np), bf(h1_np), m, n, k, bf(np.ascontiguousarray(w2_np.T)), slab=_poisoned_slab(m, n, k))
    want_slabs, chunk = ref.pair_plan(m)
    assert n_slabs == want_slabs, (n_slabs, want_slabs)
    used = -(-m // chunk)
    slabs = slab.view(torch.float32)[:n_slabs * stride].view(n_slabs, stride)[:, :n * k + n]
    assert torch.isfinite(slabs).all() and not slabs[used:].any()
    assert {4096: 0, 4127: 7, 8209: 2}[m] == n_slabs - used
    total = ops.slab_reduce(slab, n_slabs, stride, n * k + n, torch.full((n * k + n,), float('nan'), device=DEV))
    want = ref.wgrad_dgrad(dz2_np, h1_np, w2_np.T, n_slabs, exact=(kind == 'exact'))
    label = 'pair grid %s m=%d (%d slabs of %d rows)' % (kind, m, n_slabs, chunk)
    _held(total, want['dwdb'], label + ' dW2 | db2')
    _held(dz1, want['dz1'], label + ' dZ1')
    _shares(label, want['shares'])


# ------------------------------------------------------------------------------------------------------------ layer-1 weight gradient
@pytest.mark.parametrize('kind', ['exact', 'wide'])
@pytest.mark.parametrize('m,n,k', [(4127, 512, 600), (4097, 512, 640), (4127, 512, 609)])
def test_layer1_wgrad(m, n, k, kind):
    """ops.linear_wgrad_slabs_bf16 + ops.slab_reduce (rows=None, a 640-wide operand with k columns in use; the half-width plan: 32
    splits, 6 of them empty) against dW1 | db1.  The last 1024 rows of A are zero, dZ1 is not: db1 must carry them."""
    if kind == 'exact':
        c = ref.exact_wgrad(m, n, k)
        dz1_np, a_np = c['dz1'], c['a']
    else:
        _, _, dz1_np = _device_chain(m)
        a_np = ref.wide_wgrad(m, n, k)['a']
    assert not a_np[m - 1024:].any() and dz1_np[m - 1024:].any()
    assert ops.wgrad_slabs_ok(m, n, k, 640, 512)
    slab, n_slabs, stride = ops.linear_wgrad_slabs_bf16(bf(dz1_np), bf(a_np), None, m, n, k, slab=_poisoned_slab(m, n, k))
    want_slabs, chunk = ref.wgrad_plan(m, n, k, 640)
    assert (n_slabs, want_slabs, chunk) == (32, 32, 160)
    slabs = slab.view(torch.float32)[:n_slabs * stride].view(n_slabs, stride)[:, :n * k + n]
    assert torch.isfinite(slabs).all() and not slabs[-(-m // chunk):].any()
    total = ops.slab_reduce(slab, n_slabs, stride, n * k + n, torch.full((n * k + n,), float('nan'), device=DEV))
    want = ref.wgrad(dz1_np, a_np, k, n_slabs, exact=(kind == 'exact'))
    _held(total, want['dwdb'], 'layer-1 wgrad %s (%d, %d, %d) dW1 | db1' % (kind, m, n, k))


# ------------------------------------------------------------------------------------------------------------ layer-1 forward
def test_layer1_forward_in_the_front_launch():
    """ops.phone_front(..., linear=...) at (4127, 600, 512), exact operands: H1 equals the reference's bf16 except at ambiguous elements."""
    b, p, t, extra = 29, 107, 700, 1024
    m, k, n = b * p + extra, 600, 512
    assert m == 4127
    rng = np.random.RandomState(17)
    dur = rng.randint(1, 12, size=(b, p)).astype(np.int64)
    seq = np.minimum(dur.sum(1), t).astype(np.int64)
    target = rng.standard_normal(b * t).astype(F32)
    assert ops.phone_front_ok(b, p, t, extra)
    c = ref.exact_fwd(m, k, n)
    got = ops.phone_front(dev(dur), dev(target), dev(seq), t, extra, linear=(bf(c['a']), k, bf(c['w']), dev(c['bias']), n, ops.ACT_SIGMOID))
    want = ref.linear_fwd(c['a'], c['w'], c['bias'], k, exact=True)
    assert tuple(got[6].shape) == (m, n)
    _held(got[6], want['y'], 'layer-1 forward exact (4127, 600, 512) H1')
    _shares('layer-1 forward', want['shares'], ('y',))


# ------------------------------------------------------------------------------------------------------------ what the model runs
STEP_KERNELS = {'mg_phone_front_linear_fwd_bf16', 'mg_f0_l2tail_rows_slabs_bf16', 'mg_expand_column_reduce_f32', 'mg_linear_wgrad_dgrad_bf16',
                'mg_linear_wgrad_slabs_bf16'}          # each reached by a test above (f0_l2tail_rows_expand is the _slabs_ entry)


def _kernels(calls):
    """The step's entry points without the update's (Adam's scalars and the plan kernel: tests/test_gpu_adam_plan.py)."""
    return [c for c in calls if 'adam' not in c and 'store_pair' not in c]


def test_the_model_runs_the_entry_points_tested_here():
    """One eager step and one graphs.GraphedTrainStep capture of models.F0Model(precision='bf16') on the smallest eligible batch (32 x 96
    = 3072 table rows + 1024 extra = 4096 rows, 15 360 frames) under _lib.CALL_LOG: the step's entry points are exactly the ones this
    module tests.  If dispatch changes, this fails instead of this module silently testing kernels that no longer ship."""
    from morgana_amd import data, graphs, models, optim, synthetic
    from morgana_amd import functional as F_hip
    feats = data.to_device(synthetic.make_batch(32, 480, seed=6, frames_per_phone=5.0), DEV)
    assert feats['normalised_lab'].shape[:2] == (32, 96)
    data.add_bf16_table(feats)

    def fresh():
        model = models.F0Model(precision='bf16').to(DEV)
        own = model.state_dict()
        for key, value in synthetic.f0_model_state().items():
            own[key].copy_(torch.from_numpy(value))
        return model, optim.Adam(model.parameters(), lr=0.01, fused_loop=True)

    def step_calls(log):
        first = len(log) - 1 - log[::-1].index('mg_phone_front_linear_fwd_bf16')
        return [c for c in log[first:] if not c.endswith('_status')]

    model, opt = fresh()
    for i in range(2):                                   # the first step builds the operand shadows
        if i == 1:
            _lib.CALL_LOG = []
        try:
            opt.zero_grad()
            loss, _ = model(feats)
            F_hip.backward(loss)
            opt.step()
            log = list(_lib.CALL_LOG or [])
        finally:
            _lib.CALL_LOG = None
    eager = step_calls(log)
    assert sorted(_kernels(eager)) == sorted(STEP_KERNELS), eager
    model, opt = fresh()
    _lib.CALL_LOG = []
    try:
        step = graphs.GraphedTrainStep(model, opt, feats, warmup=2)
        log = list(_lib.CALL_LOG)
    finally:
        _lib.CALL_LOG = None
    captured = step_calls(log)
    # captured whole, the expansion and the tail's slab sum ride in a later launch: the pair grid's riders
    # (mg_linear_wgrad_dgrad_expand_bf16) or the update launch's first blocks
    rides = {'mg_linear_wgrad_dgrad_expand_bf16'} if 'mg_linear_wgrad_dgrad_expand_bf16' in captured else {'mg_linear_wgrad_dgrad_bf16'}
    assert sorted(_kernels(captured)) == sorted((STEP_KERNELS - {'mg_expand_column_reduce_f32', 'mg_linear_wgrad_dgrad_bf16'}) | rides), captured
    assert torch.isfinite(step()).all()
