"""The generic bf16 Linear kernels (gemm_bf16.hip, gemm_bf16_big.hip, gemm_nt_runs.hip), the fused backward (bwd_fused_bf16.hip,
bwd_fused64_bf16.hip) and the fp32 entry points of gemm_f32.hip held to the float64 restatement of tests/linear_ref64.py ELEMENT BY
ELEMENT (``-m gpu``, MI355X): every assertion is ratio(device, Bounded reference) <= 1 over every element.  Where the reference's
bound is zero - ``exact`` operands through a bias / ReLU / no epilogue, every weight gradient of the exact family, and every bf16
output that is not ambiguous - that is bit equality with float64 arithmetic.

The rows run are the tables of tests/test_linear_bf16_ref64_host.py (FWD_TABLE, DGRAD_TABLE, WGRAD_TABLE, FUSED_TABLE): the smallest
shapes that reach each tile program, with the tuning values that switch forms in the product build, set in try / finally and reset
to 0.  Nothing in the library reports the kernel a call reached; the host test holds the restated dispatch to that table, and here
the (n_slabs, stride) the slab entry points return are asserted against the restated plans.

Two operand families per case.  ``exact``: dyadic grids, every partial sum representable (asserted in the generator), so a dropped,
doubled or misplaced term shows in full; the ambiguous share of a bf16 output is asserted to be exactly 0 wherever the epilogue's
bound is zero (forward: none and ReLU; dgrad: every epilogue and the gathered form; the fused backward's dZ1).  ``wide``: realistic scales; the structural load
lies on its fp32-output forms - with the worst-case bound a bf16 output of a K = 600 forward is ambiguous in about half of its
elements (its bound then carries one bf16 spacing) - and its bf16 runs are kept for padding, zero rows and epilogue scale.  Shares
are printed per case.

Buffer discipline: every output is pre-filled with a sentinel and has guard rows on both sides, which must not change; columns
n .. ld of a forward / dgrad output must be zero; slab floats beyond n_slabs * stride must keep the sentinel.  Row maps hold
in-range rows, -1 and rows of the zero block behind the table: a gathered zero row gives act(bias) in the forward (to the bit for
none / ReLU, and the same bits for -1 as for a zero row always) and nothing in a weight gradient (the exact family's zero bound).

For the two M > 32 768 weight-gradient rows and the long fused shape the kernel computes everything and the reference is formed for
a subset of the output units (linear_ref64.unit_subset: the first and last unit of every 128-unit tile and 64 others - 66 of 128,
82 of 1152, 72 of 512 units, i.e. 52 %, 7 % and 14 % of dW; every k column of those units, and db whole)."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import linear_ref64 as ref
from morgana_amd import _lib, ops
from parity_report import note
from recurrent_ref64 import bf16_round, ratio
from test_linear_bf16_ref64_host import DGRAD_TABLE, F32_SHAPES, FUSED_FORMS, FUSED_TABLE, FWD_TABLE, WGRAD_TABLE

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32 = np.float32
F64 = np.float64
GUARD = 3                                 # guard rows on each side of an output
SENTINEL = 768.0                          # a bf16 value no case produces
EXTRA = 8                                 # zero rows behind a table
TUNE_KEYS = {'form': ref.TUNE_FORM, 'order': ref.TUNE_WGRAD_ORDER, 'ab': ref.TUNE_AB}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bf(x):
    """A host array of bf16 VALUES as a bf16 device tensor (the conversion is exact)."""
    return dev(np.asarray(x, dtype=F32)).to(torch.bfloat16)


def host(t):
    return t.float().cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


@contextlib.contextmanager
def tuned(tune):
    lib = _lib.load()
    try:
        for key, value in tune.items():
            assert lib.mg_set_tuning(TUNE_KEYS[key], value) == 0, (key, value)
        yield
    finally:
        for key in tune:
            lib.mg_set_tuning(TUNE_KEYS[key], 0)


def _id(value):
    """Readable test ids: 2049x129x128, form3, ..."""
    if isinstance(value, tuple) and value and all(isinstance(v, int) for v in value):
        return 'x'.join(str(v) for v in value)
    if isinstance(value, tuple):
        return '+'.join('%s%s' % kv for kv in value) or 'default'
    return str(value)


def call(name, *args):
    _lib.check(getattr(_lib.load(), name)(*args), name)


def _held(got, want, label):
    """ratio(device, reference) <= 1 over every element, recorded; on failure says how many elements are out and where the first is."""
    got = np.asarray(got).reshape(want.v.shape)
    r = note(ratio(got, want), label, bound=1.0)
    print('%-100s observed / bound = %.4g' % (label, r))
    if r > 1.0:
        bad = ~(np.abs(got.astype(F64) - want.v) <= want.e)
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError('%s: observed / bound = %.4g; %d of %d elements out, first at %s: got %.9g want %.9g +- %.3g'
                             % (label, r, int(bad.sum()), bad.size, first, got[first], want.v[first], np.asarray(want.e)[first]))
    return r


def _guarded(m, ld, dtype):
    """(whole buffer, the m rows in its middle) pre-filled with the sentinel."""
    whole = torch.full((m + 2 * GUARD, ld), SENTINEL, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + m]


def _guards_intact(whole, m):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + m:] == SENTINEL).all())


def _take(b, rows):
    """Rows of a Bounded."""
    return type(b)(b.v[rows], np.asarray(b.e)[rows])


# ------------------------------------------------------------------------------------------------------------ forward
@functools.lru_cache(maxsize=2)
def _fwd_case(kind, shape):
    m, k, n = shape
    return (ref.exact_fwd if kind == 'exact' else ref.wide_fwd)(m, k, n, n_table=m, extra=EXTRA)


@functools.lru_cache(maxsize=16)
def _fwd_ref(kind, shape, with_bias, act, out_f32):
    """The reference of the whole table (m rows + the zero rows); a gathered launch takes its rows from it."""
    m, k, n = shape
    c = _fwd_case(kind, shape)
    return ref.linear_fwd(c['a'], None, c['w'], c['bias'] if with_bias else None, k, n, act, out_f32, exact=(kind == 'exact'))


def _fwd_launch(c, rows_t, m, k, n, with_bias, act, out_f32, runs, a_t, w_t, bias_t):
    ldy = (n + 7) // 8 * 8 if out_f32 else ref.pad_ld(n)
    whole, y = _guarded(m, ldy, torch.float32 if out_f32 else torch.bfloat16)
    call('mg_linear_fwd_bf16', ops._p(a_t), a_t.shape[1], ops._p(rows_t), m, k, ops._p(w_t), w_t.shape[1], ops._p(bias_t if with_bias else None), n,
         ops._p(y), ldy, 1 if out_f32 else 0, act | (ops.ACT_ROWS_RUNS if runs else 0), ops._stream())
    torch.cuda.synchronize()
    assert _guards_intact(whole, m), 'the forward wrote outside its rows'
    out = host(y)
    assert not out[:, n:].any(), 'padding columns of the output must be zero'
    return out[:, :n]


FWD_RUNS = sorted({(row[0], tuple(sorted(row[3].items())), row[2]) for row in FWD_TABLE})


@pytest.mark.parametrize('shape,tune,maps,kind', [run + (kind,) for run in FWD_RUNS for kind in ('exact', 'wide')], ids=_id)
def test_forward(shape, tune, maps, kind):
    """mg_linear_fwd_bf16: four activations, with and without bias, bf16 and fp32 out; ungathered and through a row map."""
    m, k, n = shape
    tune = dict(tune)
    c = _fwd_case(kind, shape)
    a_t, w_t, bias_t = bf(c['a']), bf(c['w']), dev(c['bias'])
    if maps == 'runs':
        jobs = [(kind_, True) for kind_ in ('runs', 'short', 'random', 'one')]
    else:
        jobs = [(None, False), ('mix', False)]
    shares = {}
    with tuned(tune):
        for map_kind, runs in jobs:
            rows = None if map_kind is None else ref.row_map(map_kind, m, m, EXTRA, seed=m)
            rows_t = None if rows is None else dev(rows)
            for with_bias in (True, False):
                for act in ref.ACTS:
                    for out_f32 in ((False,) if runs else (False, True)):
                        want = _fwd_ref(kind, shape, with_bias, act, out_f32)
                        y = _take(want['y'], np.where(rows < 0, m + EXTRA - 1, rows)) if rows is not None else _take(want['y'], slice(0, m))
                        got = _fwd_launch(c, rows_t, m, k, n, with_bias, act, out_f32, runs, a_t, w_t, bias_t)
                        label = 'fwd %s %s %s rows=%s bias=%d act=%d %s' % (kind, shape, tune, map_kind, with_bias, act, 'f32' if out_f32 else 'bf16')
                        _held(got, y, label)
                        if not out_f32:
                            shares[act] = want['share']
                        if kind == 'exact' and act in (ref.ACT_NONE, ref.ACT_RELU):
                            assert want['share'] == 0.0 and not y.e.any()
                        if rows is not None:                     # -1 and a zero row: the same bits; act(bias) - act(0) without a bias - for none / ReLU
                            zero = got[(rows < 0) | (rows >= m)]
                            assert (zero.shape[0] >= 2 or map_kind == 'one') and (zero == zero[:1]).all(), label
                            if act in (ref.ACT_NONE, ref.ACT_RELU) and zero.shape[0]:
                                b = c['bias'] if with_bias else np.zeros(n, dtype=F32)
                                b = b if act == ref.ACT_NONE else np.maximum(b, 0)
                                assert np.array_equal(zero[0], b if out_f32 else bf16_round(b)), label
    print('fwd %s %s %s ambiguous shares of the bf16 output by activation: %s' % (kind, shape, tune, shares))


# ------------------------------------------------------------------------------------------------------------ dgrad
@functools.lru_cache(maxsize=2)
def _dgrad_case(kind, shape):
    m, k, n = shape
    return (ref.exact_dgrad if kind == 'exact' else ref.wide_dgrad)(m, k, n)


DGRAD_RUNS = sorted({(row[0], tuple(sorted(row[3].items()))) for row in DGRAD_TABLE})
DGRAD_H = {ref.ACT_NONE: None, ref.ACT_SIGMOID: 'h', ref.ACT_TANH: 'hs', ref.ACT_RELU: 'hs'}


def _dgrad_launch(c, m, k, n, act, out_f32, dy_t, wt_t, h_t, h_rows_t=None):
    lddx = ref.pad_ld(k)
    whole, dx = _guarded(m, lddx, torch.float32 if out_f32 else torch.bfloat16)
    if h_rows_t is None:
        call('mg_linear_dgrad_act_bf16', ops._p(dy_t), dy_t.shape[1], m, n, ops._p(wt_t), wt_t.shape[1], k, ops._p(h_t),
             h_t.shape[1] if h_t is not None else 0, act, ops._p(dx), lddx, 1 if out_f32 else 0, ops._stream())
    else:
        call('mg_linear_dgrad_gathered_bf16', ops._p(dy_t), dy_t.shape[1], m, n, ops._p(wt_t), wt_t.shape[1], k, ops._p(h_t), h_t.shape[1],
             ops._p(h_rows_t), ops._p(dx), lddx, 1 if out_f32 else 0, ops._stream())
    torch.cuda.synchronize()
    assert _guards_intact(whole, m), 'the dgrad wrote outside its rows'
    out = host(dx)
    assert not out[:, k:].any(), 'padding columns of the output must be zero'
    return out[:, :k]


@pytest.mark.parametrize('shape,tune,kind', [run + (kind,) for run in DGRAD_RUNS for kind in ('exact', 'wide')], ids=_id)
def test_dgrad(shape, tune, kind):
    """mg_linear_dgrad_act_bf16: none, sigmoid, tanh and ReLU derivative epilogues, bf16 and fp32 out; at the large-tile shape also
    mg_linear_dgrad_gathered_bf16 with H read through h_rows from a table."""
    m, k, n = shape
    tune = dict(tune)
    c = _dgrad_case(kind, shape)
    dy_t, wt_t = bf(c['dy']), bf(c['wt'])
    shares = {}
    with tuned(tune):
        for act in ref.ACTS:
            hkey = DGRAD_H[act]
            h_t = None if hkey is None else bf(c[hkey])
            for out_f32 in (False, True):
                want = ref.linear_dgrad(c['dy'], c['wt'], None if hkey is None else c[hkey], k, n, act, out_f32, exact=(kind == 'exact'))
                got = _dgrad_launch(c, m, k, n, act, out_f32, dy_t, wt_t, h_t)
                _held(got, want['dx'], 'dgrad %s %s %s act=%d %s' % (kind, shape, tune, act, 'f32' if out_f32 else 'bf16'))
                if not out_f32:
                    shares[act] = want['share']
                if kind == 'exact':                      # every derivative epilogue is exact on these grids: bit equality, no ambiguous element
                    assert want['share'] == 0.0 and not want['dx'].e.any(), (act, out_f32)
        if ref.dgrad_program(m, k, n, ref.pad_ld(n), ref.pad_ld(n), ref.pad_ld(k), ab=tune.get('ab', 0)).startswith('gemm_nt_big'):
            h_rows = np.random.RandomState(m).randint(0, 300, m).astype(np.int32)          # H is a table of 300 rows
            h_rows[0], h_rows[m - 1] = 299, 0
            h_t = bf(c['h'][:300])
            for out_f32 in (False, True):
                want = ref.linear_dgrad(c['dy'], c['wt'], c['h'][:300], k, n, ref.ACT_SIGMOID, out_f32, h_rows=h_rows, exact=(kind == 'exact'))
                got = _dgrad_launch(c, m, k, n, ref.ACT_SIGMOID, out_f32, dy_t, wt_t, h_t, dev(h_rows))
                _held(got, want['dx'], 'dgrad gathered %s %s %s %s' % (kind, shape, tune, 'f32' if out_f32 else 'bf16'))
                if kind == 'exact':
                    assert want['share'] == 0.0 and not want['dx'].e.any(), out_f32
    print('dgrad %s %s %s ambiguous shares of the bf16 output by activation: %s' % (kind, shape, tune, shares))


# ------------------------------------------------------------------------------------------------------------ weight gradient
@functools.lru_cache(maxsize=2)
def _wgrad_case(kind, shape, lda):
    m, k, n = shape
    return (ref.exact_wgrad if kind == 'exact' else ref.wide_wgrad)(m, k, n, lda=lda, n_table=m, extra=EXTRA)


@functools.lru_cache(maxsize=8)
def _wgrad_ref(kind, shape, lda, n_slabs, map_kind, dy_map, prior):
    m, k, n = shape
    c = _wgrad_case(kind, shape, lda)
    rows = None if map_kind is None else ref.row_map(map_kind, m, m, EXTRA, seed=m)
    dy_rows = None if not dy_map else _dy_rows(m)
    units = ref.unit_subset(n) if m > 32768 else None
    return ref.linear_wgrad(c['dy'], c['a'], rows, k, n, n_slabs, dy_rows=dy_rows, prior_w=(c['prior_w'] if units is None else c['prior_w'][units]) if prior else None,
                            prior_b=c['prior_b'] if prior else None, exact=(kind == 'exact'), units=units), units


def _dy_rows(m):
    r = np.random.RandomState(7 * m).randint(0, m, m).astype(np.int32)
    r[0], r[m - 1] = m - 1, 0
    return r


def _check_wgrad(label, dw, db, want, units):
    dw = host(dw)
    _held(dw if units is None else dw[units], want['dw'], label + ' dW')
    if db is not None:
        _held(host(db), want['db'], label + ' db')


WGRAD_RUNS = sorted((row[0], row[1], kind, tuple(sorted(row[2].items())), row[3], row[4], row[5]) for row in WGRAD_TABLE for kind in ('exact', 'wide'))


@pytest.mark.parametrize('shape,lda,kind,tune,program,rows_program,plan', WGRAD_RUNS, ids=_id)
def test_weight_gradient(shape, lda, tune, program, rows_program, plan, kind):
    """mg_linear_wgrad_bf16 and, where it takes the shape, mg_linear_wgrad_rows_bf16: dW and db in one buffer (one reduce launch),
    separate buffers onto a non-zero prior with accumulate (two), want_bias=False; mg_linear_wgrad_slabs_bf16 + mg_slab_reduce_f32; A
    ungathered and through a row map with -1 and zero rows."""
    m, k, n = shape
    tune = dict(tune)
    c = _wgrad_case(kind, shape, lda)
    dy_t, a_t = bf(c['dy']), bf(c['a'])
    n_slabs = plan[0]
    big = program.startswith('wgrad_big')
    label = 'wgrad %s %s %s' % (kind, shape, tune)
    with tuned(tune):
        for map_kind in ((None, 'mix') if m <= 32768 else (None,)):          # the two long shapes gather through the rows entry below
            rows_t = None if map_kind is None else dev(ref.row_map(map_kind, m, m, EXTRA, seed=m))
            # one buffer, accumulate = 0, onto a sentinel; guard floats on both sides
            want, units = _wgrad_ref(kind, shape, lda, n_slabs, map_kind, False, False)
            both = torch.full((n * k + n + 2 * 64,), SENTINEL, device=DEV)
            dw, db = both[64:64 + n * k].view(n, k), both[64 + n * k:64 + n * k + n]
            ops.linear_wgrad_bf16(dy_t, a_t, rows_t, m, n, k, out_w=dw, out_b=db)
            assert bool((both[:64] == SENTINEL).all()) and bool((both[-64:] == SENTINEL).all())
            _check_wgrad(label + ' rows=%s one buffer' % map_kind, dw, db, want, units)
            # separate buffers, accumulate = 1 onto a non-zero prior
            want, units = _wgrad_ref(kind, shape, lda, n_slabs, map_kind, False, True)
            dw2, db2 = dev(c['prior_w']).clone(), dev(c['prior_b']).clone()
            ops.linear_wgrad_bf16(dy_t, a_t, rows_t, m, n, k, out_w=dw2, out_b=db2, accumulate=True)
            _check_wgrad(label + ' rows=%s accumulate' % map_kind, dw2, db2, want, units)
            # no bias: dW held to the same reference (and as before to the bit), nothing written behind it
            want, units = _wgrad_ref(kind, shape, lda, n_slabs, map_kind, False, False)
            lone = torch.full((n * k + 64,), SENTINEL, device=DEV)
            ops.linear_wgrad_bf16(dy_t, a_t, rows_t, m, n, k, want_bias=False, out_w=lone[:n * k].view(n, k))
            assert bool((lone[n * k:] == SENTINEL).all())
            _check_wgrad(label + ' rows=%s no bias' % map_kind, lone[:n * k].view(n, k), None, want, units)
            assert torch.equal(lone[:n * k].view(n, k), dw)
            if big:
                # the slabs themselves: the plan, zeros in empty splits, nothing past n_slabs * stride; one reduce launch for dW | db
                nbytes = int(_lib.load().mg_linear_wgrad_workspace_bytes(m, n, k))
                slab = torch.full((nbytes // 4 + 64,), float('nan'), device=DEV)
                slab[nbytes // 4:] = SENTINEL
                _, got_slabs, got_stride = ops.linear_wgrad_slabs_bf16(dy_t, a_t, rows_t, m, n, k, slab=slab[:nbytes // 4].view(torch.uint8))
                assert (got_slabs, got_stride) == (n_slabs, n * k + n), (got_slabs, got_stride, plan)
                assert bool((slab[nbytes // 4:] == SENTINEL).all())
                if nbytes // 4 > n_slabs * got_stride:
                    assert bool(torch.isnan(slab[n_slabs * got_stride:nbytes // 4]).all()), 'floats beyond n_slabs * stride were written'
                used = -(-m // plan[1])
                slabs = slab[:n_slabs * got_stride].view(n_slabs, got_stride)
                assert bool(torch.isfinite(slabs).all()) and not bool(slabs[used:].any())
                total = ops.slab_reduce(slab, n_slabs, got_stride, n * k + n, torch.full((n * k + n,), SENTINEL, device=DEV))
                want, units = _wgrad_ref(kind, shape, lda, n_slabs, map_kind, False, False)
                _check_wgrad(label + ' rows=%s slabs' % map_kind, total[:n * k].view(n, k), total[n * k:], want, units)
        if rows_program is not None:
            dy_rows_t = dev(_dy_rows(m))
            rows_slabs = ref.wgrad_plan_big(m, n, k, lda, ref.pad_ld(n), tune.get('ab', 0))[0]      # the rows entry always takes the wide plan
            for map_kind, prior in ((None, False), ('mix', True)):
                rows_t = None if map_kind is None else dev(ref.row_map(map_kind, m, m, EXTRA, seed=m))
                want, units = _wgrad_ref(kind, shape, lda, rows_slabs, map_kind, True, prior)
                if prior:
                    dw, db = dev(c['prior_w']).clone(), dev(c['prior_b']).clone()
                else:
                    dw, db = torch.full((n, k), SENTINEL, device=DEV), torch.full((n,), SENTINEL, device=DEV)
                ops.linear_wgrad_rows_bf16(dy_t, dy_rows_t, a_t, rows_t, m, n, k, out_w=dw, out_b=db, accumulate=prior)
                _check_wgrad(label + ' rows entry rows=%s' % map_kind, dw, db, want, units)
                # dW and db in one buffer (one reduce launch) and no bias at all, each with a sentinel behind
                want, units = _wgrad_ref(kind, shape, lda, rows_slabs, map_kind, True, False)
                both = torch.full((n * k + n + 64,), SENTINEL, device=DEV)
                ops.linear_wgrad_rows_bf16(dy_t, dy_rows_t, a_t, rows_t, m, n, k, out_w=both[:n * k].view(n, k), out_b=both[n * k:n * k + n])
                assert bool((both[n * k + n:] == SENTINEL).all())
                _check_wgrad(label + ' rows entry rows=%s one buffer' % map_kind, both[:n * k].view(n, k), both[n * k:n * k + n], want, units)
                lone = torch.full((n * k + 64,), SENTINEL, device=DEV)
                ops.linear_wgrad_rows_bf16(dy_t, dy_rows_t, a_t, rows_t, m, n, k, want_bias=False, out_w=lone[:n * k].view(n, k))
                assert bool((lone[n * k:] == SENTINEL).all())
                _check_wgrad(label + ' rows entry rows=%s no bias' % map_kind, lone[:n * k].view(n, k), None, want, units)
        elif big:
            with pytest.raises(ValueError):                # the half-width and 640-wide tiles have no gathered-dY form: an error, no fallback
                ops.linear_wgrad_rows_bf16(dy_t, dev(_dy_rows(m)), a_t, None, m, n, k)


# ------------------------------------------------------------------------------------------------------------ fused backward
FUSED_MAPS = ('runs', 'short', 'random', 'one', 'mixed', 'pads')


@functools.lru_cache(maxsize=2)
def _fused_case(kind, shape):
    m, n_hidden, k0 = shape
    return (ref.exact_fused if kind == 'exact' else ref.wide_fused)(m, n_hidden, k0, m, extra=64)


@functools.lru_cache(maxsize=4)
def _fused_ref(kind, shape, n_slabs, map_kind, second=False):
    m, n_hidden, k0 = shape
    c = _fused_case(kind, shape)
    rows = None if map_kind is None else ref.row_map(map_kind, m, m, 64, seed=m)
    units = ref.unit_subset(n_hidden) if m > 20000 else None
    return ref.fused_bwd(c['dz2'], c['w2t'], c['h1'], c['a'], rows, n_hidden, k0, n_slabs, exact=(kind == 'exact'), exact_rows=(kind == 'exact'),
                         units=units, second=second), units


def _fused_operands(c):
    return bf(c['dz2']), bf(c['w2t']), bf(c['h1']), bf(c['a'])


def _fused_prior(n_hidden, k0):
    """A non-zero prior on the exact family's grid (j / 8, at most 10 in size: with sum |terms| < 246 every partial sum stays exact)."""
    rng = np.random.RandomState(n_hidden + k0)
    return (rng.randint(-80, 81, (n_hidden, k0)) / 8.0).astype(F32), (rng.randint(-80, 81, n_hidden) / 8.0).astype(F32)


def _check_fused_prior(label, both, want, units, c, kind, m, n_hidden, k0, n_slabs):
    """dW1 | db1 accumulated onto _fused_prior, against the reference plus the prior."""
    pw, pb = _fused_prior(n_hidden, k0)
    exact = kind == 'exact'
    assert not exact or c['sum_abs'] + 10.0 < 2.0 ** 8
    dwh = host(both[:n_hidden * k0]).reshape(n_hidden, k0)
    _held(dwh if units is None else dwh[units], ref.plus_prior(want['dw1'], pw if units is None else pw[units], m + n_slabs, exact), label + ' dW1')
    _held(host(both[n_hidden * k0:n_hidden * k0 + n_hidden]), ref.plus_prior(want['db1'], pb, m + n_slabs, exact), label + ' db1')


# the long shape runs the maps that differ in ring traffic (runs, short, random); its reference covers a subset of the units
FUSED_RUNS = [(shape, plan, kind, map_kind) for shape, plan in FUSED_TABLE for kind in ('exact', 'wide')
              for map_kind in (FUSED_MAPS + (None,) if shape[0] < 20000 else FUSED_MAPS[:3])]


@pytest.mark.parametrize('shape,plan,kind,map_kind', FUSED_RUNS, ids=_id)
def test_fused_backward(shape, plan, kind, map_kind):
    """mg_linear_bwd_fused_bf16 under every form the product build has (MG_TUNE_FORM 0, 12, 13, 7; no row map: the single-buffered
    kernel) against dW1 | db1 formed from the ROUNDED dZ1; dW and db in separate sentinel buffers, and (runs map, no map)
    accumulate = 1 onto a non-zero prior in one buffer."""
    m, n_hidden, k0 = shape
    c = _fused_case(kind, shape)
    dz2, w2t, h1, a = _fused_operands(c)
    rows_t = None if map_kind is None else dev(ref.row_map(map_kind, m, m, 64, seed=m))
    want, units = _fused_ref(kind, shape, plan[0], map_kind)
    if kind == 'exact':
        assert want['share'] == 0.0 and not want['dw1'].e.any() and not want['db1'].e.any()
    for with_rows, form, program in FUSED_FORMS:
        if with_rows != (map_kind is not None):
            continue
        with tuned({'form': form} if form else {}):
            dw, db = torch.full((n_hidden, k0), SENTINEL, device=DEV), torch.full((n_hidden + 64,), SENTINEL, device=DEV)
            ops.linear_bwd_fused_bf16(dz2, w2t, h1, a, rows_t, m, n_hidden, k0, out_w=dw, out_b=db[:n_hidden])
        assert bool((db[n_hidden:] == SENTINEL).all())
        label = 'fused %s %s rows=%s %s' % (kind, shape, map_kind, program)
        dwh = host(dw)
        _held(dwh if units is None else dwh[units], want['dw1'], label + ' dW1')
        _held(host(db[:n_hidden]), want['db1'], label + ' db1')
        if map_kind == 'pads':
            assert not dwh.any()
    if map_kind in ('runs', None):                    # accumulate = 1 onto a non-zero prior, dW | db in one buffer (one reduce launch)
        pw, pb = _fused_prior(n_hidden, k0)
        both = torch.cat([dev(pw).reshape(-1), dev(pb), torch.full((64,), SENTINEL, device=DEV)])
        ops.linear_bwd_fused_bf16(dz2, w2t, h1, a, rows_t, m, n_hidden, k0, out_w=both[:n_hidden * k0].view(n_hidden, k0),
                                  out_b=both[n_hidden * k0:n_hidden * k0 + n_hidden], accumulate=True)
        assert bool((both[n_hidden * k0 + n_hidden:] == SENTINEL).all())
        _check_fused_prior('fused %s %s rows=%s accumulate' % (kind, shape, map_kind), both, want, units, c, kind, m, n_hidden, k0, plan[0])
    print('fused %s %s rows=%s ambiguous share of dZ1: %.3g' % (kind, shape, map_kind, want['share']))


@pytest.mark.parametrize('shape,plan,kind', [(shape, plan, kind) for shape, plan in FUSED_TABLE for kind in ('exact', 'wide')], ids=_id)
def test_fused_backward_slab_entries(shape, plan, kind):
    """mg_linear_bwd_fused_slabs_bf16 and mg_linear_bwd_fused2_slabs_bf16: n_slabs, strides, offsets and counts as the restated plan,
    empty floats untouched, both layers' slab sums within the reference's bounds, accumulate onto a prior through the reduce."""
    m, n_hidden, k0 = shape
    c = _fused_case(kind, shape)
    dz2, w2t, h1, a = _fused_operands(c)
    lib = _lib.load()
    n1, n2 = n_hidden * k0 + n_hidden, 128 * n_hidden + 128
    for map_kind in ('runs', 'short'):
        rows_t = dev(ref.row_map(map_kind, m, m, 64, seed=m))
        want, units = _fused_ref(kind, shape, plan[0], map_kind, second=True)
        label = 'fused slabs %s %s rows=%s' % (kind, shape, map_kind)
        nbytes = int(lib.mg_linear_bwd_fused_workspace_bytes(m, n_hidden, k0))
        slab = torch.full((nbytes // 4 + 64,), SENTINEL, device=DEV)
        _, n_slabs, stride = ops.linear_bwd_fused_slabs_bf16(dz2, w2t, h1, a, rows_t, m, n_hidden, k0, slab=slab[:nbytes // 4].view(torch.uint8))
        assert (n_slabs, stride) == (plan[0], n1), (n_slabs, stride, plan)
        assert bool((slab[n_slabs * stride:] == SENTINEL).all()), 'floats beyond n_slabs * stride were written'
        total = ops.slab_reduce(slab, n_slabs, stride, n1, torch.full((n1,), SENTINEL, device=DEV))
        dwh = host(total[:n_hidden * k0]).reshape(n_hidden, k0)
        _held(dwh if units is None else dwh[units], want['dw1'], label + ' dW1')
        _held(host(total[n_hidden * k0:]), want['db1'], label + ' db1')
        pw, pb = _fused_prior(n_hidden, k0)
        onto = torch.cat([dev(pw).reshape(-1), dev(pb), torch.full((64,), SENTINEL, device=DEV)])
        ops.slab_reduce(slab, n_slabs, stride, n1, onto, accumulate=True)
        assert bool((onto[n1:] == SENTINEL).all())
        _check_fused_prior(label + ' reduce onto a prior', onto, want, units, c, kind, m, n_hidden, k0, n_slabs)
        nbytes = int(lib.mg_linear_bwd_fused2_workspace_bytes(m, n_hidden, k0))
        slab = torch.full((nbytes // 4 + 64,), SENTINEL, device=DEV)
        _, n_slabs, (off1, st1, cnt1), (off2, st2, cnt2) = ops.linear_bwd_fused2_slabs_bf16(dz2, w2t, h1, a, rows_t, m, n_hidden, k0,
                                                                                            slab=slab[:nbytes // 4].view(torch.uint8))
        assert (n_slabs, off1, st1, cnt1, off2, st2, cnt2) == (plan[0], 0, n1, n1, plan[0] * n1, n2, n2)
        assert bool((slab[off2 + n_slabs * st2:] == SENTINEL).all()), 'floats beyond the second layer\'s slabs were written'
        got1 = ops.slab_reduce(slab[off1:], n_slabs, st1, cnt1, torch.full((cnt1,), SENTINEL, device=DEV))
        got2 = ops.slab_reduce(slab[off2:], n_slabs, st2, cnt2, torch.full((cnt2,), SENTINEL, device=DEV))
        dwh = host(got1[:n_hidden * k0]).reshape(n_hidden, k0)
        _held(dwh if units is None else dwh[units], want['dw1'], label + ' fused2 dW1')
        _held(host(got1[n_hidden * k0:]), want['db1'], label + ' fused2 db1')
        _held(host(got2[:128 * n_hidden]).reshape(128, n_hidden), want['dw2'], label + ' fused2 dW2')
        _held(host(got2[128 * n_hidden:]), want['db2'], label + ' fused2 db2')


# ------------------------------------------------------------------------------------------------------------ fp32 entry points
@pytest.mark.parametrize('shape,kind', [(shape, kind) for shape in F32_SHAPES for kind in ('exact', 'wide')], ids=_id)
def test_fp32_entry_points(shape, kind):
    """mg_linear_fwd_f32, mg_linear_dgrad_act_f32, mg_linear_wgrad_f32 against the same reference: nothing is rounded to bf16 there, so
    exact operands give bit equality (asserted through the zero bound).  The wide operands are full fp32 values, not bf16 ones, the gradients with
    the row scales of the bf16 family (e^+-3, one row in ten zero, a heavy last row)."""
    m, k, n = shape
    exact = kind == 'exact'
    rng = np.random.RandomState(m)
    if exact:
        cf, cd, cw = ref.exact_fwd(m, k, n, lda=k, extra=EXTRA), ref.exact_dgrad(m, k, n), ref.exact_wgrad(m, k, n, lda=k, extra=EXTRA)
    else:
        cf = {'a': np.concatenate([rng.uniform(0, 1, (m, k)), np.zeros((EXTRA, k))]).astype(F32), 'w': rng.uniform(-0.1, 0.1, (n, k)).astype(F32),
              'bias': rng.uniform(-0.1, 0.1, n).astype(F32)}
        cd = {'dy': ref.scaled_grads(rng, m, n, bf16=False), 'wt': rng.uniform(-0.1, 0.1, (k, n)).astype(F32),
              'h': rng.uniform(0.05, 0.95, (m, k)).astype(F32), 'hs': rng.uniform(-0.95, 0.95, (m, k)).astype(F32)}
        cw = {'dy': cd['dy'], 'a': cf['a']}
    maps = [None] + ([ref.row_map('mix', m, m, EXTRA, seed=m)] if shape == (777, 609, 256) else [])
    label = 'f32 %s %s' % (kind, shape)
    w_t, bias_t = dev(np.ascontiguousarray(cf['w'][:, :k])), dev(cf['bias'])
    for rows in maps:
        a_t = dev(np.ascontiguousarray(cf['a'][:, :k]))
        for act in ref.ACTS:
            got = ops.linear_fwd_f32(a_t, None if rows is None else dev(rows), m, w_t, bias_t, act)
            want = ref.linear_fwd(cf['a'] if rows is not None else cf['a'][:m], rows, cf['w'], cf['bias'], k, n, act, out_f32=True, exact=exact, fast=False)
            _held(host(got), want['y'], label + ' fwd act=%d rows=%s' % (act, rows is not None))
        aw = np.ascontiguousarray(cw['a'][:, :k])
        n_slabs = ref.wgrad_plan_f32(m, n, k)[0]
        dw, db = ops.linear_wgrad_f32(dev(np.ascontiguousarray(cw['dy'][:, :n])), dev(aw), None if rows is None else dev(rows), n, k)
        want = ref.linear_wgrad(cw['dy'], aw, rows, k, n, n_slabs, exact=exact)
        _held(host(dw), want['dw'], label + ' wgrad dW rows=%s' % (rows is not None))
        _held(host(db), want['db'], label + ' wgrad db rows=%s' % (rows is not None))
    w_nk = dev(np.ascontiguousarray(cd['wt'][:k, :n].T))
    dy_t = dev(np.ascontiguousarray(cd['dy'][:, :n]))
    for act in ref.ACTS:
        hkey = DGRAD_H[act]
        h = None if hkey is None else np.ascontiguousarray(cd[hkey][:m, :k])
        got = ops.linear_dgrad_f32(dy_t, w_nk, None if h is None else dev(h), act)
        want = ref.linear_dgrad(cd['dy'], cd['wt'], h, k, n, act, out_f32=True, exact=exact)
        _held(host(got), want['dx'], label + ' dgrad act=%d' % act)
