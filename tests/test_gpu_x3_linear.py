"""The generic 'bf16x3' Linear entry points of morgana_amd/ops.py - linear_fwd_x3, linear_dgrad_x3, linear_wgrad_x3_rows,
linear_wgrad_x3_stacked, linear_wgrad_x3 - on the three-plane buffers of ops.split3, each against the float64 restatement of
tests/x3_ref64.py (``-m gpu``, MI355X).  Every assertion on a product is ratio(device, Bounded reference) <= 1, twice: against the three
products of the split planes under the fp32 accumulation bound gamma(T + 2) sum |a||w|, and against float64 arithmetic on the original
fp32 operands under that bound plus the mode's published 2^-16 sum |a||w|.  Every ratio goes to the parity report (``note``).

Operands (x3_ref64.make_case): row scales spread over e^+-3 and lo planes at 0.4 - 0.6 of their largest possible weight with one sign
along every contraction index, so that a dropped or mispaired cross term is 13 - 1800 bounds away in the forward and the dgrad and in
the weight gradients up to m = 777, and 2.2 - 5.3 bounds at m = 2049 / 4100 / 4999 (tests/test_x3_ref64_host.py asserts these
figures on these inputs; the weight gradient's bound grows with 3 m, a cross term cannot: |lo| <= 2^-8 |x|).

Shapes (m, k, n) and the tile programs they reach.  The contraction index of forward / dgrad is 3 pad_ld(k) / 3 pad_ld(n) - 120, 1920,
1920, 1920, 384, 1920, 48 for the forward (pad_ld rounds 600, 609 and 620 to 640), stepped in tiles of 32 (NT_BK of gemm_bf16.hip, the
stage depth of gemm_nt_big_kernel).  (130, 40, 96): 120 = 3 x 32 + 24, a ragged last k tile, and plane boundaries (40, 80) inside k
tiles; one ragged 128-row tile of gemm_nt_bf16_kernel<128, 128>; N = 96 below the 128 tile.  (5, 9, 100): 48 = 32 + 16, planes of 16; an
fp32 output padded to 104 columns.  (777, 609, 256) and (64, 600, 512): the 128 x 128 program, 60 k tiles, plane boundaries on tile 20
and 40, M = 777 ragged / M below one tile.  (4100, 600, 512), (4999, 128, 512), (2049, 620, 128): M >= 2048 and N % 128 == 0 -
gemm_nt_big_kernel<128> (256-row tiles, ragged last one; 60 or 12 k tiles against a ring of 6 stages; its 256-wide form needs 128
tile columns, M >= 16 384 at N = 512, and stays with the whole-model tests); with a row map the same programs gather.  The dgrad's
output is pad_ld(k) wide, so only k = 128 (4999 rows) takes the large tile there.  Weight gradients: rows / stacked contract over 3 m
rows - (4100, 600, 512): wgrad_big_kernel<5> (12 300 rows, 640-wide operand, four n tiles: the half-width plan), (2049, 620, 128):
wgrad_big_kernel<10> (6 147 rows, one n tile), the others wgrad_bf16_kernel<128, 128> with 3 m = 15, 192, 390, 2 331, 14 997 rows over
1 - 30 slabs; linear_wgrad_x3 contracts over m: the large tile at m = 4100 only, with and without the gather.

Headroom of the bounds, measured by tests/test_x3_ref64_host.py (float32 numpy over the same layouts, ascending and permuted order;
worst observed / bound): forward 0.145, dgrad 0.107, weight gradient rows 0.131 / stacked 0.187 / separate planes 0.187, bias
gradient 0.107, sigmoid gradient 0.407, its weight gradient 0.410; against the fp32 operands (the published 2^-16, not a derived
worst case: one dominant term uses most of it) forward 0.607, dgrad 0.467, weight gradients 0.738 - 0.778.  On this module's own
operands the split alone uses at most 0.91 of the 2^-16 (weight gradient of (5, 9, 100)); the rest of that figure is the first bound.
"""
import functools

import numpy as np
import pytest
import torch

import x3_ref64 as ref
from morgana_amd import ops
from parity_report import note
from recurrent_ref64 import Bounded, ratio

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = -12345.0
ACTS = (ops.ACT_NONE, ops.ACT_SIGMOID, ops.ACT_TANH, ops.ACT_RELU)        # functional.LinearStackFn hands all four to linear_fwd_x3


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _held(got, want, label):
    """ratio(device, reference) <= 1, recorded."""
    r = note(ratio(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, want), label, bound=1.0)
    print('%-70s observed / bound = %.4f' % (label, r))
    assert r <= 1.0, (label, r)


@functools.lru_cache(maxsize=None)
def _case(shape):
    return ref.make_case(shape)


@functools.lru_cache(maxsize=None)
def _wgrad_ref(shape, gathered):
    c = _case(shape)
    if gathered:
        return ref.linear_wgrad(c['g'], c['table'], c['rows'], c['extra'])
    return ref.linear_wgrad(c['g'], c['a'])


def _prior(shape, first):
    n, k = first.v.shape
    rng = np.random.RandomState(n + k)
    return (rng.standard_normal((n, k)) * np.abs(first.v).mean()).astype(np.float32), rng.standard_normal(n).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ operands
@pytest.mark.parametrize('shape', ref.SHAPES)
def test_split_operands_are_the_reference_operands(shape):
    """Every buffer the products below read, bit for bit what the reference splits on the host: planes, their order, zero padding,
    the zero rows behind a table - so that the references' operands ARE the kernels' operands."""
    c = _case(shape)
    a, w, g, table = dev(c['a']), dev(c['w']), dev(c['g']), dev(c['table'])
    outs = ops.split3([(a, 0, False), (table, 0, False, c['extra']), (w, 1, False), (w, 0, True), (g, 1, False), (g, 2, False),
                       (table, 2, False, c['extra']), (g, 3, False), (a, 4, False)])
    wants = [ref.plane_bits(c['a'], 0), ref.plane_bits(c['table'], 0, extra=c['extra']), ref.plane_bits(c['w'], 1),
             ref.plane_bits(c['w'], 0, transpose=True), ref.plane_bits(c['g'], 1), ref.plane_bits(c['g'], 2),
             ref.plane_bits(c['table'], 2, extra=c['extra']), ref.plane_bits(c['g'], 3), ref.plane_bits(c['a'], 4)]
    for i, (got, want) in enumerate(zip(outs, wants)):
        assert tuple(got.shape) == want.shape and np.array_equal(_bits(got), want), i


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('gathered', [False, True])
@pytest.mark.parametrize('shape', ref.SHAPES)
def test_linear_fwd_x3(shape, gathered):
    """All four activations, with and without bias; without a row map, and with one over a split made with extra > 0 whose entries
    point into the table, at the zero rows behind it (padding frames) and below zero (a zero row)."""
    m, k, n = shape
    c = _case(shape)
    src, extra, rows = (c['table'], c['extra'], c['rows']) if gathered else (c['a'], 0, None)
    a3, w3 = ops.split3([(dev(src), 0, False, extra), (dev(c['w']), 1, False)])
    rows_dev = dev(rows) if gathered else None
    for bias in (c['bias'], None):
        pre_first, pre_second = ref.linear_fwd(src, c['w'], bias, ops.ACT_NONE, rows, extra)
        for act in ACTS if bias is not None else (ops.ACT_NONE, ops.ACT_SIGMOID):
            y = ops.linear_fwd_x3(a3, rows_dev, m, w3, dev(bias) if bias is not None else None, n, act)
            assert tuple(y.shape) == (m, n) and y.dtype == torch.float32
            first, second = ref.activate(pre_first, act), ref.activate(pre_second, act)
            tag = 'fwd %s act %d bias %d gathered %d' % (shape, act, bias is not None, gathered)
            _held(y, first, tag + ', planes')
            _held(y, second, tag + ', fp32 operands')
    if gathered:
        # rows that gather a zero row give act(bias) exactly: no trace of any table row
        y = ops.linear_fwd_x3(a3, rows_dev, m, w3, dev(c['bias']), n, ops.ACT_NONE).cpu().numpy()
        zero = (rows < 0) | (rows >= src.shape[0])
        assert zero.any() and np.array_equal(y[zero], np.broadcast_to(c['bias'], y[zero].shape))
    with pytest.raises(ValueError):
        ops.linear_fwd_x3(a3, rows_dev, m, w3[:, :w3.shape[1] - 8], None, n, ops.ACT_NONE)


@pytest.mark.parametrize('shape', ref.SHAPES)
def test_linear_fwd_x3_activations_in_their_steep_part(shape):
    """The epilogues on ordinary operands with pre-activations of order 1 (x3_ref64.make_activation_case): make_case's one-signed
    products sit deep in saturation on most rows, where a sigmoid or tanh cannot be told from a constant."""
    m, k, n = shape
    c = ref.make_activation_case(shape)
    a3, w3 = ops.split3([(dev(c['a']), 0, False), (dev(c['w']), 1, False)])
    pre_first, pre_second = ref.linear_fwd(c['a'], c['w'], c['bias'])
    assert np.abs(pre_first.v).mean() < 3 and (pre_first.v > 0).mean() > 0.1 and (pre_first.v < 0).mean() > 0.1
    for act in ACTS:
        y = ops.linear_fwd_x3(a3, None, m, w3, dev(c['bias']), n, act)
        _held(y, ref.activate(pre_first, act), 'fwd steep %s act %d, planes' % (shape, act))
        _held(y, ref.activate(pre_second, act), 'fwd steep %s act %d, fp32 operands' % (shape, act))


# ------------------------------------------------------------------------------------------------------------ dgrad
@pytest.mark.parametrize('shape', ref.SHAPES)
def test_linear_dgrad_x3(shape):
    """g3 in order 1 against split3(w, 0, transpose=True); the output has exactly k columns (nothing of the padded width leaks)."""
    m, k, n = shape
    c = _case(shape)
    g3, wt3 = ops.split3([(dev(c['g']), 1, False), (dev(c['w']), 0, True)])
    dx = ops.linear_dgrad_x3(g3, m, wt3, k)
    assert tuple(dx.shape) == (m, k) and dx.is_contiguous()
    first, second = ref.linear_dgrad(c['g'], c['w'])
    _held(dx, first, 'dgrad %s, planes' % (shape,))
    _held(dx, second, 'dgrad %s, fp32 operands' % (shape,))
    # the kernel's own output is pad_ld(k) wide: the entry point returns its first k columns, the same numbers
    padded = ops.linear_dgrad_bf16(g3, m, g3.shape[1], wt3, k, None, out_f32=True)
    assert tuple(padded.shape) == (m, ops.pad_ld(k)) and torch.equal(padded[:, :k], dx)


# ------------------------------------------------------------------------------------------------------------ weight gradients
def _modes(shape, call, first, second, terms, db_ref, tag):
    """One weight-gradient form in its three modes.  call(out_w, out_b, accumulate) -> (dw, db)."""
    n, k = first.v.shape
    dw, db = call(None, None, False)
    assert tuple(dw.shape) == (n, k) and tuple(db.shape) == (n,)
    _held(dw, first, tag + ' fresh dW, planes')
    _held(dw, second, tag + ' fresh dW, fp32 operands')
    _held(db, db_ref(None), tag + ' fresh db')
    # accumulate=False over a sentinel: overwritten (the same numbers as the fresh call: one deterministic order)
    both = torch.full((n * k + n,), SENTINEL, dtype=torch.float32, device=DEV)
    out_w, out_b = both[:n * k].view(n, k), both[n * k:]
    got_w, got_b = call(out_w, out_b, False)
    assert got_w.data_ptr() == out_w.data_ptr() and got_b.data_ptr() == out_b.data_ptr()
    assert torch.equal(out_w, dw) and torch.equal(out_b, db)
    # accumulate=True over known contents: added to
    prior_w, prior_b = _prior(shape, first)
    both = torch.cat((dev(prior_w).reshape(-1), dev(prior_b)))
    out_w, out_b = both[:n * k].view(n, k), both[n * k:]
    call(out_w, out_b, True)
    acc_first, acc_second = ref.add_prior(first, second, prior_w, terms)
    _held(out_w, acc_first, tag + ' accumulate dW, planes')
    _held(out_w, acc_second, tag + ' accumulate dW, fp32 operands')
    _held(out_b, db_ref(prior_b), tag + ' accumulate db')
    # separate (non-adjacent) destinations
    out_w, out_b = torch.full((n, k), SENTINEL, device=DEV), torch.full((n + 3,), SENTINEL, device=DEV)
    call(out_w, out_b[:n], False)
    assert torch.equal(out_w, dw) and torch.equal(out_b[:n], db) and bool((out_b[n:] == SENTINEL).all())
    return dw, db


@pytest.mark.parametrize('shape', ref.SHAPES)
def test_linear_wgrad_x3_rows(shape):
    """The row-interleaved (3 m, ldp) reading of the order-1 gradient split against the forward's order-0 activation split, db from
    split3's column sums.  Every n of these shapes has a plane width split3_colsum_ok takes (96 and 100 pad to 128: taken, not
    refused - the rule is 256 % (pad_ld(n) / 8) == 0; test_colsum_width_rule holds a width it refuses)."""
    m, k, n = shape
    c = _case(shape)
    assert ops.split3_colsum_ok(n)
    (g1, colsum), a0 = ops.split3([(dev(c['g']), 1, False, 0, None, True), (dev(c['a']), 0, False)])
    first, second = _wgrad_ref(shape, False)
    n_slabs = colsum.shape[0]
    dw, db = _modes(shape, lambda ow, ob, acc: ops.linear_wgrad_x3_rows(g1, colsum, a0, n, k, out_w=ow, out_b=ob, accumulate=acc), first, second,
                    3 * m, lambda prior: ref.bias_grad(c['g'], n_slabs, prior=prior), 'wgrad rows %s' % (shape,))
    # colsum=None: no bias gradient, out_b untouched
    dw2, db2 = ops.linear_wgrad_x3_rows(g1, None, a0, n, k)
    assert db2 is None and torch.equal(dw2, dw)
    out_w, out_b = torch.full((n, k), SENTINEL, device=DEV), torch.full((n,), SENTINEL, device=DEV)
    _, db3 = ops.linear_wgrad_x3_rows(g1, None, a0, n, k, out_w=out_w, out_b=out_b)
    assert db3 is None and torch.equal(out_w, dw) and bool((out_b == SENTINEL).all())
    with pytest.raises(ValueError):
        ops.linear_wgrad_x3_rows(g1[:m - 1], colsum, a0, n, k)


@pytest.mark.parametrize('shape', ref.SHAPES)
def test_linear_wgrad_x3_stacked(shape):
    """Three row-stacked planes: the gradient in order 3 [hi ; hi ; lo] (with its column sums) against the activation in order 4."""
    m, k, n = shape
    c = _case(shape)
    (g3, colsum), a4 = ops.split3([(dev(c['g']), 3, False, 0, None, True), (dev(c['a']), 4, False)])
    first, second = _wgrad_ref(shape, False)
    n_slabs = colsum.shape[0]
    dw, db = _modes(shape, lambda ow, ob, acc: ops.linear_wgrad_x3_stacked(g3, colsum, a4, n, k, out_w=ow, out_b=ob, accumulate=acc), first, second,
                    3 * m, lambda prior: ref.bias_grad(c['g'], n_slabs, prior=prior), 'wgrad stacked %s' % (shape,))
    dw2, db2 = ops.linear_wgrad_x3_stacked(g3, None, a4, n, k)
    assert db2 is None and torch.equal(dw2, dw)
    out_w, out_b = torch.full((n, k), SENTINEL, device=DEV), torch.full((n,), SENTINEL, device=DEV)
    _, db3 = ops.linear_wgrad_x3_stacked(g3, None, a4, n, k, out_w=out_w, out_b=out_b)
    assert db3 is None and torch.equal(out_w, dw) and bool((out_b == SENTINEL).all())
    with pytest.raises(ValueError):
        ops.linear_wgrad_x3_stacked(g3[:2], colsum, a4, n, k)


@pytest.mark.parametrize('gathered', [False, True])
@pytest.mark.parametrize('shape', ref.SHAPES)
def test_linear_wgrad_x3_planes(shape, gathered):
    """Separate planes (order 2), three accumulating launches; with a row map on the activation side (a table with zero rows behind
    it).  db = the column sums of hi + lo."""
    m, k, n = shape
    c = _case(shape)
    src, extra, rows = (c['table'], c['extra'], c['rows']) if gathered else (c['a'], 0, None)
    g2, a2 = ops.split3([(dev(c['g']), 2, False), (dev(src), 2, False, extra)])
    rows_dev = dev(rows) if gathered else None
    first, second = _wgrad_ref(shape, gathered)
    _modes(shape, lambda ow, ob, acc: ops.linear_wgrad_x3(g2, a2, rows_dev, m, n, k, out_w=ow, out_b=ob, accumulate=acc), first, second, 3 * m,
           lambda prior: ref.bias_grad(c['g'], 1, from_planes=True, prior=prior), 'wgrad planes %s gathered %d' % (shape, gathered))


@pytest.mark.parametrize('shape', ref.SHAPES)
def test_fused_sigmoid_gradient_split_then_wgrad(shape):
    """split3's fused sigmoid gradient (job element 5, ``sig``) followed by the weight gradient: the planes are the split of the fp32
    product g s (1 - s) in the kernel's order, bit for bit; dW and db are inside the bounds of that operand, and dW is within the
    derived bound of float64 g s (1 - s) (x3_ref64.wgrad_of_product)."""
    m, k, n = shape
    c = _case(shape)
    y32, y64, y_err = ref.sigmoid_grad(c['g'], c['s'])
    (g1, colsum), a0 = ops.split3([(dev(c['g']), 1, False, 0, dev(c['s']), True), (dev(c['a']), 0, False)])
    assert np.array_equal(_bits(g1), ref.plane_bits(y32, 1))
    _held(y32, Bounded(y64, y_err), 'sigmoid gradient %s (host fp32 product the planes equal)' % (shape,))
    dw, db = ops.linear_wgrad_x3_rows(g1, colsum, a0, n, k)
    first, second = ref.linear_wgrad(y32, c['a'])
    _held(dw, first, 'sigmoid-gradient wgrad %s, planes' % (shape,))
    _held(dw, ref.wgrad_of_product(y64, c['a'], first), 'sigmoid-gradient wgrad %s, float64 g s (1 - s)' % (shape,))
    _held(db, ref.bias_grad(y32, colsum.shape[0]), 'sigmoid-gradient db %s' % (shape,))
    # the separate-plane form takes the same fused split
    g2, a2 = ops.split3([(dev(c['g']), 2, False, 0, dev(c['s'])), (dev(c['a']), 2, False)])
    dw2, db2 = ops.linear_wgrad_x3(g2, a2, None, m, n, k)
    _held(dw2, first, 'sigmoid-gradient wgrad (planes form) %s' % (shape,))
    _held(db2, ref.bias_grad(y32, 1, from_planes=True), 'sigmoid-gradient db (planes form) %s' % (shape,))


def test_colsum_width_rule():
    """Which widths the column-sum split (and with it linear_wgrad_x3_rows in functional.LinearStackFn) takes: those whose 8-column
    chunks divide a workgroup.  96 and 100 pad to 128 columns and are taken; 130 and 160 pad to 192 (24 chunks) and are refused by
    split3 itself, so the row-interleaved form is never reached for them."""
    for n, ok in ((96, True), (100, True), (128, True), (512, True), (130, False), (160, False), (600, False)):
        assert ops.split3_colsum_ok(n) is ok, n
        x = torch.ones((4, n), dtype=torch.float32, device=DEV)
        if ok:
            planes, slabs = ops.split3([(x, 1, False, 0, None, True)])[0]
            got = ops.slab_reduce(slabs, slabs.shape[0], slabs.shape[1], n, torch.empty(n, device=DEV))
            assert bool((got == 4.0).all())
        else:
            with pytest.raises(ValueError):
                ops.split3([(x, 1, False, 0, None, True)])
