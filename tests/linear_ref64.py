"""Float64 restatement of the generic bf16 Linear entry points and the fused backward (gemm_bf16.hip, gemm_bf16_big.hip,
gemm_nt_runs.hip, bwd_fused_bf16.hip, bwd_fused64_bf16.hip) and of the fp32 entry points of gemm_f32.hip, one function per entry,
each computed from the operands THAT launch was given and each output a ``Bounded`` (value, per-element bound) - numpy only.

    linear_fwd       mg_linear_fwd_bf16 / mg_linear_fwd_f32                 Y = act(gather(A) W^T + b)
    linear_dgrad     mg_linear_dgrad_act_bf16 / _gathered_bf16 / _act_f32   dX = (dY W) f'(H[h_rows])
    linear_wgrad     mg_linear_wgrad[_slabs|_rows]_bf16 / _f32              dW = dY[dy_rows]^T gather(A), db = column sums (+ prior)
    fused_bwd        mg_linear_bwd_fused[_slabs|2_slabs]_bf16               dW1 | db1 from dZ2 (and dW2 | db2 for fused2)

Bounds (the project's existing ones, nothing new): a product accumulated in fp32 in ANY order g(K) sum |a||w| (phone_step_ref64.mm /
rows_product / rows_sum; K = rows + slabs for a sum finished over slabs, + 1 where ``accumulate`` adds a prior); FAST_SIGMOID_ABS for
mg_sigmoid_fast; ``b_tanh`` for tanhf; EPS of the magnitudes per elementwise fp32 operation, as ``Bounded`` arithmetic charges it, in
the kernels' association order - with ONE refinement that only tightens it: an operation on operands that carry no error whose
float64 result is representable in fp32 was exact (IEEE operations are correctly rounded), so it is charged nothing (``_mul`` /
``_sub``).  That keeps the ``exact`` family exact through the derivative epilogues.

Rounding points, read from the kernels:
* forward (gemm_nt_bf16_kernel, gemm_nt_big_kernel, gemm_nt_persist_kernel, gemm_nt_runs_kernel): the accumulators start from zero,
  the bias is added to the finished fp32 sum, the activation is applied in fp32 (mg_sigmoid_fast / tanhf / x < 0 ? 0 : x), ONE rounding
  to bf16 as the value is stored (none for an fp32 output).  Columns n .. ld of the output are written as zeros.  The small kernels
  contract over min(lda, ldw) columns, not K: the operands' padding columns must hold zeros (the generators' do).
* dgrad: sigmoid (v h) (1 - h), tanh v (1 - h h), ReLU h <= 0 ? 0 : v on the fp32 sum v with h the bf16 activation read as fp32;
  one rounding to bf16 as stored.
* weight gradients: bf16 operands, fp32 partial sums per split, slabs summed in fp32 (mg_slab_reduce_f32), never rounded to bf16.  db
  is summed from the bf16 dY (scalar adds in wgrad_bf16_kernel, a ones column through the matrix cores in the wide tiles).
* fused backward (wgrad_fused_kernel, wgrad_fused_pipe_kernel, wgrad_fused64_kernel<2|3>, wgrad_fused3_kernel): dZ1 = (d h) (1 - h)
  with d the fp32 sum over layer 2's 128 outputs, ROUNDED TO BF16 as it is stored to LDS; dW1 and db1 are formed from the rounded
  value (db1 through a ones column), dW2 | db2 of fused2 from the bf16 dZ2 and H1 as given.

``exact=True``: the caller's operands make every partial sum exactly representable in fp32 (``exact_condition``, asserted in the
``exact_*`` generators), so the products' bound is zero and a dropped, doubled or misplaced term shows in full.

DISPATCH.  ``fwd_program`` / ``dgrad_program`` / ``wgrad_program`` / ``fused_program`` return the NAME of the tile program a call
reaches, restating mg_try_nt_big, mg_try_nt_runs and the N <= 32 split; wgrad_plan_b, mg_wgrad_big_plan, wgrad_ksplit and
mg_launch_wgrad_big; fused_plan and fused_launch.  Where an entry point returns n_slabs and a stride the GPU tests assert the
restated plan against them; everywhere else this restatement is the ONLY statement of what ran - nothing in the library reports the
kernel chosen - which is why tests/test_linear_bf16_ref64_host.py keeps the table of shapes and programs."""
import numpy as np

from phone_step_ref64 import _grid, _row_weights, _up, exact_condition, g, mm, round_bf16, rows_product, rows_sum
from recurrent_ref64 import EPS, ETA, Bounded, b_sigmoid, b_tanh, bf16_round

F64 = np.float64
F32 = np.float32
ACT_NONE, ACT_SIGMOID, ACT_TANH, ACT_RELU = 0, 1, 2, 3
ACTS = (ACT_NONE, ACT_SIGMOID, ACT_TANH, ACT_RELU)
TUNE_FORM, TUNE_WGRAD_ORDER, TUNE_AB = 0, 5, 7          # keys of mg_set_tuning (include/morgana_hip.h)


def pad_ld(n):
    """ops.pad_ld: leading dimension of a bf16 buffer with n columns."""
    return (n + 63) // 64 * 64 if n >= 64 else (n + 7) // 8 * 8


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------ dispatch, restated
def _nt_big(m, kc, n_out, lda, ldb, ldc, out_f32, grad, form=0, ab=0):
    """mg_try_nt_big (gemm_bf16_big.hip): the program, or None where it does not take the shape.  kc = contraction length, n_out =
    output width; grad = a derivative epilogue with H."""
    if m < 2048 or lda % 64 or ldb % 64 or n_out % 128 or ldc != n_out or lda < _up(kc, 64) or ldb < _up(kc, 64):
        return None
    if ab == 98 and m < 32768:
        return None
    wide = n_out % 256 == 0
    if wide and ab != 97 and (ab == 99 or _cdiv(m, 256) * (n_out // 256) < 128):
        wide = False
    bn = 256 if wide else 128
    tiles_n = n_out // bn
    if not out_f32 and not grad and _cdiv(kc, 32) >= 5 and 32 % tiles_n == 0 and form != 6:
        return 'gemm_nt_persist_kernel<%d,%d>' % (bn, 32 if wide or form == 3 else 64)
    return 'gemm_nt_big_kernel<%d>' % bn


def fwd_program(m, k, n, lda, ldw, ldy, out_f32=False, rows=False, runs=False, form=0, ab=0):
    """mg_linear_fwd_bf16."""
    if runs and rows and not out_f32 and ldy == n and form != 14:
        if (m >= 2048 and n % 128 == 0 and lda % 64 == 0 and ldw % 64 == 0 and lda >= _up(k, 64) and ldw >= _up(k, 64) and
                _cdiv(k, 32) >= 5 and 64 % (n // 128) == 0):                                             # mg_try_nt_runs
            return 'gemm_nt_runs_kernel<ahead>' if form == 16 else 'gemm_nt_runs_kernel'
    big = _nt_big(m, k, n, lda, ldw, ldy, out_f32, False, form, ab) if ldy == n else None
    return big or ('gemm_nt_bf16_kernel<128,32>' if n <= 32 else 'gemm_nt_bf16_kernel<128,128>')


def dgrad_program(m, k, n, lddy, ldwt, lddx, out_f32=False, act=ACT_SIGMOID, form=0, ab=0):
    """mg_linear_dgrad_act_bf16 / mg_linear_dgrad_gathered_bf16 of a Linear(k -> n): contraction n, output width k."""
    big = _nt_big(m, n, k, lddy, ldwt, lddx, out_f32, act != ACT_NONE, form, ab) if lddx == k else None
    return big or ('gemm_nt_bf16_kernel<128,32>' if k <= 32 else 'gemm_nt_bf16_kernel<128,128>')


def wgrad_plan_small(m, n, k):
    """wgrad_plan_b (gemm_bf16.hip) -> (n_slabs, rows per slab, narrow)."""
    narrow = n <= 32
    tiles = _cdiv(n, 32 if narrow else 128) * _cdiv(k, 128)
    s = max(1, min(_cdiv(1024, tiles), _cdiv(m, 512), 65535))
    chunk = _up(_cdiv(m, s), 32)
    return max(1, _cdiv(m, chunk)), chunk, narrow


def wgrad_plan_f32(m, n, k):
    """wgrad_plan (gemm_f32.hip) -> (n_slabs, rows per slab, narrow)."""
    narrow = n <= 32
    tiles = _cdiv(n, 32 if narrow else 128) * _cdiv(k, 128)
    s = max(1, min(_cdiv(1024, tiles), _cdiv(m, 128 if tiles <= 2 else 512), 65535))
    chunk = _up(_cdiv(m, s), 16)
    return max(1, _cdiv(m, chunk)), chunk, narrow


def _ksplit(m, n, lda, ab=0):
    """wgrad_ksplit."""
    if ab == 92:
        return False
    if lda == 640:
        return m <= 32768 and n // 128 >= 4
    return lda == 512 and n == 128 and m <= 32768 and ab != 93


def wgrad_plan_big(m, n, k, lda, lddy, ab=0):
    """mg_wgrad_big_plan -> (n_slabs, rows per slab) or None (MG_TUNE_WGRAD_SPLITS at 0)."""
    if m < 4096 or n % 128 or lddy < n or lddy % 8:
        return None
    if not ((lda == 640 and 512 < k <= 640) or (lda == 512 and 384 < k <= 512)):
        return None
    tiles_n = n // 128
    s = _cdiv(256, tiles_n)
    if m <= 32768 and tiles_n >= 4:
        s = 192 // tiles_n
    if _ksplit(m, n, lda, ab):
        s = 256 // (2 * tiles_n) if lda == 640 else 48
    if m <= 32768 and tiles_n == 1:
        s = 96
    if m > 32768 and tiles_n == 1:
        s = 192
    one_round = False
    if m > 32768 and tiles_n > 1 and not _ksplit(m, n, lda, ab) and _up(s, 8) * tiles_n > 256 and tiles_n <= 128:
        s, one_round = 256 // tiles_n, True
    chunk = _up(_cdiv(m, s), 32)
    while chunk > 4096:
        s *= 2
        chunk = _up(_cdiv(m, s), 32)
    s = _cdiv(m, chunk)
    if not one_round:
        s = _up(s, 8)
    return (s, chunk) if s <= 65535 else None


def wgrad_program(m, k, n, lda, lddy, dy_rows=False, order=0, ab=0):
    """mg_linear_wgrad_bf16 / _slabs_ / _rows_ -> (program, n_slabs, slab stride in floats).  The rows entry and the slabs entry
    refuse what is not a wide-tile shape (program None)."""
    plan = wgrad_plan_big(m, n, k, lda, lddy, ab)
    if dy_rows:
        if plan is None or lda != 512 or _ksplit(m, n, lda, ab):
            return None, 0, 0
        return ('wgrad_big_rows_kernel<4,2>' if n % 256 == 0 and ab != 91 else 'wgrad_big_rows_kernel<8>'), plan[0], n * k + n
    if plan is None or order == 3:
        s, _, narrow = wgrad_plan_small(m, n, k)
        return ('wgrad_bf16_kernel<32,128>' if narrow else 'wgrad_bf16_kernel<128,128>'), s, n * k
    ks = _ksplit(m, n, lda, ab)
    if not ks and lda == 512 and n % 256 == 0 and ab != 91:
        prog = 'wgrad_big_kernel<4,2>'
    elif ks:
        prog = 'wgrad_big_kernel<4>' if lda == 512 else 'wgrad_big_kernel<5>'
    elif lda == 640 and n % 256 == 0 and ab != 91:
        prog = 'wgrad_big_kernel<5,2>'
    else:
        prog = 'wgrad_big_kernel<10>' if lda == 640 else 'wgrad_big_kernel<8>'
    return prog, plan[0], n * k + n


def fused_plan(m, n_hidden):
    """fused_plan (bwd_fused_bf16.hip) -> (n_slabs, frames per slab)."""
    s = _cdiv(256, n_hidden // 128)
    chunk = _up(_cdiv(m, s), 32)
    while chunk > 4096:
        s *= 2
        chunk = _up(_cdiv(m, s), 32)
    return _cdiv(m, chunk), chunk


def fused_program(rows=True, form=0, fused2=False):
    """fused_launch / mg_linear_bwd_fused2_slabs_bf16."""
    if fused2:
        return 'wgrad_fused3_kernel'
    if rows and form in (0, 12):
        return 'wgrad_fused64_kernel<%d>' % (2 if form == 12 else 3)
    return 'wgrad_fused_pipe_kernel' if rows and form != 7 else 'wgrad_fused_kernel'


FUSED64_AHEAD = 3            # bwd_fused64_bf16.hip: the product form fetches its tiles three 64-frame steps ahead (5 ring groups)


# ------------------------------------------------------------------------------------------------------------ elementwise fp32
def _is_f32(v):
    with np.errstate(over='ignore'):
        return v.astype(F32).astype(F64) == v


def _mul(a, b):
    a, b = Bounded.lift(a), Bounded.lift(b)
    v = a.v * b.v
    prop = a.e * np.abs(b.v) + np.abs(a.v) * b.e + a.e * b.e
    return Bounded(v, prop + np.where((prop == 0) & _is_f32(v), 0.0, EPS * np.abs(v) + ETA))


def _sub(a, b):
    a, b = Bounded.lift(a), Bounded.lift(b)
    v = a.v - b.v
    prop = a.e + b.e
    return Bounded(v, prop + np.where((prop == 0) & _is_f32(v), 0.0, EPS * (np.abs(a.v) + np.abs(b.v))))


def gather(a, rows, k):
    """a[rows][:, :k] in float64 with zero rows where rows < 0 (rows None: a[:, :k])."""
    a = np.asarray(a, dtype=F64)[:, :k]
    if rows is None:
        return a
    rows = np.asarray(rows)
    return np.where(rows[:, None] < 0, 0.0, a[np.maximum(rows, 0)])


def _store(b, out_f32):
    if out_f32:
        return b, 0.0
    return round_bf16(b)


# ------------------------------------------------------------------------------------------------------------ the entries
def linear_fwd(a, rows, w, bias, k, n, act, out_f32=False, exact=False, fast=True):
    """-> dict y [M, n] (Bounded), share (ambiguous share of a bf16 output).  fast: mg_sigmoid_fast (the bf16 kernels); the fp32
    kernels evaluate 1 / (1 + expf(-z))."""
    z = mm(Bounded(gather(a, rows, k)), np.asarray(w, dtype=F64)[:n, :k], bias, exact)
    if act == ACT_SIGMOID:
        z = b_sigmoid(z, fast=fast)
    elif act == ACT_TANH:
        z = b_tanh(z)
    elif act == ACT_RELU:
        z = Bounded(np.where(z.v < 0, 0.0, z.v), np.where(z.v + z.e < 0, 0.0, z.e))      # every value within the bound is negative: 0 exactly
    y, share = _store(z, out_f32)
    return {'y': y, 'share': share}


def linear_dgrad(dy, wt, h, k, n, act, out_f32=False, h_rows=None, exact=False):
    """dy [M, >=n], wt = W^T [k, >=n], h None or the activation's output [*, >=k] (read through h_rows).  -> dict dx [M, k], share."""
    v = mm(Bounded(np.asarray(dy, dtype=F64)[:, :n]), np.asarray(wt, dtype=F64)[:k, :n], None, exact)
    if h is not None and act != ACT_NONE:
        hh = np.asarray(h, dtype=F64)[:, :k]
        if h_rows is not None:
            hh = hh[np.asarray(h_rows)]
        if act == ACT_SIGMOID:
            v = _mul(_mul(v, hh), _sub(1.0, hh))
        elif act == ACT_TANH:
            v = _mul(v, _sub(1.0, _mul(hh, hh)))
        else:
            v = Bounded(np.where(hh <= 0, 0.0, v.v), np.where(hh <= 0, 0.0, v.e))
    dx, share = _store(v, out_f32)
    return {'dx': dx, 'share': share}


def plus_prior(b, prior, k_terms, exact):
    """b + prior as ``accumulate`` adds it: one more fp32 term (exact: the caller's prior keeps every partial sum representable)."""
    if prior is None:
        return b
    prior = np.asarray(prior, dtype=F64).reshape(b.v.shape)
    return Bounded(b.v + prior, b.e + (0.0 if exact else g(k_terms + 1) * np.abs(prior)))


def linear_wgrad(dy, a, rows, k, n, n_slabs, dy_rows=None, prior_w=None, prior_b=None, exact=False, units=None):
    """dW [n, k] (+ prior_w), db [n] (+ prior_b) over the rows of dy (or the index pairs dy_rows / rows; rows None: a[dy_rows]).
    ``units``: form dW for these output units only (db whole)."""
    if dy_rows is not None and rows is None:
        rows = dy_rows
    y = gather(dy, dy_rows, n)
    x = gather(a, rows, k)
    m = min(y.shape[0], x.shape[0])                        # rows None: the first rows of a (the zero rows behind a table stay out)
    y, x = y[:m], x[:m]
    k_terms = m + n_slabs
    yy = y if units is None else y[:, units]
    dw = plus_prior(rows_product(Bounded(yy), Bounded(x), k_terms, exact), prior_w, k_terms, exact)
    db = plus_prior(rows_sum(Bounded(y), k_terms, exact), prior_b, k_terms, exact)
    return {'dw': dw, 'db': db}


def fused_dz1(dz2, w2t, h1, n_hidden, exact=False, round_it=True):
    v = mm(Bounded(np.asarray(dz2, dtype=F64)[:, :128]), np.asarray(w2t, dtype=F64)[:n_hidden, :128], None, exact)
    hh = np.asarray(h1, dtype=F64)[:, :n_hidden]
    v = _mul(_mul(v, hh), _sub(1.0, hh))
    return round_bf16(v) if round_it else (v, 0.0)


def fused_bwd(dz2, w2t, h1, a, rows, n_hidden, k0, n_slabs, exact=False, exact_rows=False, units=None, second=False, round_dz1=True):
    """dz2 [M, >=128], w2t = W2^T [n_hidden, >=128], h1 [M, >=n_hidden], a the table [*, 640].  exact: the product dZ2 W2 is exact;
    exact_rows: so are the sums over frames of the ROUNDED dZ1 (the generator asserts both).  -> dw1, db1 (+ dw2, db2), share."""
    dz1, share = fused_dz1(dz2, w2t, h1, n_hidden, exact, round_dz1)
    x = gather(a, rows, k0)[:dz1.v.shape[0]]
    k_terms = x.shape[0] + n_slabs
    d = dz1 if units is None else Bounded(dz1.v[:, units], dz1.e[:, units])
    res = {'dw1': rows_product(d, Bounded(x), k_terms, exact_rows), 'db1': rows_sum(dz1, k_terms, exact_rows), 'share': share}
    if second:
        y, h = np.asarray(dz2, dtype=F64)[:, :128], np.asarray(h1, dtype=F64)[:, :n_hidden]
        res['dw2'] = rows_product(Bounded(y), Bounded(h), k_terms, exact_rows)
        res['db2'] = rows_sum(Bounded(y), k_terms, exact_rows)
    return res


# ------------------------------------------------------------------------------------------------------------ operands
def _padded(x, ld):
    out = np.zeros((x.shape[0], ld), dtype=F32)
    out[:, :x.shape[1]] = x
    return out


def row_map(kind, m, n_table, extra, seed=0):
    """Row maps into a table of n_table rows followed by ``extra`` zero rows: in-range rows, -1 and rows of the zero block.
    'mix' = every frame its own row; 'runs' = phone-like runs (1 to 39 frames) with -1 pads; 'short' = runs of 1 to 4; 'random' = no
    runs at all; 'one' = one long run; 'mixed' = stretches of every kind; 'pads' = all -1."""
    rng = np.random.RandomState(900 + seed)
    hi = n_table + extra

    def runs(count, longest):
        return np.repeat(rng.randint(-1, hi, size=count), rng.randint(1, longest, size=count))[:count]

    if kind == 'runs':
        r = runs(m, 40)
    elif kind == 'short':
        r = runs(m, 5)
    elif kind in ('random', 'mix'):
        r = rng.randint(-1, hi, size=m)
    elif kind == 'one':
        r = np.full(m, 7)
    elif kind == 'pads':
        r = np.full(m, -1)
    else:
        parts, left = [], m
        while left > 0:
            c = min(left, int(rng.randint(50, 400)))
            parts.append(runs(c, (40, 5, 2, 400)[rng.randint(0, 4)]))
            left -= c
        r = np.concatenate(parts)
    r = r.astype(np.int32)
    if kind not in ('one', 'pads'):                      # every kind of row is present, and the LAST frame is a live one
        r[0], r[1], r[2], r[m - 1] = -1, n_table + extra - 1, 0, n_table - 1
    return r


def _rows_condition(y, gy, a, ga):
    """exact_condition for sums over the rows of y [M, N] against ANY gather of the rows of a (zero rows included) and against ones
    (the bias sums): every |a| is at most amax, a grid value, so sum_m |y[m, i]| amax bounds every gathered sum.  Returns it."""
    a = np.asarray(a, dtype=F64)
    amax = float(np.abs(a).max())
    assert np.array_equal(a * 2.0 ** ga, np.round(a * 2.0 ** ga)) and np.array_equal(bf16_round(a), a)
    return max(exact_condition(y, gy, np.full((np.asarray(y).shape[0], 1), max(amax, 2.0 ** -ga)), ga, over_rows=True),
               exact_condition(y, gy, np.ones((np.asarray(y).shape[0], 1)), 0, over_rows=True))


def exact_fwd(m, k, n, lda=None, n_table=None, extra=0, seed=0):
    """A in +-j/64, W in +-j/4096 (|j| <= 127), bias in j/2^18: A W^T + b exact in fp32 in any order (asserted).  A is a table of
    n_table (default m) rows plus ``extra`` zero rows, lda wide with zero padding columns."""
    rng = np.random.RandomState(11000 + seed)
    lda = pad_ld(k) if lda is None else lda
    n_table = m if n_table is None else n_table
    a = np.zeros((n_table + extra, lda), dtype=F32)
    a[:n_table, :k] = _grid(rng, -63, 63, (n_table, k), 6)
    c = {'a': a, 'w': _padded(_grid(rng, -127, 127, (n, k), 12), lda), 'bias': _grid(rng, -26000, 26000, n, 18)}
    c['sum_abs'] = exact_condition(a, 6, c['w'], 12, c['bias'])
    return c


def wide_fwd(m, k, n, lda=None, n_table=None, extra=0, seed=0):
    """W in +-0.1, activations in (0, 1), bias +-0.1."""
    rng = np.random.RandomState(12000 + seed)
    lda = pad_ld(k) if lda is None else lda
    n_table = m if n_table is None else n_table
    a = np.zeros((n_table + extra, lda), dtype=F32)
    a[:n_table, :k] = bf16_round(rng.uniform(0, 1, (n_table, k)).astype(F32))
    return {'a': a, 'w': _padded(bf16_round(rng.uniform(-0.1, 0.1, (n, k)).astype(F32)), lda), 'bias': rng.uniform(-0.1, 0.1, n).astype(F32)}


def scaled_grads(rng, m, n, bf16=True):
    """Normal gradients times 0.01 to 1: the rows' scales spread over e^+-3, one row in ten zero, the last row live and heavy.
    bf16=False: full fp32 values (the fp32 entry points)."""
    x = (rng.standard_normal((m, n)) * 0.01 * (_row_weights(rng, m) * m)[:, None]).astype(F32)
    return bf16_round(x) if bf16 else x


_scaled_grads = scaled_grads


def exact_dgrad(m, k, n, h_table=None, seed=0):
    """dY in +-j/32, W^T in +-j/256 (|j| <= 20), H in j/16 (0 < j < 16) or, for tanh / ReLU, +-j/16 with zeros: dY W is exact
    (asserted) and so, on nearly every element, are (v h)(1 - h) and v (1 - h h)."""
    rng = np.random.RandomState(13000 + seed)
    c = {'dy': _padded(_grid(rng, -31, 31, (m, n), 5), pad_ld(n)), 'wt': _padded(_grid(rng, -20, 20, (k, n), 8), pad_ld(n)),
         'h': _padded(_grid(rng, 1, 15, (h_table or m, k), 4), pad_ld(k)), 'hs': _padded(_grid(rng, -15, 15, (h_table or m, k), 4), pad_ld(k))}
    c['sum_abs'] = exact_condition(c['dy'], 5, c['wt'], 8)
    return c


def wide_dgrad(m, k, n, h_table=None, seed=0):
    rng = np.random.RandomState(14000 + seed)
    return {'dy': _padded(_scaled_grads(rng, m, n), pad_ld(n)), 'wt': _padded(bf16_round(rng.uniform(-0.1, 0.1, (k, n)).astype(F32)), pad_ld(n)),
            'h': _padded(bf16_round(rng.uniform(0.05, 0.95, (h_table or m, k)).astype(F32)), pad_ld(k)),
            'hs': _padded(bf16_round(rng.uniform(-0.95, 0.95, (h_table or m, k)).astype(F32)), pad_ld(k))}


def exact_wgrad(m, k, n, lda=None, n_table=None, extra=0, seed=0):
    """dY in +-j/32, A in +-j/32, the priors in j/1024: dW, db over m rows and the sum with a prior exact (asserted: multiples of
    2^-10 with sum |terms| + |prior| < 2^14)."""
    rng = np.random.RandomState(15000 + seed)
    lda = pad_ld(k) if lda is None else lda
    n_table = m if n_table is None else n_table
    a = np.zeros((n_table + extra, lda), dtype=F32)
    a[:n_table, :k] = _grid(rng, -31, 31, (n_table, k), 5)
    c = {'dy': _padded(_grid(rng, -31, 31, (m, n), 5), pad_ld(n)), 'a': a, 'prior_w': _grid(rng, -4000, 4000, (n, k), 10),
         'prior_b': _grid(rng, -4000, 4000, n, 10)}
    worst = _rows_condition(c['dy'], 5, a, 5)
    assert worst + 4.0 < 2.0 ** 14, worst
    c['sum_abs'] = worst
    return c


def wide_wgrad(m, k, n, lda=None, n_table=None, extra=0, seed=0):
    rng = np.random.RandomState(16000 + seed)
    lda = pad_ld(k) if lda is None else lda
    n_table = m if n_table is None else n_table
    a = np.zeros((n_table + extra, lda), dtype=F32)
    a[:n_table, :k] = bf16_round(rng.uniform(0, 1, (n_table, k)).astype(F32))
    return {'dy': _padded(_scaled_grads(rng, m, n), pad_ld(n)), 'a': a, 'prior_w': rng.standard_normal((n, k)).astype(F32),
            'prior_b': rng.standard_normal(n).astype(F32)}


def exact_fused(m, n_hidden, k0, n_table, extra=64, seed=0):
    """dZ2 with ONE nonzero per frame (+-1/2 or +-1), W2 in +-j/256 (|j| <= 16), H1 in {1/4, 1/2, 3/4}, the table in j/8 (j < 8): dZ2 W2 is a
    single product, (v h)(1 - h) has at most 7 significant bits, so the bf16 dZ1 IS the float64 value, a multiple of 2^-13; with the
    table its sums over frames are exact (asserted for the worst gather).  dZ2's second-layer sums (fused2) are exact too."""
    rng = np.random.RandomState(17000 + seed)
    dz2 = np.zeros((m, 128), dtype=F32)
    dz2[np.arange(m), rng.randint(0, 128, m)] = rng.choice([-1.0, -0.5, 0.5, 1.0], m)
    a = np.zeros((n_table + extra, 640), dtype=F32)
    a[:n_table, :k0] = _grid(rng, 0, 7, (n_table, k0), 3)
    c = {'dz2': dz2, 'w2t': _padded(_grid(rng, -16, 16, (n_hidden, 128), 8), 128), 'h1': _padded(rng.choice([0.25, 0.5, 0.75], (m, n_hidden)).astype(F32), pad_ld(n_hidden)),
         'a': a}
    exact_condition(dz2, 1, c['w2t'], 8)
    dz1, share = fused_dz1(dz2, c['w2t'], c['h1'], n_hidden, exact=True)
    assert share == 0.0 and not dz1.e.any()
    c['sum_abs'] = _rows_condition(bf16_round(dz1.v), 13, a, 3)
    _rows_condition(dz2, 1, c['h1'][:, :n_hidden], 2)
    return c


def wide_fused(m, n_hidden, k0, n_table, extra=64, seed=0):
    """W2 in +-0.1, H1 in (0.05, 0.95), the table in (0, 1), dZ2 normal times 0.01 to 1 with one row in ten zero."""
    rng = np.random.RandomState(18000 + seed)
    a = np.zeros((n_table + extra, 640), dtype=F32)
    a[:n_table, :k0] = bf16_round(rng.uniform(0, 1, (n_table, k0)).astype(F32))
    return {'dz2': _scaled_grads(rng, m, 128), 'w2t': bf16_round(rng.uniform(-0.1, 0.1, (n_hidden, 128)).astype(F32)),
            'h1': _padded(bf16_round(rng.uniform(0.05, 0.95, (m, n_hidden)).astype(F32)), pad_ld(n_hidden)), 'a': a}


def unit_subset(n, seed=0):
    """Output units a reference may be restricted to: the first and the last unit of every 128-unit tile and 64 others."""
    edges = sorted({t * 128 for t in range(_cdiv(n, 128))} | {min(n, t * 128 + 128) - 1 for t in range(_cdiv(n, 128))})
    rest = np.setdiff1d(np.arange(n), edges)
    more = np.random.RandomState(19000 + seed).choice(rest, size=min(64, rest.size), replace=False)
    return np.sort(np.concatenate([np.asarray(edges, dtype=np.int64), more]))
