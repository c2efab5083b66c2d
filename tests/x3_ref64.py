"""Float64 references, each element with a DERIVED fp32 bound, of two pieces of hot-path arithmetic:

* the generic 'bf16x3' Linear products (ops.linear_fwd_x3 / linear_dgrad_x3 / linear_wgrad_x3_rows / _stacked / linear_wgrad_x3 on
  the three-plane buffers of csrc/split3.hip), and
* the update as the last node of a step (mg_adam_step_plan_f32, adam_plan_kernel in csrc/optim.hip).

Plain numpy, no GPU and no torch.  ``gamma``, ``bf16_round``, ``Bounded`` and ``ratio`` are those of tests/recurrent_ref64.py.

Split-operand products.  x = hi + lo with hi = bf16(x), lo = bf16(x - hi); a bf16 value is exact in float64, and so is each product
of two of them in the fp32 accumulator of a bf16 MFMA.  The kernels contract ONE index of length 3 ldp over the planes the layouts
pair - (hi, hi), (hi, lo), (lo, hi) - so the reference forms exactly those three products in float64: the kernel's arithmetic with
only the fp32 accumulation removed.  An fp32 sum of T products plus a bias in ANY order is within gamma(T + 2) (sum |a||w| + |bias|)
of it: T = 3 ldp for forward and dgrad (padding columns are terms too: zeros, added exactly), T = 3 m for a weight gradient, which
contracts over the rows - whatever the split over M, the slab reduce or the three accumulating launches of linear_wgrad_x3 do to
the order.  ``accumulate=True`` makes the destination's prior content one more term of the same sum: gamma(T + 3) (sum + |prior|).
Activations: sigmoid through its derivative (<= 1/4) plus three fp32 operations' worth on the output plus the absolute error the
hardware-exp form documents (common.h: mg_sigmoid_fast, v_exp_f32 + v_rcp_f32; the figure is gru_cell.h's, FAST_SIGMOID_ABS) - the
bf16 tile programs use that form with an fp32 output as well; tanh (tanhf) through its derivative (<= 1) plus three operations'
worth; ReLU is 1-Lipschitz and exact.

The bias gradient.  linear_wgrad_x3_rows / _stacked: the column sums of the fp32 gradient itself (split3's ``colsum`` slabs, one per
workgroup, then the slab reduce): m terms in n_slabs partial sums, gamma(m + n_slabs) sum |g|.  linear_wgrad_x3: the column sums of
hi + lo, taken by the weight-gradient launches of the hi and of the lo plane; bounded with the SAME expression at n_slabs = 1, the
least a launch can cut (the strictly order-independent count of that form is 2 m terms; the figure used is up to twice as tight).

The second figure of every product: its distance from float64 arithmetic on the ORIGINAL fp32 operands, bounded by the first bound
plus 2^-16 sum |a||w| - the mode's published precision claim (tests/test_gpu_activations.py: _eps) for the dropped lo lo term and the
two split remainders x - hi - lo.  (|lo| <= 2^-8 |x| and |x - hi - lo| <= 2^-9 |lo|: operands whose lo planes all sit at the full
2^-8 with one sign would reach 2^-16 with the lo lo term alone; ``make_case`` keeps |lo| <= 0.6 * 2^-8 |x|, 0.36 * 2^-16 for that term
and 0.6 * 2^-17 per remainder, and ordinary operands stay far below.)  It does not know the planes, so a plane order the first
reference might mirror cannot hide from it.

The update.  g = grad + sum over sources and slabs, in float64 from the fp32 inputs; T_i = 1 + the slabs that cover element i terms in
any order: gamma(T_i + 1) (|grad| + sum |slab values|).  Then mg_adam_update's documented order (optim.hip) on ``Bounded`` values -
g *= grad_scale; g = fma(weight_decay, p, g) unless weight_decay == 0; m = fma(g - m, 1 - beta1, m); v = fma((1 - beta2) g, g,
v beta2); denom = sqrt(v) / bc2_sqrt + eps; p -= step_size (m / denom) - with the FLOAT32 scalars the kernel receives (ops.adam_scalars;
1 - beta in fp32 as the kernel forms it).  A fused multiply-add is charged as the two operations it replaces.  sqrt and the
division carry their first-order sensitivities (``b_sqrt``, ``b_div``): d sqrt(v) <= e / (2 sqrt(v - e)), and never more than sqrt(e);
d (a / b) <= e_a / (|b| - e_b) + |a| e_b / (|b| (|b| - e_b)) - the sensitivity of p to g through 1 / denom.

The bf16 operand copies (``shadow_bits``) are exact functions of the DEVICE's fp32 parameter - bf16(p), and for pair planes
bf16(p - hi) - asserted bit for bit from the value the test has just bounded, never re-derived from the float64 p."""
import numpy as np

from recurrent_ref64 import EPS, FAST_SIGMOID_ABS, F64, U, Bounded, b_sigmoid, b_tanh, bf16_bits, bf16_round, gamma, ratio  # noqa: F401

LOLO = 2.0 ** -16          # the dropped lo lo term and the split remainders, relative to sum |a||w|: the PUBLISHED figure (the derived
                           # worst case is SPLIT_WORST below, used where the operand's mantissas are not the test's to choose)
ACT_NONE, ACT_SIGMOID, ACT_TANH, ACT_RELU = 0, 1, 2, 3          # MG_ACT_* of include/morgana_hip.h


def pad_ld(n):
    """ops.pad_ld: the leading dimension of a plane with n columns."""
    return (n + 63) // 64 * 64 if n >= 64 else (n + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------------------ inputs
SHAPES = ((130, 40, 96), (777, 609, 256), (64, 600, 512), (4100, 600, 512), (4999, 128, 512), (2049, 620, 128), (5, 9, 100))
EXTRA = 8            # zero rows behind a gathered table (the rows padding frames map to)


def heavy_lo(rng, shape, row_exp=None, sign=None):
    """fp32 values whose lo planes carry real weight and do not cancel: 2^E (1 + (j + f) / 128) with j in 0..15 (hi's mantissa, exact in
    bf16) and f in [0.22, 0.30] of a bf16 ulp (lo): |lo| / |x| lies in [1.5e-3, 2.4e-3] = [0.39, 0.60] * 2^-8 everywhere.  E: one
    exponent per row, round(u / ln 2) with u uniform in [-3, 3] (row scales spread over e^+-3, as test_split3_planes'), or ``row_exp``.
    ``sign``: +-1 broadcast against the shape, None = all positive.  With one sign along the contraction index every lo hi term of a
    product has the same sign, so a dropped or mispaired cross term moves the result by >= 1.5e-3 of sum |a||w| - against a bound of
    gamma(T + 2) sum |a||w|, 1.15e-4 at T = 1920 - while the dropped lo lo term stays below 0.36 * 2^-16 of it (the looser figure's
    allowance; lo planes at the full 2^-8 with one sign would use all of it on their own)."""
    rows, cols = shape
    e = np.round(rng.uniform(-3, 3, (rows, 1)) / np.log(2.0)) if row_exp is None else np.asarray(row_exp, dtype=F64).reshape(rows, 1)
    x = 2.0 ** e * (1.0 + (rng.randint(0, 16, shape) + rng.uniform(0.22, 0.30, shape)) / 128.0)
    if sign is not None:
        x = x * sign
    return x.astype(np.float32)


def make_case(shape, seed=0, heavy=True):
    """The operands of one (m, k, n) case of the GPU test (and of the host test's sensitivity check): activations a (m, k) > 0,
    weights w (n, k) and gradients g (m, n) signed per output feature (one sign along k for the forward, along n for the dgrad, along
    the rows for the weight gradient), bias (n,), sigmoid outputs s (m, n), and a gathered form - table (R, k), EXTRA zero rows behind
    it, rows (m,) int32 with entries in the table, in the zero rows (padding frames) and < 0.
    ``heavy`` False: ordinary operands instead - standard normal times a row scale e^u, u uniform in [-3, 3] (test_split3_planes') -
    for the host test's float32 evaluations, whose headroom figures describe the bounds, not these inputs."""
    m, k, n = shape
    rng = np.random.RandomState(1000 * seed + m + 3 * k + 7 * n)
    sn = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    if heavy:
        make = lambda shp, sign=None: heavy_lo(rng, shp, sign=sign)
    else:
        make = lambda shp, sign=None: (rng.standard_normal(shp) * np.exp(rng.uniform(-3, 3, (shp[0], 1)))).astype(np.float32)
    a = make((m, k))
    w = make((n, k), sign=sn[:, None])
    g = make((m, n), sign=sn[None, :])
    bias = (rng.standard_normal(n) * 0.25 * k * 2.0 ** np.round(rng.uniform(-3, 3, n) / np.log(2.0))).astype(np.float32)
    s = rng.uniform(0.02, 0.98, (m, n)).astype(np.float32)
    r = max(m // 7, 2)
    table = make((r, k))
    rows = rng.randint(-1, r + EXTRA, size=m).astype(np.int32)
    rows[:3] = (r - 1, r, r + EXTRA - 1)[:min(3, m)]          # the last table row, the first and the last zero row
    return {'a': a, 'w': w, 'g': g, 'bias': bias, 's': s, 'table': table, 'rows': rows, 'extra': EXTRA}


def make_activation_case(shape, seed=0):
    """Ordinary operands with pre-activations of order 1, for the activation epilogues: a uniform in (0, 1), w uniform in
    (-1, 1) 3 / sqrt(k) (a pre-activation of about unit spread), bias normal 0.5 - sigmoid and tanh in their steep part and a ReLU
    with both branches, under a bound of gamma(3 ldp + 2) 0.75 sqrt(k), 7e-6 at k = 9 to 2e-3 at k = 600, before the derivative."""
    m, k, n = shape
    rng = np.random.RandomState(77 + 1000 * seed + m + 3 * k + 7 * n)
    return {'a': rng.uniform(0, 1, (m, k)).astype(np.float32), 'w': (rng.uniform(-1, 1, (n, k)) * 3 / np.sqrt(k)).astype(np.float32),
            'bias': (rng.standard_normal(n) * 0.5).astype(np.float32)}


# ------------------------------------------------------------------------------------------------------------ the split
def split(x):
    """fp32 array -> (hi, lo) as float64 VALUES: hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in fp32)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_round(x)
    lo = bf16_round((x - hi).astype(np.float32))
    return hi.astype(F64), lo.astype(F64)


def plane_bits(x, order, transpose=False, extra=0):
    """The bf16 bit patterns mg_split3_bf16 writes for fp32 ``x`` (rows, cols): orders 0 / 1 -> (rows + extra, 3 ldp) = [hi | hi | lo] /
    [hi | lo | hi]; order 2 -> (2, rows + extra, ldp) = [hi ; lo]; orders 3 / 4 -> (3, rows + extra, ldp) = [hi ; hi ; lo] / [hi ; lo ; hi];
    ``transpose``: of x^T.  Padding columns and the extra rows are zero."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).T if transpose else x, dtype=np.float32)
    hi = bf16_round(x)
    hb, lb = bf16_bits(hi), bf16_bits((x - hi).astype(np.float32))
    rows, cols = x.shape
    ldp = pad_ld(cols)
    planes = {0: (hb, hb, lb), 1: (hb, lb, hb), 2: (hb, lb), 3: (hb, hb, lb), 4: (hb, lb, hb)}[order]
    if order >= 2:
        out = np.zeros((len(planes), rows + extra, ldp), dtype=np.uint16)
        for q, p in enumerate(planes):
            out[q, :rows, :cols] = p
    else:
        out = np.zeros((rows + extra, 3 * ldp), dtype=np.uint16)
        for q, p in enumerate(planes):
            out[:rows, q * ldp:q * ldp + cols] = p
    return out


def _gather(x, rows, extra=0):
    """x (R, K) with ``extra`` zero rows behind it, gathered by ``rows`` (None: all R + extra rows; an entry < 0: a zero row)."""
    x = np.asarray(x, dtype=F64)
    if extra:
        x = np.concatenate([x, np.zeros((extra, x.shape[1]))])
    if rows is None:
        return x
    rows = np.asarray(rows)
    return np.where(rows[:, None] < 0, 0.0, x[np.maximum(rows, 0)])


def _three(ah, al, bh, bl, t=False):
    """(value, magnitude) of ah bh + ah bl + al bh over the shared index; t: contract the FIRST axes (X^T Y), else (X Y^T)."""
    if t:
        mm = lambda x, y: x.T @ y
    else:
        mm = lambda x, y: x @ y.T
    value = mm(ah, bh + bl) + mm(al, bh)                       # hi + lo of two bf16 values is exact in float64
    mag = mm(np.abs(ah), np.abs(bh) + np.abs(bl)) + mm(np.abs(al), np.abs(bh))
    return value, mag


def activate(pre, act):
    """A Bounded pre-activation through activation ``act`` (the bounds of the module docstring)."""
    if act == ACT_NONE:
        return pre
    if act == ACT_SIGMOID:
        return b_sigmoid(pre, fast=True)
    if act == ACT_TANH:
        return b_tanh(pre)
    if act == ACT_RELU:
        return Bounded(np.maximum(pre.v, 0.0), pre.e)
    raise ValueError(act)


def _act64(v, act):
    if act == ACT_SIGMOID:
        with np.errstate(over='ignore'):
            return 1.0 / (1.0 + np.exp(-v))
    return np.tanh(v) if act == ACT_TANH else np.maximum(v, 0.0) if act == ACT_RELU else v


# ------------------------------------------------------------------------------------------------------------ the three products
def linear_fwd(a, w, bias, act=ACT_NONE, rows=None, extra=0, pairs='x3'):
    """act(gather(A, rows) W^T + bias): a (R, K) fp32 (``extra`` zero rows behind it), w (N, K) fp32, bias (N,) or None.
    Returns (Bounded from the split planes, Bounded from the original operands).  ``pairs`` exists for the sensitivity checks of the
    host test: 'x3' = the three products; 'no_lohi' / 'no_hilo' omit one; 'lolo' pairs (lo, lo) where the layout pairs (lo, hi)."""
    ah, al = split(a)
    wh, wl = split(w)
    ah, al = _gather(ah, rows, extra), _gather(al, rows, extra)
    b = np.zeros(w.shape[0]) if bias is None else np.asarray(bias, dtype=F64)
    value, mag = _three(ah, al, wh, wl)
    if pairs == 'no_lohi':
        value = ah @ (wh + wl).T
    elif pairs == 'no_hilo':
        value = ah @ wh.T + al @ wh.T
    elif pairs == 'lolo':
        value = ah @ (wh + wl).T + al @ wl.T
    elif pairs != 'x3':
        raise ValueError(pairs)
    terms = 3 * pad_ld(w.shape[1])
    pre = Bounded(value + b, gamma(terms + 2) * (mag + np.abs(b)))
    a64 = _gather(np.asarray(a, dtype=F64), rows, extra)
    w64 = np.asarray(w, dtype=F64)
    pre2 = Bounded(a64 @ w64.T + b, pre.e + LOLO * (np.abs(a64) @ np.abs(w64).T))
    return activate(pre, act), activate(pre2, act)


def linear_dgrad(g, w):
    """dX = dY W: g (M, N) fp32 split [hi | lo | hi], w (N, K) fp32 whose transpose is split [hi | hi | lo].  Returns the two Bounded."""
    gh, gl = split(g)
    wh, wl = split(w)
    value, mag = _three(gh, gl, wh.T, wl.T)                    # (gh, wh) + (gh, wl) + (gl, wh): the pairs of order 1 against order 0
    first = Bounded(value, gamma(3 * pad_ld(g.shape[1]) + 2) * mag)
    g64, w64 = np.asarray(g, dtype=F64), np.asarray(w, dtype=F64)
    return first, Bounded(g64 @ w64, first.e + LOLO * (np.abs(g64) @ np.abs(w64)))


def linear_wgrad(g, a, rows=None, extra=0, pairs='x3'):
    """dW = dY^T gather(A, rows): g (M, N) fp32, a (R, K) fp32.  The same three products in every device form ((hi, hi), (hi, lo),
    (lo, hi) as (gradient, activation) planes).  Returns the two Bounded (``add_prior`` makes them those of accumulate=True).
    ``pairs``: as linear_fwd, for the sensitivity checks ('no_lohi' drops (gradient lo, activation hi))."""
    gh, gl = split(g)
    ah, al = split(a)
    ah, al = _gather(ah, rows, extra), _gather(al, rows, extra)
    value, mag = _three(gh, gl, ah, al, t=True)
    if pairs == 'no_lohi':
        value = gh.T @ (ah + al)
    elif pairs == 'no_hilo':
        value = (gh + gl).T @ ah
    elif pairs == 'lolo':
        value = gh.T @ (ah + al) + gl.T @ al
    elif pairs != 'x3':
        raise ValueError(pairs)
    first = Bounded(value, gamma(3 * g.shape[0] + 2) * mag)
    g64, a64 = np.asarray(g, dtype=F64), _gather(np.asarray(a, dtype=F64), rows, extra)
    return first, Bounded(g64.T @ a64, first.e + LOLO * (np.abs(g64).T @ np.abs(a64)))


def add_prior(first, second, prior, terms):
    """The two Bounded of a ``terms``-term weight gradient accumulated onto ``prior`` (accumulate=True): the prior content is one more
    term of the same any-order sum, gamma(terms + 3) (sum |g||a| + |prior|); the looser figure keeps its 2^-16 part."""
    prior = np.asarray(prior, dtype=F64)
    mag = first.e / gamma(terms + 2)
    new_first = Bounded(prior + first.v, gamma(terms + 3) * (mag + np.abs(prior)))
    return new_first, Bounded(prior + second.v, new_first.e + (second.e - first.e))


def bias_grad(g, n_slabs, from_planes=False, prior=None):
    """db: the column sums of the fp32 gradient (``from_planes`` False: split3's colsum, n_slabs partial sums) or of hi + lo (True:
    linear_wgrad_x3; pass n_slabs = 1).  Bound gamma(m + n_slabs) sum |g| (+ the prior content as one more term)."""
    if from_planes:
        hi, lo = split(g)
        x, mag = hi + lo, (np.abs(hi) + np.abs(lo)).sum(axis=0)
    else:
        x = np.asarray(g, dtype=F64)
        mag = np.abs(x).sum(axis=0)
    m = x.shape[0]
    if prior is None:
        return Bounded(x.sum(axis=0), gamma(m + n_slabs) * mag)
    prior = np.asarray(prior, dtype=F64)
    return Bounded(prior + x.sum(axis=0), gamma(m + n_slabs + 1) * (mag + np.abs(prior)))


def sigmoid_grad(g, s):
    """The fused sigmoid-gradient split's operand: (the fp32 values g * s * (1 - s) in the kernel's product order - exact inputs of
    the products that follow, for the first reference; the float64 product; the bound of its fp32 evaluation: three operations, EPS each)."""
    g32, s32 = np.asarray(g, dtype=np.float32), np.asarray(s, dtype=np.float32)
    y32 = g32 * s32 * (np.float32(1) - s32)
    y64 = np.asarray(g, dtype=F64) * np.asarray(s, dtype=F64) * (1.0 - np.asarray(s, dtype=F64))
    return y32, y64, 3 * EPS * np.abs(y64) + 2.0 ** -149


SPLIT_WORST = 2.0 ** -15   # the same claim as LOLO, as a worst case: |lo_a lo_w| <= 2^-16 |a||w|, the remainders |x - hi - lo| <= 2^-9 |lo| <= 2^-17 |x| each, cross terms < 2^-24


def wgrad_of_product(y64, a, first):
    """The weight gradient of the fused sigmoid gradient against float64 arithmetic on y64 = g s (1 - s) itself: ``first`` (the bound
    of the products of the fp32 values' planes) plus the fp32 evaluation of y (3 EPS) plus the split's DERIVED worst case 2^-15 -
    y's mantissas are not the test's to choose, so the published 2^-16 (an average-case figure) does not bound a sum that one row
    dominates."""
    a64 = np.asarray(a, dtype=F64)
    return Bounded(y64.T @ a64, first.e + (SPLIT_WORST + 3 * EPS) * (np.abs(y64).T @ np.abs(a64)))


# ------------------------------------------------------------------------------------------------------------ the update
def b_sqrt(x):
    v = np.sqrt(x.v)
    with np.errstate(divide='ignore', invalid='ignore'):
        lo = np.sqrt(np.maximum(x.v - x.e, 0.0))
        first = np.where(x.e == 0, 0.0, np.where(lo > 0, x.e / (2 * lo), np.inf))
    return Bounded(v, np.minimum(first, np.sqrt(x.e)) + EPS * v)


def b_div(a, b):
    a, b = Bounded.lift(a), Bounded.lift(b)
    v = a.v / b.v
    lo = np.abs(b.v) - b.e
    with np.errstate(divide='ignore', invalid='ignore'):
        e = np.where(lo > 0, a.e / lo + np.abs(a.v) * b.e / (np.abs(b.v) * lo), np.inf)
    return Bounded(v, e + EPS * np.abs(v))


def f32(x):
    return float(np.float32(x))


def summed_gradient(grad, sources):
    """g = grad + sum_sources sum_slabs slab[s, i - begin] as a Bounded; sources = [(begin, count, slabs (n_slabs, >= count) array)]."""
    total = np.asarray(grad, dtype=F64).copy()
    mag = np.abs(total)
    terms = np.ones(total.shape)
    for begin, count, slabs in sources:
        s = np.asarray(slabs, dtype=F64)[:, :count]
        total[begin:begin + count] += s.sum(axis=0)
        mag[begin:begin + count] += np.abs(s).sum(axis=0)
        terms[begin:begin + count] += s.shape[0]
    return Bounded(total, gamma(terms + 1) * mag)


def adam_update(param, g, exp_avg, exp_avg_sq, betas, eps, weight_decay, scalars, grad_scale=1.0):
    """mg_adam_update on Bounded values.  g: Bounded (``summed_gradient``) or an fp32 array; scalars = (step_size, bc2_sqrt) float32.
    Returns Bounded (p, m, v)."""
    one = np.float32(1)
    b1, b2 = np.float32(betas[0]), np.float32(betas[1])
    omb1, omb2 = float(one - b1), float(one - b2)              # 1.f - beta, as the kernel forms it
    step_size, bc2_sqrt = f32(scalars[0]), f32(scalars[1])
    p, m, v = Bounded(np.asarray(param, dtype=F64)), Bounded(np.asarray(exp_avg, dtype=F64)), Bounded(np.asarray(exp_avg_sq, dtype=F64))
    g = Bounded.lift(g) * f32(grad_scale)
    if f32(weight_decay) != 0.0:
        g = p * f32(weight_decay) + g
    m = (g - m) * omb1 + m
    v = (g * omb2) * g + v * float(b2)
    denom = b_div(b_sqrt(v), bc2_sqrt) + f32(eps)
    p = p - b_div(m, denom) * step_size
    return p, m, v


def adam_plan(param, grad, exp_avg, exp_avg_sq, betas, eps, weight_decay, scalars, grad_scale=1.0, sources=()):
    return adam_update(param, summed_gradient(grad, sources), exp_avg, exp_avg_sq, betas, eps, weight_decay, scalars, grad_scale)


def adam_scalars(lr, betas, step):
    """(step_size, bc2_sqrt) as mg_adam_scalars forms them: lr and the betas arrive as float32, the arithmetic is the host's double, the
    results are rounded to float32 (for the host test; GPU tests take ops.adam_scalars, and test_gpu_adam_plan.py compares the two)."""
    lr, b1, b2 = f32(lr), f32(betas[0]), f32(betas[1])
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return np.float32(lr / bc1), np.float32(np.sqrt(bc2))


def shadow_bits(p_dev, offset, rows, cols):
    """(hi, lo) bf16 bit patterns (rows, cols) of the DEVICE's fp32 parameters p_dev[offset : offset + rows cols]."""
    w = np.ascontiguousarray(p_dev[offset:offset + rows * cols], dtype=np.float32).reshape(rows, cols)
    hi = bf16_round(w)
    return bf16_bits(hi), bf16_bits((w - hi).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ float32 emulations (host test)
def fma32(a, b, c):
    return (np.asarray(a, dtype=F64) * np.asarray(b, dtype=F64) + np.asarray(c, dtype=F64)).astype(np.float32)


def adam_update_f32(param, g, exp_avg, exp_avg_sq, betas, eps, weight_decay, scalars, grad_scale=1.0):
    """mg_adam_update step by step in float32 numpy (the fused multiply-adds through float64 and one rounding)."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (param, g, exp_avg, exp_avg_sq))
    b1, b2 = f(betas[0]), f(betas[1])
    g = g * f(grad_scale)
    if f(weight_decay) != 0:
        g = fma32(f(weight_decay), p, g)
    m = fma32(g - m, f(1) - b1, m)
    v = fma32((f(1) - b2) * g, g, v * b2)
    denom = np.sqrt(v) / f(scalars[1]) + f(eps)
    p = p - f(scalars[0]) * (m / denom)
    return p, m, v


def slab_sum_f32(grad, sources, order='partitions'):
    """grad + the slab sums in float32: 'partitions' = the slab reduce's order (16 interleaved partitions, each ascending, added in
    ascending order onto the gradient), 'ascending' = slab after slab onto the gradient."""
    out = np.asarray(grad, dtype=np.float32).copy()
    for begin, count, slabs in sources:
        s = np.asarray(slabs, dtype=np.float32)[:, :count]
        acc = out[begin:begin + count].copy()
        if order == 'ascending':
            for row in s:
                acc = acc + row
        else:
            for p in range(16):
                t = np.zeros(count, dtype=np.float32)
                for row in s[p::16]:
                    t = t + row
                acc = acc + t
        out[begin:begin + count] = acc
    return out
