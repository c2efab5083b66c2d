"""Float64 restatement of the five launches of the bf16 phone-rate training step (bench.py C2), one function per launch, each computed
from the operands THAT launch was given and each output a ``Bounded`` (value, bound) - numpy only, no torch, no GPU.

    linear_fwd     mg_phone_front_linear_fwd_bf16        H1 = bf16(sigmoid(A W1^T + b1))
    l2tail_rows    mg_f0_l2tail_rows[_slabs]_bf16        layers 2-4, the weighted squared error and their backward (l2tail_bf16.hip (1)-(9))
    l2tail_frames  mg_f0_l2tail[_slabs]_bf16             the same kernel with the (B, T) mask and 1 / (n_b B)
    tail_rows      mg_f0_tail_rows_bf16                  the 128-wide tail (tail_bf16.hip) from a given H2
    wgrad_dgrad    mg_linear_wgrad_dgrad[_expand]_bf16   dW2 | db2 (the fp32 sum of the slabs) and dZ1 = bf16((dZ2 W2) H1 (1 - H1))
    wgrad          mg_linear_wgrad_slabs_bf16            dW1 | db1 on a 640-wide operand with k columns in use
    expand_loss    mg_expand_column_reduce_f32           pred[rows] and the loss plus the constant term

The bounds are properties of fp32 arithmetic and of the roundings the kernels' code shows, not of what a device returns:

* a product accumulated in fp32 in ANY order: g(K) sum |a||w| with g(K) = gamma(K) / (1 - gamma(K)), gamma(K) = (K + 4) 2^-24 of
  recurrent_ref64 (the +4 covers a bias added before or after and the product roundings of a scalar chain; the denominator makes the
  first-order figure rigorous at the K = 33 000 of a weight gradient).  A sum over rows finished over slabs has K = rows + slabs;
* ``mg_sigmoid_fast``: FAST_SIGMOID_ABS, as ``b_sigmoid(fast=True)`` charges it;
* elementwise fp32 operations: ``Bounded`` arithmetic, in the kernels' association order;
* a value the kernel ROUNDS TO BF16 (an output, or the next product's operand): ``round_bf16`` rounds the float64 value.  Where
  bf16(v - e) == bf16(v + e) every fp32 value within the bound rounds to the same bf16 (rounding is monotone): the element is exact
  from there on, e = 0.  Otherwise it is AMBIGUOUS: the device may hold the neighbouring bf16, and one bf16 spacing at |v| is added to
  the bound.  The share of ambiguous elements is returned with every result (``shares``).  Where the kernels round (l2tail_bf16.hip):
  H2 before Z3, and H2 (1 - H2) from the ROUNDED value; W3 in both of its products; dZ3 in dH2 and dW3 but NOT in db3; dW4 / db4 /
  the loss never; dZ2 as it is stored.

``exact=True`` states that the caller's operands make every partial sum of the launch's contractions exactly representable in fp32
(``exact_condition``): the products' bound is then ZERO and a dropped, doubled or misplaced term shows in full.  It assumes that the
matrix cores keep at least 24 significant bits below the largest addend of an accumulate step.

Two operand generators per launch: ``exact_*`` (dyadic grids, the condition asserted) and ``wide_*`` (realistic scales: W2 +-0.08, H1 in
(0.05, 0.95), row weights spread over e^+-3 with one row in ten at weight 0, standard normal targets)."""
import numpy as np

from recurrent_ref64 import EPS, ETA, Bounded, b_sigmoid, bf16_round, gamma

F64 = np.float64
F32 = np.float32
N_TAIL = 32 * 128 + 32 + 32 + 1                # dW3 | db3 | dW4 | db4; the loss follows
GRAD_SCALES = (1.0, 0.125, 1.0 / 3.0)


def g(k):
    """gamma(k) made rigorous: k U / (1 - k U) instead of its first-order form."""
    return gamma(k) / (1.0 - gamma(k))


# ------------------------------------------------------------------------------------------------------------ launch arithmetic
def l2tail_blocks(m):
    """Workgroups (= slabs) of f0_l2tail_kernel: one 32-row tile per wave, 4 waves, at most 256 workgroups (l2tail_bf16.hip)."""
    return max(1, min(256, -(-(-(-m // 32)) // 4)))


def tail_blocks(m):
    """Workgroups of f0_tail_kernel (tail_bf16.hip): at most 512."""
    return max(1, min(512, -(-(-(-m // 32)) // 4)))


def _up(x, a):
    return -(-x // a) * a


def wgrad_plan(m, n, k, lda):
    """(splits, rows per split) of mg_wgrad_big_plan (gemm_bf16_big.hip) at phone-rate row counts 4096 <= m <= 32768, restated."""
    assert 4096 <= m <= 32768 and n % 128 == 0
    tiles_n = n // 128
    s = -(-256 // tiles_n)
    if tiles_n >= 4:
        s = 192 // tiles_n
    if lda == 640 and tiles_n >= 4:                       # the half-width plan (wgrad_ksplit)
        s = 256 // (2 * tiles_n)
    elif lda == 512 and n == 128:
        s = 48
    if tiles_n == 1:
        s = 96
    chunk = _up(-(-m // s), 32)
    while chunk > 4096:
        s *= 2
        chunk = _up(-(-m // s), 32)
    return _up(-(-m // chunk), 8), chunk


def pair_plan(m):
    """(splits, rows per split) of mg_launch_wgrad_dgrad_pair for the 128 x 512 layer: the plan's split count, lowered in steps of 8
    until every XCD has at most 32 working blocks (two k halves per split, two 256-wide dgrad tiles per 256 rows); None = it does
    not take the shape."""
    s, chunk = wgrad_plan(m, 128, 512, 512)
    tiles_m, tiles_n, kt = -(-m // 256), 2, 2

    def fits(s_, chunk_):
        s_real = -(-m // chunk_)
        for x in range(8):
            nt = (-(-(tiles_m - x) // 8) if tiles_m > x else 0) * tiles_n
            wg = sum(kt for b in range(x, s_, 8) if b < s_real)
            if nt + wg > 32:
                return False
        return True

    cand = s
    while cand >= 48 // kt:
        chunk_ = chunk if cand == s else _up(-(-m // cand), 32)
        if chunk_ > 4096:
            break
        s_ = _up(-(-m // chunk_), 8)
        if s_ <= s and fits(s_, chunk_):
            return s_, chunk_
        cand -= 8
    return None


# ------------------------------------------------------------------------------------------------------------ bf16 rounding
def bf16_spacing(x):
    """Spacing of the bf16 grid at |x| (8 significant bits; never below the spacing of the bf16 subnormals)."""
    _, ex = np.frexp(np.abs(np.asarray(x, dtype=F64)))
    return np.ldexp(1.0, np.maximum(ex - 8, -133))


def round_bf16(b):
    """A Bounded fp32 value as the kernel rounds it to bf16 -> (Bounded, share of ambiguous elements)."""
    b = Bounded.lift(b)
    v = bf16_round(b.v)
    amb = bf16_round(b.v - b.e) != bf16_round(b.v + b.e)
    e = np.where(amb, b.e + bf16_spacing(np.abs(b.v) + b.e), 0.0)
    return Bounded(v, e), float(amb.mean()) if amb.size else 0.0


# ------------------------------------------------------------------------------------------------------------ products
def mm(a, w, bias=None, exact=False):
    """a [M,K] (Bounded) x w [N,K]^T (+ bias) accumulated in fp32 in any order."""
    a = Bounded.lift(a)
    w = np.asarray(w, dtype=F64)
    k = w.shape[1]
    v = a.v @ w.T
    if bias is not None:
        bias = np.asarray(bias, dtype=F64)
        v = v + bias
    e = a.e @ np.abs(w).T if np.any(a.e) else 0.0          # (products of this size are the reference's cost: none is formed for nothing)
    if not exact:
        mag = np.abs(a.v) @ np.abs(w).T
        if bias is not None:
            mag = mag + np.abs(bias)
        e = e + g(k) * mag + k * ETA
    return Bounded(v, e)


def rows_product(a, b, k_terms, exact=False):
    """sum over rows of a[m, i] b[m, j] -> [I, J], accumulated in fp32 in any order over k_terms = rows + slabs terms."""
    a, b = Bounded.lift(a), Bounded.lift(b)
    v, e = a.v.T @ b.v, 0.0
    if np.any(a.e):
        e = e + a.e.T @ (np.abs(b.v) + b.e)
    if np.any(b.e):
        e = e + np.abs(a.v).T @ b.e
    if not exact:
        e = e + g(k_terms) * (np.abs(a.v).T @ np.abs(b.v)) + k_terms * ETA
    return Bounded(v, e)


def rows_sum(a, k_terms, exact=False):
    """sum over rows (axis 0) of a Bounded in fp32 in any order."""
    a = Bounded.lift(a)
    e = a.e.sum(axis=0)
    if not exact:
        e = e + g(k_terms) * np.abs(a.v).sum(axis=0)
    return Bounded(a.v.sum(axis=0), e)


def cat(*parts):
    return Bounded(np.concatenate([p.v.reshape(-1) for p in parts]), np.concatenate([np.asarray(p.e).reshape(-1) for p in parts]))


# ------------------------------------------------------------------------------------------------------------ the launches
def linear_fwd(a, w, bias, k, exact=False):
    """Layer 1: bf16(sigmoid_fast(a[:, :k] w[:, :k]^T + bias)); a, w hold the bf16 operands' values.  -> dict y, shares."""
    z = mm(Bounded(np.asarray(a, dtype=F64)[:, :k]), np.asarray(w, dtype=F64)[:, :k], bias, exact)
    y, share = round_bf16(b_sigmoid(z, fast=True))
    return {'y': y, 'shares': {'y': share}}


def _tail_chain(h2, w3, b3, w4, b4, target, s1, cw, lw, k_rows):
    """Steps (3)-(9) of l2tail_bf16.hip = tail_bf16.hip (2)-(9) from the bf16 H2 the kernel holds.  s1 [M]: the row weight / the mask;
    cw: the factor of dpred (2 grad_scale [inv]); lw: the factor of the loss term (None = 1); k_rows = rows + slabs."""
    w3r = bf16_round(np.asarray(w3, dtype=F32)).astype(F64)
    w4 = np.asarray(w4, dtype=F64).reshape(-1)
    b4 = float(np.asarray(b4, dtype=F64).reshape(-1)[0])
    s1 = np.asarray(s1, dtype=F64)
    z3 = mm(h2, w3r, b3)
    h3 = b_sigmoid(z3, fast=True)
    pred = Bounded(h3.v @ w4 + b4, h3.e @ np.abs(w4) + g(32) * (np.abs(h3.v) @ np.abs(w4) + abs(b4)) + 32 * ETA)
    err = pred - Bounded(np.asarray(target, dtype=F64))
    dpred = (err * s1) * cw
    lt = (err * err) * s1
    if lw is not None:
        lt = lt * lw
    loss, db4 = rows_sum(lt, k_rows), rows_sum(dpred, k_rows)
    dp = Bounded(dpred.v[:, None], dpred.e[:, None])
    dz3 = ((dp * w4[None, :]) * h3) * (1.0 - h3)
    dw4 = rows_sum(dp * h3, k_rows)
    db3 = rows_sum(dz3, k_rows)                          # the fp32 dZ3
    dz3r, sh_dz3 = round_bf16(dz3)
    dh2 = mm(dz3r, w3r.T)
    dz2, sh_dz2 = round_bf16((dh2 * h2) * (1.0 - h2))
    dw3 = rows_product(dz3r, h2, k_rows)
    return {'pred': pred, 'loss': loss, 'dz2': dz2, 'dw3': dw3, 'db3': db3, 'dw4': dw4, 'db4': db4,
            'grads': cat(dw3, db3, dw4, db4), 'shares': {'dz3': sh_dz3, 'dz2': sh_dz2}}


def _layer2(h1, w2, b2, exact):
    z2 = mm(Bounded(np.asarray(h1, dtype=F64)[:, :512]), np.asarray(w2, dtype=F64)[:, :512], b2, exact)     # the accumulators start from b2
    return round_bf16(b_sigmoid(z2, fast=True))


def l2tail_rows(h1, w2, b2, w3, b3, w4, b4, ybar, weight, grad_scale=1.0, exact=False):
    """h1 [M, >=512], w2 [128, >=512]: the values of the bf16 operands.  loss = sum_m weight[m] (pred[m] - ybar[m])^2."""
    m = np.asarray(h1).shape[0]
    h2, share = _layer2(h1, w2, b2, exact)
    res = _tail_chain(h2, w3, b3, w4, b4, ybar, weight, 2.0 * float(F32(grad_scale)), None, m + l2tail_blocks(m))
    res['shares']['h2'] = share
    return res


def l2tail_frames(h1, w2, b2, w3, b3, w4, b4, target, seq_len, b, t, grad_scale=1.0, exact=False):
    """The seq_len form: a = [t < n_b], inv = 1 / (n_b B) (one fp32 division), dpred = (e a) (2 grad_scale inv), loss term (e e a) inv."""
    m = b * t
    nb = np.clip(np.full(b, t, dtype=F64) if seq_len is None else np.asarray(seq_len, dtype=F64), 0, t)
    mask = (np.arange(t)[None, :] < nb[:, None]).reshape(-1).astype(F64)
    inv_v = np.repeat(1.0 / (nb * b), t)
    inv = Bounded(inv_v, 2 * EPS * inv_v)
    h2, share = _layer2(h1, w2, b2, exact)
    res = _tail_chain(h2, w3, b3, w4, b4, target, mask, inv * (2.0 * float(F32(grad_scale))), inv, m + l2tail_blocks(m))
    res['shares']['h2'] = share
    return res


def tail_rows(h2, w3, b3, w4, b4, ybar, weight, grad_scale=1.0):
    """tail_bf16.hip on the H2 it is given (bf16 values, [M, 128])."""
    m = np.asarray(h2).shape[0]
    return _tail_chain(Bounded(np.asarray(h2, dtype=F64)[:, :128]), w3, b3, w4, b4, ybar, weight, 2.0 * float(F32(grad_scale)), None,
                       m + tail_blocks(m))


def wgrad_dgrad(dz2, h1, w2t, n_slabs, exact=False):
    """dz2 [M, 128], h1 [M, 512], w2t = W2^T [512, 128] (bf16 values).  -> dwdb = dW2 (128 x 512) | db2, dz1 [M, 512] bf16."""
    dz2, h1 = np.asarray(dz2, dtype=F64)[:, :128], np.asarray(h1, dtype=F64)[:, :512]
    k_rows = dz2.shape[0] + n_slabs
    dw = rows_product(Bounded(dz2), Bounded(h1), k_rows, exact)
    db = rows_sum(Bounded(dz2), k_rows, exact)
    v = mm(Bounded(dz2), np.asarray(w2t, dtype=F64)[:, :128], None, exact)
    dz1, share = round_bf16((v * h1) * (1.0 - Bounded(h1)))
    return {'dwdb': cat(dw, db), 'dw': dw, 'db': db, 'dz1': dz1, 'shares': {'dz1': share}}


def wgrad(dz1, a, k, n_slabs, exact=False):
    """dz1 [M, N], a [M, lda] with k columns in use (bf16 values).  -> dwdb = dW1 (N x k) | db1."""
    dz1, a = np.asarray(dz1, dtype=F64), np.asarray(a, dtype=F64)[:, :k]
    k_rows = dz1.shape[0] + n_slabs
    dw, db = rows_product(Bounded(dz1), Bounded(a), k_rows, exact), rows_sum(Bounded(dz1), k_rows, exact)
    return {'dwdb': cat(dw, db), 'dw': dw, 'db': db}


def expand_loss(pred_rows, rows, loss, partials):
    """The repeated prediction (exact) and loss + sum(partials), the partial sums added in fp32 in any order."""
    partials = np.asarray(partials, dtype=F64)
    loss = Bounded.lift(loss)
    c = partials.sum()
    return {'pred': np.asarray(pred_rows)[np.asarray(rows)],
            'loss': Bounded(loss.v + c, loss.e + g(partials.size + 1) * (np.abs(loss.v) + np.abs(partials).sum()))}


# ------------------------------------------------------------------------------------------------------------ operands
def exact_condition(a, ga, w, gw, bias=None, over_rows=False):
    """ASSERTS that a contraction of a (multiples of 2^-ga) with w (multiples of 2^-gw) - over the columns (a [M,K], w [N,K]), or
    over_rows (a [M,I], w [M,J]) - has every partial sum exactly representable in fp32 whatever the order: all terms (and the bias)
    are multiples of 2^-(ga + gw) and sum |terms| (+ |bias|) < 2^(24 - ga - gw).  Returns the worst sum |terms|."""
    a, w = np.asarray(a, dtype=F64), np.asarray(w, dtype=F64)
    gg = ga + gw
    assert np.array_equal(a * 2.0 ** ga, np.round(a * 2.0 ** ga)) and np.array_equal(w * 2.0 ** gw, np.round(w * 2.0 ** gw))
    assert np.array_equal(bf16_round(a), a) and np.array_equal(bf16_round(w), w), 'operands must be bf16 values'
    mag = np.abs(a).T @ np.abs(w) if over_rows else np.abs(a) @ np.abs(w).T
    if bias is not None:
        bias = np.asarray(bias, dtype=F64)
        assert np.array_equal(bias * 2.0 ** gg, np.round(bias * 2.0 ** gg))
        mag = mag + np.abs(bias)
    worst = float(mag.max())
    assert worst < 2.0 ** (24 - gg), (worst, gg)
    return worst


def _grid(rng, lo, hi, shape, bits):
    return (rng.randint(lo, hi + 1, size=shape) / 2.0 ** bits).astype(F32)


def _row_weights(rng, m):
    """Row weights spread over e^+-3, one row in ten at 0; the LAST row is live and heavy (e^3): it is the one a ragged tile's edge
    handling can lose or count twice."""
    w = np.exp(rng.uniform(-3, 3, m)) * (rng.uniform(0, 1, m) > 0.1) / m
    w[m - 1] = np.exp(3.0) / m
    return w.astype(F32)


def _tail_params(rng, sparse=False):
    """W3, b3, w4, b4 (fp32: the kernel rounds W3 to bf16 itself).  ``sparse``: four nonzero weights per unit of layer 3, so that
    sum |H2||W3| - and with it the bound of Z3, whose operand H2 comes out of a sigmoid and cannot lie on a grid - stays small: the
    chain behind Z3 then keeps nearly every dZ3 and dZ2 unambiguous, and they are compared to the bit."""
    w3 = rng.uniform(-0.2, 0.2, (32, 128))
    if sparse:
        keep = np.zeros((32, 128), dtype=bool)
        for n in range(32):
            keep[n, rng.choice(128, size=4, replace=False)] = True
        w3 = np.where(keep, np.sign(w3) * rng.uniform(0.3, 0.6, (32, 128)), 0.0)
    return {'w3': w3.astype(F32), 'b3': rng.uniform(-0.1, 0.1, 32).astype(F32),
            'w4': rng.uniform(-0.3, 0.3, (1, 32)).astype(F32), 'b4': rng.uniform(-0.1, 0.1, 1).astype(F32)}


EXACT_L2TAIL_SEED = {33: 3}      # seeds of the shapes the GPU tests run (others 0): the reference's own H2 share is <= 1e-3 on them


def exact_l2tail(m, seed=None):
    """H1 in j/64, W2 in +-j/4096 (|j| <= 127: bf16 values up to 0.031), b2 in j/2^18: Z2 = H1 W2^T + b2 is exact in fp32 in any order
    (asserted: multiples of 2^-18 below 2^6).  The fine grid matters: sigmoid(Z2) takes as many distinct values as Z2 does, and on a
    coarse grid the few values that fall next to a bf16 rounding boundary are each hit by many elements."""
    rng = np.random.RandomState(1000 + (EXACT_L2TAIL_SEED.get(m, 0) if seed is None else seed))
    c = {'h1': _grid(rng, 1, 63, (m, 512), 6), 'w2': _grid(rng, -127, 127, (128, 512), 12), 'b2': _grid(rng, -26000, 26000, 128, 18)}
    c['sum_abs'] = exact_condition(c['h1'], 6, c['w2'], 12, c['b2'])
    c.update(_tail_params(rng, sparse=True))
    c['ybar'], c['weight'] = rng.standard_normal(m).astype(F32), _row_weights(rng, m)
    return c


def wide_l2tail(m, seed=0):
    rng = np.random.RandomState(2000 + seed)
    c = {'h1': bf16_round(rng.uniform(0.05, 0.95, (m, 512)).astype(F32)), 'w2': bf16_round(rng.uniform(-0.08, 0.08, (128, 512)).astype(F32)),
         'b2': rng.uniform(-0.1, 0.1, 128).astype(F32)}
    c.update(_tail_params(rng))
    c['ybar'], c['weight'] = rng.standard_normal(m).astype(F32), _row_weights(rng, m)
    return c


def tail_h2(m, seed=0):
    """A bf16 H2 for tail_rows (sigmoid outputs of a realistic layer 2) with the tail's parameters, targets and weights."""
    rng = np.random.RandomState(3000 + seed)
    c = {'h2': bf16_round((1.0 / (1.0 + np.exp(-rng.standard_normal((m, 128))))).astype(F32))}
    c.update(_tail_params(rng))
    c['ybar'], c['weight'] = rng.standard_normal(m).astype(F32), _row_weights(rng, m)
    return c


def exact_pair(m, seed=0):
    """dZ2 in +-j/32, H1 in j/32, W2 in +-j/256 (|j| <= 20): dW2, db2 over m rows and dZ2 W2 over 128 columns are exact (asserted)."""
    rng = np.random.RandomState(4000 + seed)
    c = {'dz2': _grid(rng, -31, 31, (m, 128), 5), 'h1': _grid(rng, 1, 31, (m, 512), 5), 'w2': _grid(rng, -20, 20, (128, 512), 8)}
    c['sum_abs'] = max(exact_condition(c['dz2'], 5, c['h1'], 5, over_rows=True), exact_condition(c['dz2'], 5, np.ones((m, 1)), 0, over_rows=True))
    exact_condition(c['dz2'], 5, c['w2'].T, 8)
    return c


def wide_pair(m, seed=0):
    """H1 and W2 at realistic scales; dZ2 with the rows' scales spread as the tail's row weights spread them."""
    rng = np.random.RandomState(5000 + seed)
    return {'dz2': bf16_round((rng.standard_normal((m, 128)) * 0.01 * (_row_weights(rng, m) * m)[:, None]).astype(F32)),
            'h1': bf16_round(rng.uniform(0.05, 0.95, (m, 512)).astype(F32)), 'w2': bf16_round(rng.uniform(-0.08, 0.08, (128, 512)).astype(F32))}


def _table(rng, m, k, extra, exact):
    a = np.zeros((m, 640), dtype=F32)                    # the last `extra` rows are the zero rows behind the table
    a[:m - extra, :k] = _grid(rng, -31, 31, (m - extra, k), 5) if exact else bf16_round(rng.uniform(0, 1, (m - extra, k)).astype(F32))
    return a


def exact_wgrad(m, n, k, extra=1024, seed=0):
    """dZ1 in +-j/32 (every row, the extra rows included), A in +-j/32 with zero extra rows: dW1 | db1 over m rows exact (asserted)."""
    rng = np.random.RandomState(6000 + seed)
    c = {'dz1': _grid(rng, -31, 31, (m, n), 5), 'a': _table(rng, m, k, extra, True)}
    c['sum_abs'] = max(exact_condition(c['dz1'], 5, c['a'], 5, over_rows=True), exact_condition(c['dz1'], 5, np.ones((m, 1)), 0, over_rows=True))
    return c


def wide_wgrad(m, n, k, extra=1024, seed=0):
    rng = np.random.RandomState(7000 + seed)
    return {'dz1': bf16_round((rng.standard_normal((m, n)) * 0.01 * (_row_weights(rng, m) * m)[:, None]).astype(F32)),
            'a': _table(rng, m, k, extra, False)}


def exact_fwd(m, k, n, seed=0):
    """A in +-j/64, W1 in +-j/4096 (|j| <= 127), b1 in j/2^18: A W1^T and the sum with b1 are exact in fp32 (asserted)."""
    rng = np.random.RandomState(8000 + seed)
    a, w = np.zeros((m, 640), dtype=F32), np.zeros((n, 640), dtype=F32)
    a[:, :k], w[:, :k] = _grid(rng, -63, 63, (m, k), 6), _grid(rng, -127, 127, (n, k), 12)
    c = {'a': a, 'w': w, 'bias': _grid(rng, -26000, 26000, n, 18)}
    c['sum_abs'] = exact_condition(a, 6, w, 12, c['bias'])
    return c
