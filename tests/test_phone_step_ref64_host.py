"""tests/phone_step_ref64.py checked on the host, without a GPU: an fp32 numpy emulation of every chain of the bf16 phone-rate step
(bf16 roundings at the kernels' points, sums in ascending and in permuted order, row sums finished over slabs) stays inside every
bound; each fault a rewrite of these kernels could plausibly make moves at least one output by two bounds or more; the ``exact``
generators' condition and the ambiguity cap hold on the seeds the GPU tests use; and the reference's gradients are the derivatives of
its own float64 loss.

HEADROOM (test_emulation_stays_inside_every_bound; worst observed / bound of the fp32 emulation against the float64 reference over
both orders - a figure of the reference, never of a kernel):

    layers 2-4 pass, rows     pred 0.771   loss 0.0018   dZ2 0.814   dW3 0.075   db3 0.0042   dW4 0.0069   db4 0.0022
    layers 2-4 pass, frames   pred 0.011   loss 0.0004   dZ2 0       dW3 0.015   db3 0.0037   dW4 0.0038   db4 0.0031
    128-wide tail             pred 0.0036  loss 0.0005   dZ2 0.951   dW3 0.021   db3 0.0014   dW4 0.0014   db4 0.0007
    pair grid                 dW2 | db2  exact 0 (equal)  wide 0.0002     dZ1  exact 0 (equal)  wide 0.996
    layer-1 weight gradient   dW1 | db1  exact 0 (equal)  wide 0.0002
    layer-1 forward           H1  exact 0 (equal), wide 0 (equal: no element of these cases flipped)
    loss + constant term      0.0006

Two kinds of figure.  A bf16 OUTPUT (dZ2, dZ1, H1) is either equal to the reference (0) or, where the emulation's rounding fell on the
other side of an ambiguous element, one bf16 spacing off against a bound of that spacing plus the fp32 bound: 0.8 - 0.996 BY
CONSTRUCTION, never above 1.  The 0.771 of pred is one row of 4127 whose H2 holds a flipped ambiguous element; rows without one sit
at 0.01.  Everything else is an fp32 quantity against a worst-case bound: sums over thousands of rows use 1e-3 of gamma(rows +
slabs) sum |terms| (rounding errors add like a random walk), short chains 1e-2.

SENSITIVITY (test_fault_is_at_least_two_bounds_away; the largest ratio over the outputs the fault reaches):
 (a) last live row of a ragged tile left out of the sums: M = 33 wide 517, exact 4.8e4; M = 4127 exact 9.8.
 (b) the clamped copy of row M - 1 counted: M = 33 wide 517; M = 4127 exact 9.8.
     (The generators make the last row live and heavy - weight e^3 / M, the top of the spread.  An average row of 4127 moves a sum by
     about 1.5 bounds: one row against gamma(4127 + 33) of the sum of all.)
 (c) H2 (1 - H2) from the unrounded H2: M = 33 exact inf (dZ2 elements that are not ambiguous must match to the bit).
 (d) units 3 and 7 of W3 exchanged in dH2: M = 33 wide 21, exact inf.
 (e) at grad_scale = 1/3, M = 33 wide: grad_scale dropped 1071, row weight applied twice 260, factor 2 missing 268.
 (f) one workgroup slab left out / summed twice: layers 2-4 at M = 4127 exact 118; pair grid exact inf, wide 75; layer 1 exact inf,
     wide 158.
 (g) an empty split's slab holds stale data (a copy of split 0's): pair grid exact inf, wide 71; layer 1 exact inf, wide 242.
 (h) the extra rows left out of db1: exact inf, wide 192.
 (i) the last 16-byte piece of a row written one piece to the left: dZ2 (M = 33 wide) 99, dZ1 inf.
OUT OF REACH of the ``wide`` operands, recorded by test_faults_out_of_reach_of_the_wide_operands: (c) reaches 0.37 and (a) at M = 4127
0.07 there.  With W2 at +-0.08 the bound of Z2 makes 6 % of H2 ambiguous - eight elements of every row - and a bf16 spacing of H2 in
Z3 leaves 75 - 90 % of dZ3 and dZ2 ambiguous and the row sums bounded at 1e-3 of sum |terms|.  Dense realistic operands therefore
check these kernels to about a bf16 spacing per element; the ``exact`` operands (Z2 exact in fp32, four weights per unit of layer 3)
keep 97 % of dZ2 unambiguous and are the ones that reach every fault above."""
import functools

import numpy as np
import pytest

import phone_step_ref64 as ref
from recurrent_ref64 import bf16_round, ratio

F32, F64 = np.float32, np.float64
ONE = F32(1)


# ------------------------------------------------------------------------------------------------------------ fp32 emulation
def _order(n, permuted, seed=0):
    return np.random.RandomState(77 + seed + n).permutation(n) if permuted else np.arange(n)


def _dot32(a, w, order, init=None):
    """a [M,K] w [N,K]^T with one fp32 accumulator per output, terms added in ``order``."""
    a, w = np.asarray(a, dtype=F32), np.asarray(w, dtype=F32)
    acc = np.zeros((a.shape[0], w.shape[0]), dtype=F32) if init is None else np.broadcast_to(np.asarray(init, dtype=F32), (a.shape[0], w.shape[0])).copy()
    for k in order:
        acc += a[:, k:k + 1] * w[:, k][None, :]
    return acc


def _sig32(x):
    x = np.asarray(x, dtype=F32)
    return ONE / (ONE + np.exp(-x))


def _seq_sum(x):
    """Strictly sequential fp32 sum over axis 0."""
    return np.cumsum(np.asarray(x, dtype=F32), axis=0, dtype=F32)[-1] if len(x) else np.zeros(np.asarray(x).shape[1:], dtype=F32)


def _slab_rows(m, chunk, n_slabs, permuted, fault=None):
    """Row indices per slab (consecutive chunks; trailing slabs may be empty), with the faults that touch which rows are counted."""
    out = []
    for s in range(n_slabs):
        idx = np.arange(min(s * chunk, m), min((s + 1) * chunk, m))
        if fault == 'drop_last_row' and len(idx) and idx[-1] == m - 1:
            idx = idx[:-1]
        if fault == 'count_clamped_row' and len(idx) and idx[-1] == m - 1:
            idx = np.append(idx, m - 1)
        if permuted and len(idx):
            idx = idx[_order(len(idx), True, s)]
        out.append(idx)
    return out


def _sum_slabs(per_slab, fault, stale=None):
    """fp32 sum of the slabs in ascending order; faults: a slab left out, summed twice, an empty one holding stale data."""
    tot = np.zeros_like(per_slab[0][0])
    used = [s for s, (_, n_rows) in enumerate(per_slab) if n_rows]
    victim = used[len(used) // 2]
    for s, (v, n_rows) in enumerate(per_slab):
        if fault == 'slab_dropped' and s == victim:
            continue
        if fault == 'stale_empty_slab' and n_rows == 0 and s == len(per_slab) - 1:
            v = per_slab[0][0] if stale is None else stale
        tot = tot + v
        if fault == 'slab_twice' and s == victim:
            tot = tot + v
    return tot


def emu_tail(c, h2, h2_grad, s1, cw, lw, n_blocks, permuted, fault=None):
    """Steps (3)-(9) in fp32.  h2: the bf16 H2; h2_grad: what H2 (1 - H2) is formed from (h2, or the unrounded value: fault c)."""
    m = h2.shape[0]
    w3r = bf16_round(c['w3'])
    w3_dh = w3r.copy()
    if fault == 'swap_w3_units':
        w3_dh[[3, 7]] = w3_dh[[7, 3]]
    w4, b4, tgt, s1 = c['w4'].reshape(-1).astype(F32), F32(c['b4'][0]), c['ybar'].astype(F32), np.asarray(s1, dtype=F32)
    h3 = _sig32(_dot32(h2, w3r, _order(128, permuted)) + c['b3'].astype(F32))
    ph = np.zeros(m, dtype=F32)
    for r in _order(32, permuted):
        ph += h3[:, r] * w4[r]
    p = ph + b4
    e = p - tgt
    cw = np.asarray(cw, dtype=F32)
    dpred = (e * s1 * s1) * cw if fault == 'weight_twice' else (e * s1) * cw
    lt = e * e * s1
    if lw is not None:
        lt = lt * np.asarray(lw, dtype=F32)
    dz3 = dpred[:, None] * w4[None, :] * h3 * (ONE - h3)
    dw4t = dpred[:, None] * h3
    dz3r = bf16_round(dz3)
    dh2 = _dot32(dz3r, w3_dh.T, _order(32, permuted))
    dz2 = bf16_round(dh2 * h2_grad * (ONE - h2_grad))
    if fault == 'piece_left':
        dz2[:, 112:120], dz2[:, 120:128] = dz2[:, 120:128].copy(), 0
    slabs = []
    for idx in _slab_rows(m, 128, n_blocks, permuted, fault):
        flat = np.concatenate([_seq_sum(dz3r[idx][:, :, None] * h2[idx][:, None, :]).reshape(-1), _seq_sum(dz3[idx]), _seq_sum(dw4t[idx]),
                               _seq_sum(dpred[idx])[None], _seq_sum(lt[idx])[None]])
        slabs.append((flat, len(idx)))
    tot = _sum_slabs(slabs, fault)
    return {'pred': p, 'loss': tot[-1], 'dz2': dz2, 'grads': tot[:-1], 'db4': tot[-2], 'dw3': tot[:4096].reshape(32, 128), 'db3': tot[4096:4128],
            'dw4': tot[4128:4160]}


def _cw(grad_scale, fault):
    gs = F32(grad_scale)
    return F32(2) if fault == 'no_grad_scale' else gs if fault == 'no_factor_two' else F32(2) * gs


_H2_CACHE = {}


def emu_l2tail_rows(c, grad_scale, permuted, fault=None):
    key = (id(c['h1']), permuted)                        # (the cases are cached below: one layer-2 emulation per case and order)
    if key not in _H2_CACHE:
        _H2_CACHE[key] = _sig32(_dot32(c['h1'], c['w2'], _order(512, permuted), init=c['b2']))
    h2u = _H2_CACHE[key]
    h2 = bf16_round(h2u)
    return emu_tail(c, h2, h2u if fault == 'unrounded_h2_grad' else h2, c['weight'], _cw(grad_scale, fault), None,
                    ref.l2tail_blocks(h2.shape[0]), permuted, fault)


def emu_l2tail_frames(c, seq_len, b, t, grad_scale, permuted):
    h2 = bf16_round(_sig32(_dot32(c['h1'], c['w2'], _order(512, permuted), init=c['b2'])))
    nb = np.repeat(seq_len, t).astype(F32)
    mask = (np.tile(np.arange(t), b) < nb).astype(F32)
    inv = ONE / (nb * F32(b))
    return emu_tail(c, h2, h2, mask, F32(2) * F32(grad_scale) * inv, inv, ref.l2tail_blocks(b * t), permuted)


def emu_tail_rows(c, grad_scale, permuted, fault=None):
    return emu_tail(c, c['h2'], c['h2'], c['weight'], _cw(grad_scale, fault), None, ref.tail_blocks(c['h2'].shape[0]), permuted, fault)


_SLAB_CACHE = {}


def emu_wgrad(dz, a, k, plan, permuted, fault=None, stale=None):
    """dW | db as the fp32 sum of the split-M slabs, each slab a sequential fp32 sum over its rows."""
    n_slabs, chunk = plan
    m = dz.shape[0]
    key = (id(dz), id(a), permuted)                      # (cached cases: the slabs' dW parts are formed once per case and order)
    dz32, a32 = np.asarray(dz, dtype=F32), np.asarray(a, dtype=F32)[:, :k]
    rows = _slab_rows(m, chunk, n_slabs, permuted)
    if key not in _SLAB_CACHE:
        dws = []
        for idx in rows:
            acc = np.zeros((dz32.shape[1], k), dtype=F32)
            for i in idx:
                acc += dz32[i][:, None] * a32[i][None, :]
            dws.append(acc.reshape(-1))
        _SLAB_CACHE[key] = dws
    slabs = []
    for idx, dw in zip(rows, _SLAB_CACHE[key]):
        d = dz32[idx]
        db = _seq_sum(d[idx < m - 1024] if fault == 'extra_rows_dropped' else d)
        slabs.append((np.concatenate([dw, db]), len(idx)))
    return _sum_slabs(slabs, fault, stale)


def emu_dgrad(dz2, w2, h1, permuted, fault=None):
    v = _dot32(dz2, np.asarray(w2, dtype=F32).T, _order(128, permuted))
    h1 = np.asarray(h1, dtype=F32)
    dz1 = bf16_round(v * h1 * (ONE - h1))
    if fault == 'piece_left':
        dz1[:, 496:504], dz1[:, 504:512] = dz1[:, 504:512].copy(), 0
    return dz1


def emu_fwd(c, k, permuted):
    z = _dot32(c['a'][:, :k], c['w'][:, :k], _order(k, permuted)) + c['bias'].astype(F32)
    return bf16_round(_sig32(z))


# ------------------------------------------------------------------------------------------------------------ cases, cached
@functools.lru_cache(maxsize=None)
def _l2tail_case(kind, m, gs):
    c = (ref.exact_l2tail if kind == 'exact' else ref.wide_l2tail)(m)
    want = ref.l2tail_rows(c['h1'], c['w2'], c['b2'], c['w3'], c['b3'], c['w4'], c['b4'], c['ybar'], c['weight'], gs, exact=(kind == 'exact'))
    return c, want


@functools.lru_cache(maxsize=None)
def _pair_case(kind, m):
    c = (ref.exact_pair if kind == 'exact' else ref.wide_pair)(m)
    return c, ref.wgrad_dgrad(c['dz2'], c['h1'], c['w2'].T, ref.pair_plan(m)[0], exact=(kind == 'exact'))


@functools.lru_cache(maxsize=None)
def _wgrad_case(kind, m, n, k):
    c = (ref.exact_wgrad if kind == 'exact' else ref.wide_wgrad)(m, n, k)
    return c, ref.wgrad(c['dz1'], c['a'], k, ref.wgrad_plan(m, 512, k, 640)[0], exact=(kind == 'exact'))


TAIL_OUTPUTS = ('pred', 'loss', 'dz2', 'dw3', 'db3', 'dw4', 'db4')


def _ratios(got, want, names):
    return {n: ratio(got[n], want[n]) for n in names}


# ------------------------------------------------------------------------------------------------------------ the bounds hold
def test_emulation_stays_inside_every_bound():
    worst = {}

    def held(label, r):
        worst[label] = max(worst.get(label, 0.0), r)

    for permuted in (False, True):
        for kind, m, gs in (('wide', 33, 1 / 3), ('wide', 129, 0.125), ('exact', 33, 1 / 3), ('exact', 4127, 1.0)):
            c, want = _l2tail_case(kind, m, gs)
            for n, r in _ratios(emu_l2tail_rows(c, gs, permuted), want, TAIL_OUTPUTS).items():
                held('l2tail_rows.' + n, r)
        b, t = 3, 11
        sl = np.array([11, 1, 7], dtype=np.int64)
        for kind in ('exact', 'wide'):
            c = (ref.exact_l2tail if kind == 'exact' else ref.wide_l2tail)(b * t, 7)
            want = ref.l2tail_frames(c['h1'], c['w2'], c['b2'], c['w3'], c['b3'], c['w4'], c['b4'], c['ybar'], sl, b, t, 0.125, exact=(kind == 'exact'))
            for n, r in _ratios(emu_l2tail_frames(c, sl, b, t, 0.125, permuted), want, TAIL_OUTPUTS).items():
                held('l2tail_frames.' + n, r)
        for m in (33, 4127):
            c = ref.tail_h2(m)
            want = ref.tail_rows(c['h2'], c['w3'], c['b3'], c['w4'], c['b4'], c['ybar'], c['weight'], 1 / 3)
            for n, r in _ratios(emu_tail_rows(c, 1 / 3, permuted), want, TAIL_OUTPUTS).items():
                held('tail_rows.' + n, r)
        for kind in ('exact', 'wide'):
            c, want = _pair_case(kind, 4127)
            held('pair.dwdb.' + kind, ratio(emu_wgrad(c['dz2'], c['h1'], 512, ref.pair_plan(4127), permuted), want['dwdb']))
            held('pair.dz1.' + kind, ratio(emu_dgrad(c['dz2'], c['w2'], c['h1'], permuted), want['dz1']))
            c, want = _wgrad_case(kind, 4127, 128, 600)
            held('wgrad.dwdb.' + kind, ratio(emu_wgrad(c['dz1'], c['a'], 600, ref.wgrad_plan(4127, 512, 600, 640), permuted), want['dwdb']))
        c = ref.exact_fwd(257, 600, 128)
        held('fwd.exact', ratio(emu_fwd(c, 600, permuted), ref.linear_fwd(c['a'], c['w'], c['bias'], 600, exact=True)['y']))
        rng = np.random.RandomState(3)
        a, w = bf16_round(rng.uniform(0, 1, (257, 600)).astype(F32)), bf16_round(rng.uniform(-0.08, 0.08, (128, 600)).astype(F32))
        cw = {'a': a, 'w': w, 'bias': rng.uniform(-0.1, 0.1, 128).astype(F32)}
        held('fwd.wide', ratio(emu_fwd(cw, 600, permuted), ref.linear_fwd(a, w, cw['bias'], 600)['y']))
        partials = rng.uniform(0, 1e-3, 400).astype(F32)
        loss32 = F32(0.7351)
        got = loss32 + (partials[_order(400, True)] if permuted else partials).sum(dtype=F32)
        held('expand_loss', ratio(got, ref.expand_loss(np.zeros(3), [0, 1], float(loss32), partials)['loss']))
    for label in sorted(worst):
        print('%-28s worst observed / bound = %.3g' % (label, worst[label]))
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if v > 1.0}
    # exact operands, exact sums: the emulation must EQUAL the float64 values where the bound is zero
    assert worst['pair.dwdb.exact'] == 0.0 and worst['wgrad.dwdb.exact'] == 0.0


# ------------------------------------------------------------------------------------------------------------ sensitivity
def _tail_fault(kind, m, gs, fault, outputs=TAIL_OUTPUTS):
    c, want = _l2tail_case(kind, m, gs)
    return max(_ratios(emu_l2tail_rows(c, gs, False, fault), want, outputs).values())


def _pair_fault(kind, fault):
    c, want = _pair_case(kind, 4127)
    if fault == 'piece_left':
        return ratio(emu_dgrad(c['dz2'], c['w2'], c['h1'], False, fault), want['dz1'])
    return ratio(emu_wgrad(c['dz2'], c['h1'], 512, ref.pair_plan(4127), False, fault), want['dwdb'])


def _wgrad_fault(kind, fault):
    c, want = _wgrad_case(kind, 4127, 128, 600)
    return ratio(emu_wgrad(c['dz1'], c['a'], 600, ref.wgrad_plan(4127, 512, 600, 640), False, fault), want['dwdb'])


SUMS = ('loss', 'dw3', 'db3', 'dw4', 'db4')
FAULTS = [
    ('a: last live row left out, M = 33 wide', lambda: _tail_fault('wide', 33, 1 / 3, 'drop_last_row', SUMS)),
    ('a: last live row left out, M = 33 exact', lambda: _tail_fault('exact', 33, 1 / 3, 'drop_last_row', SUMS)),
    ('a: last live row left out, M = 4127 exact', lambda: _tail_fault('exact', 4127, 1.0, 'drop_last_row', SUMS)),
    ('b: clamped row counted, M = 33 wide', lambda: _tail_fault('wide', 33, 1 / 3, 'count_clamped_row', SUMS)),
    ('b: clamped row counted, M = 4127 exact', lambda: _tail_fault('exact', 4127, 1.0, 'count_clamped_row', SUMS)),
    ('c: H2 (1 - H2) from the unrounded H2, exact', lambda: _tail_fault('exact', 33, 1 / 3, 'unrounded_h2_grad', ('dz2',))),
    ('d: W3 units 3 and 7 exchanged in dH2, wide', lambda: _tail_fault('wide', 33, 1 / 3, 'swap_w3_units', ('dz2',))),
    ('d: W3 units 3 and 7 exchanged in dH2, exact', lambda: _tail_fault('exact', 33, 1 / 3, 'swap_w3_units', ('dz2',))),
    ('e: grad_scale dropped', lambda: _tail_fault('wide', 33, 1 / 3, 'no_grad_scale')),
    ('e: row weight applied twice', lambda: _tail_fault('wide', 33, 1 / 3, 'weight_twice')),
    ('e: factor 2 missing', lambda: _tail_fault('wide', 33, 1 / 3, 'no_factor_two')),
    ('f: layers 2-4 slab left out, M = 4127 exact', lambda: _tail_fault('exact', 4127, 1.0, 'slab_dropped', SUMS)),
    ('f: layers 2-4 slab summed twice, M = 4127 exact', lambda: _tail_fault('exact', 4127, 1.0, 'slab_twice', SUMS)),
    ('f: pair grid slab left out, exact', lambda: _pair_fault('exact', 'slab_dropped')),
    ('f: pair grid slab summed twice, wide', lambda: _pair_fault('wide', 'slab_twice')),
    ('f: layer-1 slab left out, wide', lambda: _wgrad_fault('wide', 'slab_dropped')),
    ('f: layer-1 slab summed twice, exact', lambda: _wgrad_fault('exact', 'slab_twice')),
    ('g: pair grid empty split stale, exact', lambda: _pair_fault('exact', 'stale_empty_slab')),
    ('g: pair grid empty split stale, wide', lambda: _pair_fault('wide', 'stale_empty_slab')),
    ('g: layer-1 empty split stale, exact', lambda: _wgrad_fault('exact', 'stale_empty_slab')),
    ('g: layer-1 empty split stale, wide', lambda: _wgrad_fault('wide', 'stale_empty_slab')),
    ('h: extra rows left out of db1, exact', lambda: _wgrad_fault('exact', 'extra_rows_dropped')),
    ('h: extra rows left out of db1, wide', lambda: _wgrad_fault('wide', 'extra_rows_dropped')),
    ('i: last piece of a dZ2 row one to the left', lambda: _tail_fault('wide', 33, 1 / 3, 'piece_left', ('dz2',))),
    ('i: last piece of a dZ1 row one to the left', lambda: _pair_fault('wide', 'piece_left')),
]


@pytest.mark.parametrize('label,run', FAULTS, ids=[f[0].split(':')[0] + str(i) for i, f in enumerate(FAULTS)])
def test_fault_is_at_least_two_bounds_away(label, run):
    r = run()
    print('%-50s ratio = %.4g' % (label, r))
    assert r >= 2.0, (label, r)


def test_faults_out_of_reach_of_the_wide_operands():
    """Recorded, not excused: what dense realistic operands cannot show.  With W2 at +-0.08 about 6 % of H2 is ambiguous; each such
    element widens its row's Z3 by a bf16 spacing of H2, and through it every later quantity of the row: nearly all of dZ3 and dZ2 is
    then ambiguous and held to a bf16 spacing instead of to the bit, and the sums over rows to about 1e-3 of sum |terms|.  The
    ``exact`` operands (Z2 exact, four weights per unit of layer 3) keep 97 % of dZ2 unambiguous and reach these faults (above)."""
    c = _tail_fault('wide', 33, 1 / 3, 'unrounded_h2_grad', ('dz2',))
    a = _tail_fault('wide', 4127, 1.0, 'drop_last_row', SUMS)
    print('wide operands: (c) unrounded H2 in H2 (1 - H2) at M = 33: ratio %.3f; (a) last row left out at M = 4127: ratio %.3f' % (c, a))
    assert c < 2.0 and a < 2.0          # (if these ever reach 2 the docstrings' account of the wide bound is out of date)


# ------------------------------------------------------------------------------------------------------------ the generators' promises
GPU_L2TAIL_M = (1, 31, 33, 129, 4127, 32805)
GPU_PAIR_M = (4096, 4127, 8209)
GPU_WGRAD = ((4127, 512, 600), (4097, 512, 640), (4127, 512, 609))


def test_exact_generators_hold_their_condition_and_the_ambiguity_cap():
    """exact_condition is asserted inside every generator; here for the seeds and shapes of tests/test_gpu_phone_step_ref64.py, with
    the ambiguous share of H2 / H1 / dZ1 (expected about 2 FAST_SIGMOID_ABS / bf16 spacing = 2e-4) at most 1e-3."""
    for m in GPU_L2TAIL_M[:-1]:          # (32 805 and 65 555 rows cost seconds: the GPU tests assert their cap themselves, from the reference alone)
        c, want = _l2tail_case('exact', m, 1.0)
        assert c['sum_abs'] < 2.0 ** 6 and want['shares']['h2'] <= 1e-3, (m, want['shares'])
    c = ref.exact_l2tail(33, 7)                              # the frames form's small case
    want = ref.l2tail_frames(c['h1'], c['w2'], c['b2'], c['w3'], c['b3'], c['w4'], c['b4'], c['ybar'], np.array([11, 1, 8]), 3, 11, 1.0, exact=True)
    assert want['shares']['h2'] <= 1e-3, want['shares']
    for m in GPU_PAIR_M:
        c = ref.exact_pair(m)
        assert c['sum_abs'] < 2.0 ** 14
    # (dZ1 of the exact pair case has no such cap: products of grid values land ON bf16 ties, 1.7 % of the elements - they are
    # ambiguous under any bound above zero, and the other 98.3 % are compared to the bit)
    for m, n, k in GPU_WGRAD:
        assert ref.exact_wgrad(m, n, k)['sum_abs'] < 2.0 ** 14
    c = ref.exact_fwd(4127, 600, 512)
    share = ref.linear_fwd(c['a'], c['w'], c['bias'], 600, exact=True)['shares']['y']
    assert c['sum_abs'] < 2.0 ** 6 and share <= 1e-3, share
    # and a violated condition is caught
    with pytest.raises(AssertionError):
        ref.exact_condition(np.full((70000, 1), 31 / 32), 5, np.full((70000, 1), 31 / 32), 5, over_rows=True)


def test_split_plans_restated():
    """The split plans the bounds' K and the GPU tests' slab counts rest on (gemm_bf16_big.hip, restated): every shape of the GPU tests
    has EMPTY trailing splits."""
    assert ref.pair_plan(4096) == (64, 64) and ref.pair_plan(4127) == (72, 64) and ref.pair_plan(8209) == (88, 96)
    for m in GPU_PAIR_M[1:]:                                 # (m = 4096 is 64 full splits of 64 rows)
        s, chunk = ref.pair_plan(m)
        assert -(-m // chunk) < s
    for m, n, k in GPU_WGRAD:
        s, chunk = ref.wgrad_plan(m, n, k, 640)
        assert (s, chunk) == (32, 160) and -(-m // chunk) == 26
    assert ref.l2tail_blocks(1) == 1 and ref.l2tail_blocks(4127) == 33 and ref.l2tail_blocks(32805) == 256 and ref.l2tail_blocks(65555) == 256


# ------------------------------------------------------------------------------------------------------------ gradients of its own loss
def test_reference_gradients_are_the_derivatives_of_its_loss():
    """Central differences of the float64 loss in pred (through b4), b3 and W3 against db4, db3 and dW3.  dW3 is formed from the
    bf16-rounded dZ3 (as the kernel forms it), so it may differ from the derivative by 2^-9 sum |dZ3| |H2|; db3 and db4 may not."""
    m = 33
    c = ref.tail_h2(m, seed=2)
    w3 = bf16_round(c['w3']).astype(F64)
    h2, w4, y, wt = c['h2'].astype(F64), c['w4'].reshape(-1).astype(F64), c['ybar'].astype(F64), c['weight'].astype(F64)
    want = ref.tail_rows(c['h2'], w3, c['b3'], c['w4'], c['b4'], c['ybar'], c['weight'], 1.0)

    def loss(w3_, b3_, b4_):
        h3 = 1 / (1 + np.exp(-(h2 @ w3_.T + b3_)))
        return float((wt * (h3 @ w4 + b4_ - y) ** 2).sum())

    b3, b4 = c['b3'].astype(F64), float(c['b4'][0])
    assert abs(loss(w3, b3, b4) - want['loss'].v) <= 1e-12 * abs(want['loss'].v)
    h = 1e-6
    fd = (loss(w3, b3, b4 + h) - loss(w3, b3, b4 - h)) / (2 * h)
    assert abs(fd - want['db4'].v) <= 1e-7 * np.abs(want['db4'].v) + 1e-9
    for n in (0, 5, 31):
        d = np.zeros(32)
        d[n] = h
        fd = (loss(w3, b3 + d, b4) - loss(w3, b3 - d, b4)) / (2 * h)
        assert abs(fd - want['db3'].v[n]) <= 1e-6 * np.abs(want['db3'].v).max() + 1e-9, (n, fd, want['db3'].v[n])
    dz3_mag = None
    for n, k in ((0, 0), (7, 100), (31, 127)):
        d = np.zeros((32, 128))
        d[n, k] = h
        fd = (loss(w3 + d, b3, b4) - loss(w3 - d, b3, b4)) / (2 * h)
        if dz3_mag is None:
            h3 = 1 / (1 + np.exp(-(h2 @ w3.T + b3)))
            dpred = 2 * wt * (h3 @ w4 + b4 - y)
            dz3_mag = np.abs(dpred[:, None] * w4 * h3 * (1 - h3)).T @ np.abs(h2)
        assert abs(fd - want['dw3'].v[n, k]) <= 2.0 ** -9 * dz3_mag[n, k] + 1e-9, (n, k, fd, want['dw3'].v[n, k])
