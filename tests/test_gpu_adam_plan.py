"""mg_adam_step_plan_f32 (adam_plan_kernel, csrc/optim.hip) branch by branch against the float64 ``Bounded`` reference of
tests/x3_ref64.py (``-m gpu``, MI355X).  One ops.adam_step_plan call per case on a flat buffer of a few thousand floats; five checks:

1. param, exp_avg, exp_avg_sq: ratio(device, reference) <= 1, the bound carried from the summed gradient (any summation order)
   through every operation of mg_adam_update - recorded with ``note``;
2. the bf16 operand copies: bf16(p_dev), and bf16(p_dev - hi) in the lo half of pair planes, bit for bit from the DEVICE's parameter;
3. their padding columns, the guard elements around them and so everything outside a shadow keep a NaN-pattern sentinel, bit for bit;
4. grad: all zero with clear_grad=True, bit-identical to its input with clear_grad=False (never the summed gradient);
5. the kernel's documented contract: bitwise what ops.slab_reduce(accumulate=True) into the gradient, ops.adam_step_dev and the
   cast / split launches produce.

The deferred-tail rider (plan.tail) is test_deferred_tail_riders_on_synthetic_slabs' and stays out."""
import numpy as np
import pytest
import torch

import x3_ref64 as ref
from morgana_amd import ops
from parity_report import note
from recurrent_ref64 import ratio

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BETAS, EPS_ADAM, LR = (0.9, 0.999), 1e-8, 0.01
NAN_BITS = 0x7fc1          # a bf16 NaN pattern no cast produces (mg_f2bf of a NaN keeps its payload, and no parameter here is NaN)
GUARD = 8

# name: path (the branch of mg_adam_step_plan_f32 the case must take: 'wide' = 2 covered < n), n, sources [(begin, count, n_slabs, stride, lead floats into the slab's storage)], shadows [(offset, rows, cols, kind)],
# then optional weight_decay / grad_scale / step / clear_grad / zero (a stretch with exp_avg_sq = grad = 0).
# kind: 'both' / 'dst' / 'dst_t' plain copies, 'pair' / 'pair_dst' / 'pair_t' [hi | lo] pair planes.
_MIX = [(0, 24, 40, 'both'), (1000, 7, 9, 'dst'), (1100, 16, 8, 'dst_t'), (1300, 24, 40, 'pair'), (2300, 5, 13, 'pair_dst'),
        (2400, 12, 10, 'pair_t'), (2600, 3, 70, 'both'), (2900, 9, 9, 'both')]       # eight; 63, 65 and 81 elements are no multiple of 64
CASES = {
    # ---- wide path (sources cover less than half of n: 256-element chunks) ----
    # no source at all: every chunk takes the one-element-per-thread branch (!hit); n = 1, 255, 257, 1000 end inside a chunk (i < n)
    'wide_none_1': dict(path='wide', n=1), 'wide_none_255': dict(path='wide', n=255), 'wide_none_256': dict(path='wide', n=256), 'wide_none_257': dict(path='wide', n=257),
    'wide_none_1000': dict(path='wide', n=1000, shadows=[(100, 7, 9, 'both'), (300, 24, 20, 'pair')]),       # shadows over ranges with no source
    # one source inside one 256-chunk: chunk 1 runs sub = 3..0 of the summing form (its last 64-chunk sees no source: block_any false)
    'wide_inside': dict(path='wide', n=3000, sources=[(300, 100, 5, 104, 0)], shadows=[(300, 10, 10, 'both')]),
    # one source over a 256 boundary: chunks 0 and 1 both hit; begin % 4 == 0, stride % 4 == 0: the 16-byte loads
    'wide_straddle': dict(path='wide', n=3000, sources=[(200, 120, 17, 120, 0)]),
    # a source ending at n, n % 64 = 37 = n % 256: the last 256-chunk runs sub = 0 only (sbase + 64 sub < n), its threads 37.. idle
    'wide_end': dict(path='wide', n=2085, sources=[(1935, 150, 16, 152, 0)], shadows=[(1935, 15, 10, 'pair')]),
    # two sources in neighbouring 64-chunks of one 256-chunk (512..575 and 576..639)
    'wide_neighbours': dict(path='wide', n=3000, sources=[(522, 50, 3, 50, 0), (581, 40, 33, 44, 0)]),
    # ---- narrow path (covered >= n / 2: 64-element chunks) ----
    # four sources back to back, boundaries at multiples of 4 (16-byte loads throughout) ...
    'narrow_four_aligned': dict(path='narrow', n=1000, sources=[(0, 200, 2, 200, 0), (200, 240, 15, 240, 0), (440, 160, 16, 160, 0), (600, 300, 17, 300, 0)]),
    # ... and at 201, 439, 602: a 4-group belongs to two sources, a boundary falls inside a 64-chunk, the element-wise loads
    'narrow_four_ragged': dict(path='narrow', n=1000, sources=[(0, 201, 2, 204, 0), (201, 238, 15, 240, 0), (439, 163, 16, 164, 0), (602, 298, 17, 300, 0)],
                               shadows=[(201, 14, 17, 'both'), (602, 10, 29, 'pair'), (900, 10, 10, 'dst')]),
    'narrow_begin_odd': dict(path='narrow', n=1000, sources=[(37, 700, 5, 704, 0)]),            # begin % 4 != 0, stride % 4 == 0
    'narrow_stride_odd': dict(path='narrow', n=1000, sources=[(36, 700, 5, 701, 0)]),           # begin % 4 == 0, stride % 4 != 0
    'narrow_base_unaligned': dict(path='narrow', n=1000, sources=[(64, 700, 5, 704, 1)]),       # the slab a view one float into its storage; all else aligned
    'narrow_slabs_1': dict(path='narrow', n=1000, sources=[(64, 800, 1, 800, 0)]), 'narrow_slabs_15': dict(path='narrow', n=1000, sources=[(64, 800, 15, 800, 0)]),
    'narrow_slabs_16': dict(path='narrow', n=1000, sources=[(64, 800, 16, 800, 0)]), 'narrow_slabs_17': dict(path='narrow', n=1000, sources=[(64, 800, 17, 800, 0)]),
    'narrow_slabs_33': dict(path='narrow', n=1000, sources=[(64, 800, 33, 800, 0)], shadows=[(64, 20, 40, 'both')]),
    'narrow_end_ragged': dict(path='narrow', n=1003, sources=[(300, 703, 4, 703, 0)]),          # the last 64-chunk ends at n inside a source
    # ---- shadows: eight at once, every kind; a source without a shadow (3100..) and shadows without a source; both paths ----
    'shadows_wide': dict(path='wide', n=4000, sources=[(0, 1000, 5, 1000, 0), (3100, 300, 3, 300, 0)], shadows=_MIX),
    'shadows_narrow': dict(path='narrow', n=4000, sources=[(0, 1000, 5, 1000, 0), (1300, 960, 2, 960, 0), (3100, 300, 3, 300, 0)], shadows=_MIX),
    # ---- clear_grad=False, and the stretch where denom = eps ----
    'keep_grad_wide': dict(path='wide', n=3000, sources=[(200, 120, 17, 120, 0)], shadows=[(200, 10, 12, 'both')], clear_grad=False),
    'keep_grad_narrow': dict(path='narrow', n=1000, sources=[(0, 201, 2, 204, 0), (201, 700, 15, 700, 0)], shadows=[(201, 14, 17, 'pair')], clear_grad=False),
    'zero_stretch': dict(path='wide', n=2000, sources=[(0, 300, 5, 300, 0)], shadows=[(1500, 10, 10, 'pair')], zero=(1450, 1650), weight_decay=0.0),
}
for _wd in (0.0, 1e-2):
    for _gs in (1.0, 1.0 / 3.0):
        for _step in (1, 1000):
            CASES['scalars_wd%g_gs%.2f_step%d' % (_wd, _gs, _step)] = dict(
                path='narrow', n=1000, sources=[(0, 201, 2, 204, 0), (201, 338, 15, 340, 0)], shadows=[(201, 14, 17, 'both')], weight_decay=_wd, grad_scale=_gs,
                step=_step)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _sentinel_buffer(rows, ld):
    """(whole, view): a bf16 (rows, ld) view GUARD elements into an allocation filled with the NaN sentinel."""
    whole = torch.full((GUARD + rows * ld + GUARD,), NAN_BITS, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    return whole, whole[GUARD:GUARD + rows * ld].view(rows, ld)


def _inputs(spec, seed):
    n = spec['n']
    rng = np.random.RandomState(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 0.1).astype(np.float32)
    m = (rng.standard_normal(n) * 0.01).astype(np.float32)
    v = rng.uniform(1e-4, 1e-2, n).astype(np.float32)
    if spec.get('zero'):
        lo, hi = spec['zero']
        v[lo:hi], g[lo:hi] = 0.0, 0.0
    slabs = [(rng.standard_normal((n_slabs, stride)) * 0.05).astype(np.float32) for _, _, n_slabs, stride, _ in spec.get('sources', ())]
    return p, g, m, v, slabs


def _device_sources(spec, slabs):
    out, keep = [], []
    for (begin, count, n_slabs, stride, lead), values in zip(spec.get('sources', ()), slabs):
        store = torch.full((lead + n_slabs * stride + 3,), 7.0, dtype=torch.float32, device=DEV)
        view = store[lead:lead + n_slabs * stride].view(n_slabs, stride)
        view.copy_(dev(values))
        assert (view.data_ptr() % 16 == 0) == (lead % 4 == 0)
        keep.append(store)
        out.append((begin, count, view, n_slabs, stride))
    return out, keep


def _device_shadows(spec):
    """-> plan entries, and per shadow (kind, rows, cols, (whole, view) of dst or None, (whole, view) of dst_t or None)."""
    entries, held = [], []
    for offset, rows, cols, kind in spec.get('shadows', ()):
        pair = kind.startswith('pair')
        ldd, ldt = ops.pad_ld(cols) * (2 if pair else 1), ops.pad_ld(rows) * (2 if pair else 1)
        d = _sentinel_buffer(rows, ldd) if kind in ('both', 'dst', 'pair', 'pair_dst') else None
        t = _sentinel_buffer(cols, ldt) if kind in ('both', 'dst_t', 'pair', 'pair_t') else None
        entries.append((offset, rows, cols, d[1] if d else None, t[1] if t else None, pair))
        held.append((offset, rows, cols, pair, d, t))
    return entries, held


def _run(spec, seed):
    p, g, m, v, slabs = _inputs(spec, seed)
    wd, gs, step = spec.get('weight_decay', 1e-2), spec.get('grad_scale', 0.5), spec.get('step', 3)
    clear = spec.get('clear_grad', True)
    sc = ops.adam_scalars(LR, BETAS, step)
    scalars = torch.tensor(sc, dtype=torch.float32, device=DEV)
    sources, keep = _device_sources(spec, slabs)
    entries, held = _device_shadows(spec)
    got = [dev(x) for x in (p, g, m, v)]
    ops.adam_step_plan(got[0], got[1], got[2], got[3], BETAS, EPS_ADAM, wd, scalars, gs, slab_srcs=sources, shadows=entries, clear_grad=clear)
    torch.cuda.synchronize()
    return dict(p=p, g=g, m=m, v=v, slabs=slabs, wd=wd, gs=gs, sc=sc, scalars=scalars, clear=clear, sources=sources, keep=keep, held=held,
                got=got)


def _check(name, spec, r):
    n = spec['n']
    p_dev, g_dev, m_dev, v_dev = (t.cpu().numpy() for t in r['got'])
    # 1. the float64 reference, every bound carried from the summed gradient
    ref_sources = [(b, c, vals) for (b, c, _, _, _), vals in zip(spec.get('sources', ()), r['slabs'])]
    want = ref.adam_plan(r['p'], r['g'], r['m'], r['v'], BETAS, EPS_ADAM, r['wd'], r['sc'], r['gs'], ref_sources)
    for label, x, b in zip(('param', 'exp_avg', 'exp_avg_sq'), (p_dev, m_dev, v_dev), want):
        assert np.all(np.isfinite(b.e)), label
        q = note(ratio(x, b), '%s %s' % (name, label), bound=1.0)
        print('%-34s %-10s observed / bound = %.4f' % (name, label, q))
        assert q <= 1.0, (name, label, q)
    # 4. the gradient buffer
    if r['clear']:
        assert not g_dev.any()
    else:
        assert np.array_equal(g_dev.view(np.uint32), r['g'].view(np.uint32))
    # 5. the documented contract: reduce launches into the gradient, mg_adam_step_dev_f32, casts - bit for bit
    p2, g2, m2, v2 = (dev(x) for x in (r['p'], r['g'], r['m'], r['v']))
    for begin, count, view, n_slabs, stride in r['sources']:
        ops.slab_reduce(view, n_slabs, stride, count, g2[begin:begin + count], accumulate=True)
    ops.adam_step_dev(p2, g2, m2, v2, BETAS, EPS_ADAM, r['wd'], r['scalars'], r['gs'])
    assert torch.equal(r['got'][0], p2) and torch.equal(r['got'][2], m2) and torch.equal(r['got'][3], v2)
    # 2. + 3. shadows from the device's parameter, sentinels everywhere else
    for offset, rows, cols, pair, d, t in r['held']:
        hi, lo = ref.shadow_bits(p_dev, offset, rows, cols)
        w2d = p2[offset:offset + rows * cols].view(rows, cols)
        for held, transposed in ((d, False), (t, True)):
            if held is None:
                continue
            whole, view = held
            r_, c_ = (cols, rows) if transposed else (rows, cols)
            want_bits = np.full(tuple(view.shape), NAN_BITS, dtype=np.uint16)
            want_bits[:, :c_] = hi.T if transposed else hi
            if pair:
                half = view.shape[1] // 2
                want_bits[:, half:half + c_] = lo.T if transposed else lo
            assert np.array_equal(_bits(view), want_bits), (name, offset, transposed)
            guards = _bits(whole)
            assert (guards[:GUARD] == NAN_BITS).all() and (guards[-GUARD:] == NAN_BITS).all()
            # the launches the kernel replaces
            if pair:
                cast = ops.split_pair(w2d.contiguous(), transpose=transposed)
                assert cast.shape == view.shape
                assert torch.equal(cast[:, :c_], view[:, :c_]) and torch.equal(cast[:, half:half + c_], view[:, half:half + c_])
            else:
                cast = ops.cast_transpose_bf16(w2d.contiguous()) if transposed else ops.cast_pad_bf16(w2d.contiguous())
                assert cast.shape == view.shape and torch.equal(cast[:, :c_], view[:, :c_])
    return p_dev, m_dev, v_dev


@pytest.mark.parametrize('name', sorted(CASES))
def test_plan_case(name):
    spec = CASES[name]
    covered = sum(s[1] for s in spec.get('sources', ()))
    assert (2 * covered < spec['n']) == (spec['path'] == 'wide'), 'the case must take the path it names'
    _check(name, spec, _run(spec, seed=len(name) + spec['n']))


def test_host_adam_scalars_are_the_librarys():
    """x3_ref64.adam_scalars (the host test's, no library) against ops.adam_scalars (mg_adam_scalars), bit for bit."""
    for step in (1, 3, 1000):
        want = np.array(ops.adam_scalars(LR, BETAS, step), dtype=np.float32)
        got = np.array(ref.adam_scalars(LR, BETAS, step), dtype=np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), step


def test_zero_stretch_takes_denom_eps():
    """exp_avg_sq = 0 and grad = 0 on a stretch (weight_decay 0): v' = 0 exactly, m' = m beta1 within its bound, denom = eps - the
    parameter moves by step_size m' / eps, inside the bound the same propagation gives (no tolerance of its own)."""
    spec = CASES['zero_stretch']
    r = _run(spec, seed=11)
    p_dev, m_dev, v_dev = _check('zero_stretch', spec, r)
    lo, hi = spec['zero']
    assert not v_dev[lo:hi].any()
    move = np.abs(p_dev[lo:hi].astype(np.float64) - r['p'][lo:hi])
    assert np.median(move) > 1.0 and np.all(np.isfinite(p_dev))     # |m| 0.9 step_size / 1e-8: far from a no-op


def test_wide_and_narrow_paths_agree_bit_for_bit():
    """The same data embedded so that the path flips: one source (200, 300) in n = 3000 (wide: 600 < 3000) and in the first 560
    elements alone (narrow: 600 >= 560).  Parameters, moments and the copies of the overlapping elements are bit-equal."""
    wide = dict(path='wide', n=3000, sources=[(200, 300, 17, 300, 0)], shadows=[(200, 15, 20, 'pair')])
    narrow = dict(wide, path='narrow', n=560)
    rw = _run(wide, seed=5)
    p, g, m, v, slabs = _inputs(wide, 5)
    sc = ops.adam_scalars(LR, BETAS, 3)
    scalars = torch.tensor(sc, dtype=torch.float32, device=DEV)
    sources, keep = _device_sources(narrow, slabs)
    entries, held = _device_shadows(narrow)
    got = [dev(x[:560]) for x in (p, g, m, v)]
    ops.adam_step_plan(got[0], got[1], got[2], got[3], BETAS, EPS_ADAM, 1e-2, scalars, 0.5, slab_srcs=sources, shadows=entries, clear_grad=True)
    for i in (0, 2, 3):
        assert torch.equal(got[i], rw['got'][i][:560]), i
    assert not bool(got[1].any())
    for (_, _, _, _, d, t), (_, _, _, _, dw, tw) in zip(held, rw['held']):
        assert torch.equal(d[0].view(torch.int16), dw[0].view(torch.int16)) and torch.equal(t[0].view(torch.int16), tw[0].view(torch.int16))


def test_argument_checks_refuse_before_any_launch():
    """What mg_adam_step_plan_f32 documents as refused - a source past n, stride < count, a fifth source, a ninth shadow, pair planes
    with an odd leading dimension - raises ValueError on the host and leaves every buffer as it was."""
    n = 1000
    rng = np.random.RandomState(9)
    start = [rng.standard_normal(n).astype(np.float32) for _ in range(4)]
    start[3] = np.abs(start[3]) * 0.01
    bufs = [dev(x) for x in start]
    scalars = torch.tensor(ops.adam_scalars(LR, BETAS, 1), dtype=torch.float32, device=DEV)
    slab = torch.ones((2, 64), dtype=torch.float32, device=DEV)
    whole, plain = _sentinel_buffer(10, 16)
    whole_odd, odd = _sentinel_buffer(10, 33)

    def refused(**kw):
        with pytest.raises(ValueError):
            ops.adam_step_plan(bufs[0], bufs[1], bufs[2], bufs[3], BETAS, EPS_ADAM, 0.0, scalars, 1.0, clear_grad=True, **kw)
        torch.cuda.synchronize()
        for b, x in zip(bufs, start):
            assert np.array_equal(b.cpu().numpy().view(np.uint32), x.view(np.uint32))
        assert (_bits(whole) == NAN_BITS).all() and (_bits(whole_odd) == NAN_BITS).all()

    refused(slab_srcs=[(n - 4, 16, slab, 1, 64)])                              # a source past n
    refused(slab_srcs=[(0, 64, slab, 2, 63)])                                  # stride < count
    refused(slab_srcs=[(64 * i, 64, slab, 2, 64) for i in range(5)])           # a fifth source
    refused(shadows=[(10 * i, 10, 10, plain, None) for i in range(9)])         # a ninth shadow
    refused(shadows=[(0, 10, 16, odd, None, True)])                            # pair planes, odd ldd
    refused(shadows=[(0, 10, 10, plain, None, True)])                          # pair planes whose half (8) does not cover 10 columns
    refused(shadows=[(n - 50, 10, 10, plain, None)])                           # a shadow past n
