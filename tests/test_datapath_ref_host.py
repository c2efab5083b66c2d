"""What tests/datapath_ref.py is worth, shown without a GPU:

1. its exact-family references equal oracle/ref_cpu.py wherever the oracle has the function, and its bounded-family references agree
   with the oracle's formulas evaluated in float64 to 1e-12 relative;
2. a float32 numpy EMULATION of each bounded kernel, in the kernel's own order of operations, passes its bound on every case of the
   GPU test (tests/test_gpu_datapath.py) - the worst ratio per check is recorded and printed;
3. each fault of FAULTS, applied to the emulation, makes the matching check fail.

The emulations restate csrc/loss_norm.hip, metrics.hip, optim.hip and upsample.hip operation by operation in np.float32 (an fma is the
float64 result rounded once).  They are not references: they exist to show that the bounds admit a correct kernel and refuse a
broken one."""
import contextlib

import numpy as np
import pytest

import datapath_ref as R
from oracle import ref_cpu

F32 = np.float32
F64 = np.float64
RATIOS = {}            # check -> worst error / bound of the emulation
CAUGHT = {}            # fault -> checks that failed under it

FAULTS = ('mask off by one frame', 'mask edge per 4-vector', 'one chunk partial dropped', 'utterance 256 dropped by the finish',
          'n_b not clamped to T', 'coef without D', 'BCE gradient clamp removed', 'stream col0 off by one',
          'column walk not wrapped at D >= 256', 'last partial bf16 chunk unwritten', 'last partial bf16 chunk unzeroed',
          '-1 row read as row 0', 'one phone one frame short', 'padded frame counted in a metric', 'width counted in place of frames')


def _ratio(check, err, bound):
    with np.errstate(all='ignore'):
        r = float(np.max(np.where(np.asarray(bound) > 0, np.asarray(err) / np.maximum(bound, 1e-300), np.where(np.asarray(err) > 0, np.inf, 0.0))))
    RATIOS[check] = max(RATIOS.get(check, 0.0), r)
    return r


def _within(got, want, bound):
    """Every element within its bound; a NaN wanted must be a NaN got and the other way round."""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    nan_ok = np.array_equal(np.isnan(got), np.isnan(want))
    with np.errstate(all='ignore'):
        return bool(nan_ok and np.all((np.abs(got - want) <= bound) | np.isnan(want)))


def _err(got, want):
    with np.errstate(all='ignore'):
        e = np.abs(np.asarray(got, dtype=F64) - np.asarray(want, dtype=F64))
    return np.where(np.isnan(e), 0.0, e)


class _F64Rounded(np.float64):
    """Stands in for the oracle's F32 while its formulas are evaluated in float64: as a dtype it is float64, as a constructor of a
    PYTHON-number constant it rounds through float32 first - the constants the oracle (and torch) hold in float32 stay those values -
    while a numpy value (a result on its way out) passes unrounded."""

    def __new__(cls, value):
        return np.float64(value) if isinstance(value, (np.generic, np.ndarray)) else np.float64(np.float32(value))


@contextlib.contextmanager
def _oracle_in_float64():
    saved = ref_cpu.F32
    ref_cpu.F32 = _F64Rounded
    try:
        yield
    finally:
        ref_cpu.F32 = saved


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(all='ignore'):
        return bool(np.all(both_nan | (np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b)))))


def test_the_oracle_really_runs_in_float64_under_the_patch():
    """Pins `_oracle_in_float64`: numpy takes the subclass as the float64 dtype, Python constants round through float32, numpy values
    pass; under it the oracle returns float64 results that differ from its float32 evaluation by float32 rounding and no more; and the
    oracle's own F32 is back afterwards.  An np.float32 literal added to one of these oracle functions would fail here, not silently
    turn the 1e-12 comparisons below into float32 ones."""
    assert np.dtype(_F64Rounded) == np.dtype(np.float64)
    assert _F64Rounded(0.1) == float(F32(0.1)) != 0.1 and _F64Rounded(np.float64(0.1)) == 0.1
    pred, target, seq_len = R.masked_case(2731, 3, 'bce')
    spred, stargets, skinds, slen = R.stream_case('d257')
    skinds = ['mse' if k == 'mse' else 'bce' for k in skinds]
    calls = [lambda: ref_cpu.mse(pred, target, seq_len), lambda: ref_cpu.mse_grad(pred, target, seq_len),
             lambda: ref_cpu.bce(pred, target, seq_len), lambda: ref_cpu.bce_grad(pred, target, seq_len),
             lambda: ref_cpu.multi_stream_loss(spred, stargets, skinds, slen)[0],
             lambda: ref_cpu.multi_stream_loss(spred, stargets, skinds, slen)[1],
             lambda: ref_cpu.normalise_mvn(pred, target[0, 0], np.abs(target[0, 1]) + F32(0.5))]
    for call in calls:
        with np.errstate(all='ignore'):
            narrow = call()
            with _oracle_in_float64():
                wide = call()
        assert np.asarray(narrow).dtype == np.float32 and np.asarray(wide).dtype == np.float64
        diff = np.abs(np.asarray(wide) - np.asarray(narrow, dtype=F64))
        assert diff.max() > 0                                                   # not the float32 evaluation in a wider type
        assert np.all(diff <= 1e-4 * np.abs(wide) + 1e-30)                      # and the same formula
    assert ref_cpu.F32 is np.float32
    # the Adam class: float64 state stays float64 through a step
    with _oracle_in_float64():
        p = np.array([0.3, -0.7])
        opt = ref_cpu.Adam([p], lr=0.01)
        opt.step([np.array([1e-3, 2.0])])
        assert p.dtype == np.float64 and opt.m[0].dtype == np.float64 and opt.v[0].dtype == np.float64
        assert opt.m[0][1] == 2.0 * float(F32(1.0 - 0.9))                       # the constant F32(1.0 - b1): float32 value, float64 product


def test_the_wrappers_phone_limit_is_the_kernels():
    """ops.MAX_PHONES restates MG_MAX_PHONES of csrc/upsample.hip (the wrappers refuse first, so that no library call is logged): the
    two and the reference's copy are held together here."""
    import os
    import re
    from morgana_amd import ops
    src = open(os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), 'csrc', 'upsample.hip')).read()
    found = re.findall(r'^#define\s+MG_MAX_PHONES\s+(\d+)\s*$', src, flags=re.M)
    assert len(found) == 1 and int(found[0]) == ops.MAX_PHONES == R.MAX_PHONES


# ======================================================================================= 1. the references against the oracle
DUR_CASES = {
    'plain': np.array([[2, 3, 1, 4], [1, 1, 1, 1]], dtype=np.int64),
    'zeros': np.array([[0, 0, 3, 0, 2, 0, 0], [0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 7, 0, 0, 0]], dtype=np.int64),
}


@pytest.mark.parametrize('name', sorted(DUR_CASES))
def test_index_maps_equal_the_oracle(name):
    dur = DUR_CASES[name]
    want, lens = ref_cpu.upsample_index(dur)
    assert np.array_equal(R.upsample_index(dur, want.shape[1]), want)
    n_frames, tmax = R.upsample_lengths(dur)
    assert np.array_equal(n_frames, lens) and int(tmax) == want.shape[1]
    rows, mapped, seg = R.upsample_index_maps(dur, want.shape[1])
    b, p = dur.shape
    assert np.array_equal(rows, np.where(want < 0, -1, want + (np.arange(b) * p)[:, None]))
    assert np.array_equal(mapped == b * p, want < 0)
    for i in range(b):                                     # a phone's run names exactly the frames the oracle's map gives it
        for q in range(p):
            frames = np.nonzero(want[i] == q)[0] + i * want.shape[1]
            s, e = seg[0, i * p + q], seg[1, i * p + q]
            assert np.array_equal(np.arange(s, e), frames)


@pytest.mark.parametrize('name', sorted(DUR_CASES))
def test_upsample_backward_equals_the_oracle(name):
    dur = DUR_CASES[name]
    t = int(ref_cpu.upsample_index(dur)[0].shape[1])
    g = np.random.RandomState(1).standard_normal((dur.shape[0], t, 5)).astype(F32)
    ref = R.upsample_backward(g, dur, dur.shape[1])
    assert R.bits_equal_f32(ref['exact'], ref_cpu.upsample_backward(g, dur, dur.shape[1]))       # np.add.at adds in ascending t too
    assert np.all(np.abs(ref['exact'].astype(F64) - ref['sum']) <= ref['bound'])


def test_segment_maps_equal_the_oracle():
    lens = np.array([[2, 0, 3, 1], [1, 4, 0, 0]], dtype=np.int64)
    t = 6
    x = np.random.RandomState(2).standard_normal((2, t, 3)).astype(F32)
    split, ends = R.segment_index(lens, t, int(lens.max()))
    flat = np.concatenate([x.reshape(-1, 3), np.zeros((1, 3), dtype=F32)])
    assert np.array_equal(flat[split], ref_cpu.split_to_segments(x, lens))                        # -1 indexes the zero row
    assert np.array_equal(flat[ends], ref_cpu.get_segment_ends(x, lens))


@pytest.mark.parametrize('dtype', [np.uint8, np.bool_, np.int8, np.float32, np.int32, np.int64, np.float64])
def test_sequence_mask_equals_the_oracle(dtype):
    seq_len = np.array([0, 3, 9, 12], dtype=np.int64)
    for max_len in (0, 1, 9):
        assert np.array_equal(R.sequence_mask(seq_len, max_len, dtype), ref_cpu.sequence_mask(seq_len, max_len, dtype))


@pytest.mark.parametrize('kind', ['mse', 'bce'])
@pytest.mark.parametrize('shape', R.MASKED_SHAPES)
def test_masked_loss_reference_agrees_with_the_oracle(shape, kind):
    pred, target, seq_len = R.masked_case(shape[0], shape[1], kind)
    for sl in (seq_len, None):
        ref = R.masked_loss(pred, target, sl, kind=kind)
        with _oracle_in_float64(), np.errstate(all='ignore'):
            loss = getattr(ref_cpu, kind)(pred, target, sl)
            grad = getattr(ref_cpu, kind + '_grad')(pred, target, sl)
        assert _close(ref['loss'], loss) and _close(ref['grad'], grad)


def test_masked_loss_reference_agrees_with_the_oracle_on_an_empty_utterance():
    for kind in ('mse', 'bce'):
        pred, target, seq_len = R.masked_nan_case(kind)
        ref = R.masked_loss(pred, target, seq_len, kind=kind)
        with _oracle_in_float64(), np.errstate(all='ignore'):
            loss = getattr(ref_cpu, kind)(pred, target, np.maximum(seq_len, 0))       # the oracle's mask takes no negative length
            grad = getattr(ref_cpu, kind + '_grad')(pred, target, np.maximum(seq_len, 0))
        assert np.isnan(ref['loss']) and np.isnan(loss)
        assert np.all(np.isnan(ref['grad'][:2])) and _close(ref['grad'][2], grad[2])


@pytest.mark.parametrize('name', [c[0] for c in R.STREAM_CASES])
def test_stream_loss_reference_agrees_with_the_oracle(name):
    pred, targets, kinds, seq_len = R.stream_case(name)
    ref = R.stream_loss(pred, targets, kinds, seq_len)
    oracle_kinds = ['mse' if k == 'mse' else 'bce' for k in kinds]
    with _oracle_in_float64(), np.errstate(all='ignore'):
        loss, grad = ref_cpu.multi_stream_loss(pred, targets, oracle_kinds, seq_len)
    if np.any(seq_len == 0):
        assert np.isnan(ref['loss']) and np.isnan(loss)
        live = seq_len > 0
        assert _close(ref['grad'][live], grad[live]) and np.all(np.isnan(ref['grad'][~live]))
        return
    assert _close(ref['loss'], loss)
    # the oracle's sigmoid gradient is (p - y) / max((1 - p) p, 1e-12) * (1 - p) p like the kernel's: equal to 1e-12 where the factor is
    # not clamped; the saturated logits (|x| = 40) are compared through the bound instead
    sat = np.zeros(pred.shape, dtype=bool)
    col = 0
    for y, k in zip(targets, kinds):
        if k != 'mse':
            sat[:, :, col:col + y.shape[2]] = np.abs(pred[:, :, col:col + y.shape[2]]) >= 30
        col += y.shape[2]
    assert _close(ref['grad'][~sat], grad[~sat])
    assert np.all(np.abs(ref['grad'][sat] - grad[sat]) <= ref['grad_bound'][sat])


def test_metric_reference_agrees_with_the_oracle():
    for shape in R.METRIC_SHAPES:
        b, t, d, col0, width = shape
        for grid in (True, False):
            target, pred, voiced, seq_len = R.metric_case(shape, grid=grid)
            for kind in R.METRIC_KINDS:
                for sl in (seq_len, None):
                    total, count, bound = R.metric_sums(kind, target, pred, voiced, sl, col0=col0)
                    want_total, want_count = ref_cpu.metric_sums(kind, target, pred, voiced, sl, col0=col0)
                    assert count == want_count, (kind, shape)
                    # the oracle forms every element in float32: to 1e-12 where that is exact (grid values, no sqrt / exp), else within
                    # the float32 bound of the same elements
                    if grid and kind not in ('root_sq', 'sqdiff_voiced_exp'):
                        assert _close(total, want_total), (kind, shape)
                    else:
                        assert abs(total - want_total) <= bound, (kind, shape)
                    assert R.metric_result(kind, total, count) == pytest.approx(ref_cpu.metric_result(kind, total, count), rel=1e-15)


@pytest.mark.parametrize('weight_decay', [0.0, 1e-2])
@pytest.mark.parametrize('n', R.ADAM_SIZES)
def test_adam_reference_agrees_with_the_oracle(n, weight_decay):
    param, grads = R.adam_case(n)
    betas = tuple(float(F32(x)) for x in R.ADAM_BETAS)
    with _oracle_in_float64():
        p = param.astype(F64)
        opt = ref_cpu.Adam([p], lr=float(F32(R.ADAM_LR)), weight_decay=float(F32(weight_decay)), betas=betas, eps=float(F32(R.ADAM_EPS)))
        mine_p, mine_m, mine_v = param.astype(F64), np.zeros(n), np.zeros(n)
        for step, g in enumerate(grads, 1):
            opt.step([g.astype(F64)])
            # the scalars as the oracle forms them there: step_size a Python float (rounded to float32), sqrt(bc2) a numpy value (not)
            ss, bc = R.adam_scalars(R.ADAM_LR, betas, step)[0], np.sqrt(1.0 - betas[1] ** step)
            # one reference step from the float64 state (no float32 rounding in between): pass the state through unrounded
            mine_p, mine_m, mine_v = _adam64(mine_p, g, mine_m, mine_v, ss, bc, betas, R.ADAM_EPS, weight_decay)
            assert _close(mine_p, p) and _close(mine_m, opt.m[0]) and _close(mine_v, opt.v[0])


def _adam64(p, g, m, v, ss, bc, betas, eps, wd):
    """R.adam_step's arithmetic on float64 STATE (R.adam_step itself takes float32 state): the same lines, for the multi-step comparison."""
    b1, b2 = float(F32(betas[0])), float(F32(betas[1]))
    g2 = g.astype(F64) + float(F32(wd)) * p if wd else g.astype(F64)
    m2 = m + (g2 - m) * (1.0 - b1)
    v2 = (1.0 - b2) * g2 * g2 + v * b2
    return p - float(ss) * (m2 / (np.sqrt(v2) / float(bc) + float(F32(eps)))), m2, v2


def test_adam_reference_one_step_is_the_float64_restatement():
    param, grads = R.adam_case(1025)
    ss, bc = R.adam_scalars(R.ADAM_LR, R.ADAM_BETAS, 1)
    m = v = np.zeros(1025, dtype=F32)
    got = R.adam_step(param, grads[0], m, v, ss, bc, R.ADAM_BETAS, R.ADAM_EPS, 1e-2, 0.5)
    want = _adam64(param.astype(F64), grads[0].astype(F64) * 0.5, m.astype(F64), v.astype(F64), ss, bc, R.ADAM_BETAS, R.ADAM_EPS, 1e-2)
    for a, w in zip(got[:3], want):
        assert _close(a, w)


@pytest.mark.parametrize('decay', [0.0, 0.999, 1.0])
@pytest.mark.parametrize('n', R.ADAM_SIZES)
def test_ema_reference_agrees_with_the_oracle(n, decay):
    rng = np.random.RandomState(n)                        # the inputs of the emulation and GPU tests at this n
    s, p = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    got, _ = R.ema_update(s, p, decay)
    with _oracle_in_float64():
        want = ref_cpu.ema_update(s.astype(F64), p.astype(F64), decay)
    assert _close(got, want)


@pytest.mark.parametrize('kind', [R.NORM_MVN, R.DENORM_MVN, R.NORM_MINMAX, R.DENORM_MINMAX])
def test_normalise_reference_agrees_with_the_oracle(kind):
    fn = {R.NORM_MVN: ref_cpu.normalise_mvn, R.DENORM_MVN: ref_cpu.denormalise_mvn, R.NORM_MINMAX: ref_cpu.normalise_minmax,
          R.DENORM_MINMAX: ref_cpu.denormalise_minmax}[kind]
    for rows, d in R.NORMALISE_SHAPES:
        x, p0, p1 = R.normalise_case(rows, d, kind)
        got, _ = R.normalise(x, p0, p1, kind)
        with _oracle_in_float64():
            want = fn(x.astype(F64)[None], p0.astype(F64), p1.astype(F64))[0]
        assert _close(got, want)


# ==================================================================================================== 2. the float32 emulations
def _wave_sums(v):
    """256 thread values -> the four wave sums of the xor butterfly (mg_wave_sum)."""
    v = v.astype(F32).reshape(4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lane ^ off]).astype(F32)
    return v[:, 0]


def _tree256(red):
    red = red.astype(F32).copy()
    off = 128
    while off > 0:
        red[:off] = (red[:off] + red[off:2 * off]).astype(F32)
        off //= 2
    return red[0]


def _emu_reduce(terms, n_div, vec4, final_div, fault=None):
    """stage 1 + the finish of the masked losses.  terms (B, row_elems) float32 (already masked); n_div (B,) the finish's divisors."""
    b, row = terms.shape
    chunks = (row + R.MSE_CHUNK - 1) // R.MSE_CHUNK
    partial = np.zeros((b, chunks), dtype=F32)
    for i in range(b):
        for c in range(chunks):
            vals = np.zeros(R.MSE_CHUNK, dtype=F32)
            seg = terms[i, c * R.MSE_CHUNK:(c + 1) * R.MSE_CHUNK]
            vals[:seg.size] = seg
            per = vals.reshape(8, 256, 4).transpose(1, 0, 2).reshape(256, 32) if vec4 else vals.reshape(32, 256).T
            acc = np.zeros(256, dtype=F32)
            for k in range(32):
                acc = (acc + per[:, k]).astype(F32)
            w = _wave_sums(acc)
            partial[i, c] = F32(F32(w[0] + w[1]) + F32(w[2] + w[3]))
    if fault == 'one chunk partial dropped':
        partial[:, -1] = 0.0
    red = np.zeros(256, dtype=F32)
    with np.errstate(all='ignore'):
        for i in range(b):
            if fault == 'utterance 256 dropped by the finish' and i >= 256:
                continue
            s = F32(0.0)
            for c in range(chunks):
                s = F32(s + partial[i, c])
            red[i % 256] = F32(red[i % 256] + F32(s / F32(n_div[i])))
        return F32(_tree256(red) / F32(final_div))


def _emu_bce_elem(p, y, fault=None):
    with np.errstate(all='ignore'):
        lp = np.maximum(np.log(p), F32(-100.0)).astype(F32)
        lq = np.maximum(np.log((F32(1.0) - p).astype(F32)), F32(-100.0)).astype(F32)
        l = (-((y * lp).astype(F32) + ((F32(1.0) - y).astype(F32) * lq).astype(F32))).astype(F32)
        den = ((F32(1.0) - p).astype(F32) * p).astype(F32)
        if fault != 'BCE gradient clamp removed':
            den = np.maximum(den, F32(1e-12))
        dl = ((p - y).astype(F32) / den).astype(F32)
    return l, dl


def emu_masked_loss(pred, target, seq_len, kind, grad_scale=1.0, vec4=True, fault=None):
    """masked_mse_stage1<VEC4, KIND> + masked_mse_stage2 in float32 -> (loss, grad)."""
    p, y = np.asarray(pred, dtype=F32), np.asarray(target, dtype=F32)
    b, t, d = p.shape
    raw = np.full(b, t, dtype=np.int64) if seq_len is None else np.asarray(seq_len, dtype=np.int64)
    n = np.clip(raw, 0, t)
    n1 = np.maximum(raw, 0) if fault == 'n_b not clamped to T' else n
    if kind == 'mse':
        diff = (p - y).astype(F32)
        l, dl = (diff * diff).astype(F32), (F32(2.0) * diff).astype(F32)
    else:
        l, dl = _emu_bce_elem(p, y, fault)
    e = np.arange(t * d)[None, :]
    valid = ((n1 + (1 if fault == 'mask off by one frame' else 0)) * d)[:, None]
    m = ((e - e % 4 if fault == 'mask edge per 4-vector' else e) < valid).astype(F32).reshape(b, t, d)
    with np.errstate(all='ignore'):
        denom = F32(b) if fault == 'coef without D' else F32(b * d)
        coef = (F32(grad_scale) / (n1.astype(F32) * denom).astype(F32)).astype(F32)
        grad = ((dl * m).astype(F32) * coef[:, None, None]).astype(F32)
        loss = _emu_reduce((l * m).astype(F32).reshape(b, -1), n1, vec4, b * d, fault)
    return loss, grad


def emu_stream_loss(pred, targets, kinds, seq_len, grad_scale=1.0, fault=None):
    """stream_loss_stage1 + the finish in float32 -> (loss, grad, prob)."""
    x = np.asarray(pred, dtype=F32)
    b, t, d = x.shape
    n = np.clip(np.asarray(seq_len, dtype=np.int64), 0, t)
    widths = [y.shape[2] for y in targets]
    col0 = list(np.concatenate([[0], np.cumsum(widths)[:-1]]))
    if fault == 'stream col0 off by one':
        col0[1] += 1
    which = -np.ones(d, dtype=np.int64)
    for k, w in enumerate(widths):
        which[np.arange(d)[(np.arange(d) >= col0[k]) & (np.arange(d) < col0[k] + w)]] = k
    # the (frame, column) every element is scored at: the kernel's running walk
    tt, cc = np.divmod(np.arange(t * d), d)
    if fault == 'column walk not wrapped at D >= 256':
        for lo in range(0, t * d, R.MSE_CHUNK):
            for tid in range(256):
                e = lo + tid
                ft, fc = divmod(e, d)
                while e < min(lo + R.MSE_CHUNK, t * d):
                    tt[e], cc[e] = ft, fc % d                     # the column wraps but the frame is not advanced with it
                    ft, fc = ft + 256 // d, fc + 256 % d
                    e += 256
    term = np.zeros((b, t * d), dtype=F32)
    grad = np.zeros((b, t * d), dtype=F32)
    prob = None
    with np.errstate(all='ignore'):
        inv_nb = (F32(grad_scale) / n.astype(F32)).astype(F32)
        for k, (y, kind) in enumerate(zip(targets, kinds)):
            sel = np.nonzero(which[cc] == k)[0]
            if not sel.size:
                continue
            j = np.minimum(cc[sel] - col0[k], widths[k] - 1)
            yk = np.asarray(y, dtype=F32)[:, np.minimum(tt[sel], t - 1), j]
            xs = x.reshape(b, -1)[:, sel]
            colw = F32(F32(1.0) / F32(F32(F32(b) * F32(widths[k])) * F32(len(targets))))
            if kind == 'mse':
                diff = (xs - yk).astype(F32)
                l, dl = (diff * diff).astype(F32), (F32(2.0) * diff).astype(F32)
            else:
                p = (F32(1.0) / (F32(1.0) + np.exp(-xs).astype(F32)).astype(F32)).astype(F32)
                l, dl = _emu_bce_elem(p, yk)
                dl = (dl * ((F32(1.0) - p).astype(F32) * p).astype(F32)).astype(F32)
                prob = np.zeros((b, t * widths[k]), dtype=F32)
                prob[:, tt[sel] * widths[k] + j] = p
                prob = prob.reshape(b, t, widths[k])
            m = (tt[sel][None, :] < n[:, None]).astype(F32)
            term[:, sel] = ((l * m).astype(F32) * colw).astype(F32)
            grad[:, sel] = ((dl * m).astype(F32) * (inv_nb * colw).astype(F32)[:, None]).astype(F32)
        loss = _emu_reduce(term, n, False, 1.0)
    return loss, grad.reshape(b, t, d), prob


def emu_normalise(x, p0, p1, kind, fused=False):
    x, a, b = np.asarray(x, dtype=F32), np.asarray(p0, dtype=F32), np.asarray(p1, dtype=F32)
    with np.errstate(all='ignore'):
        if kind == R.NORM_MVN:
            return ((x - a).astype(F32) / (b + F32(1e-8)).astype(F32)).astype(F32)
        if kind == R.DENORM_MVN:
            return (x.astype(F64) * b + a).astype(F32) if fused else ((x * b).astype(F32) + a).astype(F32)
        scale = (b - a).astype(F32)
        scale = np.where(np.abs(scale) <= F32(1e-8), F32(1.0), scale)
        if kind == R.NORM_MINMAX:
            return ((x - a).astype(F32) / scale).astype(F32)
        return (x.astype(F64) * scale + a).astype(F32) if fused else ((x * scale).astype(F32) + a).astype(F32)


def emu_ema(shadow, param, decay, fused=False):
    s, p = np.asarray(shadow, dtype=F32), np.asarray(param, dtype=F32)
    w = F32(F32(1.0) - F32(decay))
    diff = (s - p).astype(F32)
    return (s.astype(F64) - F64(w) * diff).astype(F32) if fused else (s - (w * diff).astype(F32)).astype(F32)


def _fma(a, b, c):
    return (np.asarray(a, dtype=F64) * np.asarray(b, dtype=F64) + np.asarray(c, dtype=F64)).astype(F32)


def emu_adam(p, g, m, v, ss, bc, betas, eps, wd, gs):
    """mg_adam_update in float32 (contraction off, the three explicit fmas)."""
    b1, b2 = F32(betas[0]), F32(betas[1])
    g = (g * F32(gs)).astype(F32)
    if F32(wd) != 0:
        g = _fma(F32(wd), p, g)
    m = _fma((g - m).astype(F32), F32(1.0) - b1, m)
    v = _fma(((F32(1.0) - b2) * g).astype(F32), g, (v * b2).astype(F32))
    den = ((np.sqrt(v).astype(F32) / F32(bc)).astype(F32) + F32(eps)).astype(F32)
    p = (p - (F32(ss) * (m / den).astype(F32)).astype(F32)).astype(F32)
    return p, m, v


def emu_metric(kind, target, pred, voiced, seq_len, col0, width, fault=None):
    tg = np.asarray(target, dtype=F32)
    b, t, d = tg.shape
    live = np.ones((b, t), dtype=bool)
    if seq_len is not None and fault != 'padded frame counted in a metric':
        live = np.arange(t)[None, :] < np.asarray(seq_len)[:, None]
    acc = np.zeros((b, t), dtype=F32)
    with np.errstate(all='ignore'):
        for j in range(col0, col0 + width):
            a = tg[:, :, j]
            if kind == 'mean':
                acc = (acc + a).astype(F32)
                continue
            q = np.asarray(pred, dtype=F32)[:, :, j]
            diff = (np.exp(a).astype(F32) - np.exp(q).astype(F32)).astype(F32) if kind == 'sqdiff_voiced_exp' else (a - q).astype(F32)
            acc = (acc + (np.abs(diff) if kind == 'absdiff' else (diff * diff).astype(F32))).astype(F32)
        if kind == 'root_sq':
            acc = np.sqrt(acc).astype(F32)
    if kind.startswith('sqdiff_voiced'):
        vf = np.asarray(voiced, dtype=F32).reshape(b, t)
        count = float(vf[live].astype(F64).sum())
        acc = (acc * vf).astype(F32)
    elif (seq_len is not None and fault != 'width counted in place of frames') or kind == 'root_sq':
        count = float(live.sum())
    else:
        count = float(live.sum() * width)
    return float(acc[live].astype(F64).sum()), count


def emu_upsample_index(dur, t_cap, fault=None):
    """upsample_index_kernel: the inclusive scan of the clamped durations, then 'first p with cum[p] > t' per frame."""
    d = np.maximum(np.asarray(dur, dtype=np.int64), 0)
    cum = np.cumsum(d, axis=1)
    idx = -np.ones((d.shape[0], t_cap), dtype=np.int64)
    for b in range(d.shape[0]):
        edges = cum[b].copy()
        if fault == 'one phone one frame short':
            p0 = int(np.nonzero(d[b] > 0)[0][0]) if np.any(d[b] > 0) else None
            if p0 is not None and p0 + 1 < d.shape[1]:
                edges[p0] -= 1
        live = np.arange(t_cap) < cum[b, -1]
        idx[b, live] = np.searchsorted(edges, np.arange(t_cap)[live], side='right')
    return idx


def emu_gather_rows_bf16(src, rows, ld, fault=None):
    """gather_rows_bf16_kernel chunk by chunk, into a buffer pre-filled with 0xffff."""
    src = np.asarray(src, dtype=F32)
    f = src.shape[1]
    flat = np.concatenate([src.reshape(-1), np.full(8, 7.0, dtype=F32)])
    out = np.full((len(rows), ld), 0xffff, dtype=np.uint16)
    for m, r in enumerate(rows):
        if r < 0 and fault == '-1 row read as row 0':
            r = 0
        for k in range(0, ld, 8):
            v = np.zeros(8, dtype=F32)
            partial = k < f < k + 8
            if partial and fault == 'last partial bf16 chunk unwritten':
                continue
            if r >= 0:
                for j in range(8):
                    if k + j < f or (partial and fault == 'last partial bf16 chunk unzeroed'):
                        v[j] = flat[r * f + k + j]
            out[m, k:k + 8] = R.bf16_bits(v)
    return out


# ------------------------------------------------------------------------------------------ the emulations against the bounds
def _check_masked(name, ref, loss, grad, record=True):
    """-> the names of the checks that fail."""
    failed = []
    if not _within(loss, ref['loss'], ref['loss_bound']):
        failed.append(name + ' loss')
    if not _within(grad, ref['grad'], ref['grad_bound']):
        failed.append(name + ' grad')
    if record and not failed:
        if not np.isnan(ref['loss']):
            _ratio(name + ' loss', abs(float(loss) - ref['loss']), ref['loss_bound'])
        _ratio(name + ' grad', _err(grad, ref['grad']), ref['grad_bound'])
    return failed


@pytest.mark.parametrize('kind', ['mse', 'bce'])
@pytest.mark.parametrize('shape', R.MASKED_SHAPES)
def test_emulated_masked_loss_is_within_its_bounds(shape, kind):
    t, d = shape
    pred, target, seq_len = R.masked_case(t, d, kind)
    forms = (True, False) if (t * d) % 4 == 0 else (False,)
    for vec4 in forms:
        for sl, gs in ((seq_len, 1.0), (seq_len, 0.25), (None, 1.0)):
            ref = R.masked_loss(pred, target, sl, gs, kind)
            loss, grad = emu_masked_loss(pred, target, sl, kind, gs, vec4)
            assert _check_masked('masked_%s' % kind, ref, loss, grad) == []


@pytest.mark.parametrize('kind', ['mse', 'bce'])
def test_emulated_masked_loss_on_empty_utterances(kind):
    pred, target, seq_len = R.masked_nan_case(kind)
    ref = R.masked_loss(pred, target, seq_len, kind=kind)
    loss, grad = emu_masked_loss(pred, target, seq_len, kind, vec4=False)
    assert np.isnan(loss) and np.isnan(ref['loss'])
    assert np.all(np.isnan(grad[:2])) and np.all(ref['nan_rows'] == [True, True, False])
    assert _check_masked('masked_%s' % kind, ref, loss, grad) == []


def masked_finish_case():
    """B = 257 (one utterance more than the finish has threads), T = 2, D = 1, lengths 1, 2, 1, ..."""
    rng = np.random.RandomState(20261027)
    return (rng.standard_normal((257, 2, 1)).astype(F32), rng.standard_normal((257, 2, 1)).astype(F32),
            (1 + np.arange(257) % 2).astype(np.int64))


def test_emulated_masked_loss_beyond_256_utterances():
    pred, target, seq_len = masked_finish_case()
    ref = R.masked_loss(pred, target, seq_len)
    assert _check_masked('masked_mse', ref, *emu_masked_loss(pred, target, seq_len, 'mse', vec4=False)) == []


@pytest.mark.parametrize('name', [c[0] for c in R.STREAM_CASES])
def test_emulated_stream_loss_is_within_its_bounds(name):
    pred, targets, kinds, seq_len = R.stream_case(name)
    for gs in (1.0, 0.25):
        ref = R.stream_loss(pred, targets, kinds, seq_len, gs)
        loss, grad, prob = emu_stream_loss(pred, targets, kinds, seq_len, gs)
        assert _check_masked('stream_loss', ref, loss, grad) == []
        if ref['prob'] is not None:
            assert _within(prob, ref['prob'], ref['prob_bound'])
            _ratio('stream_loss prob', _err(prob, ref['prob']), ref['prob_bound'])


@pytest.mark.parametrize('kind', [R.NORM_MVN, R.DENORM_MVN, R.NORM_MINMAX, R.DENORM_MINMAX])
@pytest.mark.parametrize('shape', R.NORMALISE_SHAPES)
def test_emulated_normalise_is_within_its_bound(shape, kind):
    x, p0, p1 = R.normalise_case(shape[0], shape[1], kind)
    want, bound = R.normalise(x, p0, p1, kind)
    for fused in (False, True):
        got = emu_normalise(x, p0, p1, kind, fused)
        assert _within(got, want, bound)
        _ratio('normalise kind %d' % kind, _err(got, want), bound)


@pytest.mark.parametrize('d', [3, 64, 70])
def test_emulated_pad_normalise_is_within_its_bound(d):
    packed, offsets, mvn, minmax = R.pad_normalise_case(d)
    for kind, (p0, p1) in ((R.NORM_MVN, mvn), (R.NORM_MINMAX, minmax)):
        raw, want, bound = R.pad_normalise(packed, offsets, 6, p0, p1, kind)
        got = emu_normalise(raw, p0, p1, kind)
        got[raw.shape[0] - 4, :] = 0.0                       # utterance 0 has no frame
        live = bound > 0
        assert _within(got[live], want[live], bound[live])
        _ratio('pad_normalise kind %d' % kind, _err(got[live], want[live]), bound[live])
    assert np.all(raw[0] == 0) and np.all(raw[1, 1:] == 0) and np.array_equal(raw[3], packed[offsets[3]:offsets[3] + 6])


@pytest.mark.parametrize('decay', [0.0, 0.999, 1.0])
@pytest.mark.parametrize('n', R.ADAM_SIZES)
def test_emulated_ema_is_within_its_bound(n, decay):
    rng = np.random.RandomState(n)
    s, p = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    want, bound = R.ema_update(s, p, decay)
    for fused in (False, True):
        got = emu_ema(s, p, decay, fused)
        assert _within(got, want, bound)
        _ratio('ema_update', _err(got, want), bound)


@pytest.mark.parametrize('grad_scale', [1.0, 0.5])
@pytest.mark.parametrize('weight_decay', [0.0, 1e-2])
@pytest.mark.parametrize('n', R.ADAM_SIZES)
def test_emulated_adam_is_within_its_bound(n, weight_decay, grad_scale):
    p, grads = R.adam_case(n)
    m, v = np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
    for step, g in enumerate(grads, 1):
        ss, bc = R.adam_scalars(R.ADAM_LR, R.ADAM_BETAS, step)
        want = R.adam_step(p, g, m, v, ss, bc, R.ADAM_BETAS, R.ADAM_EPS, weight_decay, grad_scale)      # from the emulation's own state
        p, m, v = emu_adam(p, g, m, v, ss, bc, R.ADAM_BETAS, R.ADAM_EPS, weight_decay, grad_scale)
        for name, got, w, bnd in (('p', p, want[0], want[3]), ('m', m, want[1], want[4]), ('v', v, want[2], want[5])):
            assert _within(got, w, bnd), name
            _ratio('adam_step ' + name, _err(got, w), bnd)
    zero = slice(n // 3, n // 3 + n // 8 + 1)
    if weight_decay == 0.0:
        assert np.all(m[zero] == 0) and np.all(v[zero] == 0)     # the stretch where denom = eps


@pytest.mark.parametrize('kind', R.METRIC_KINDS)
@pytest.mark.parametrize('shape', R.METRIC_SHAPES)
def test_emulated_metric_is_within_its_bound(shape, kind):
    b, t, d, col0, width = shape
    target, pred, voiced, seq_len = R.metric_case(shape)
    for sl in (seq_len, None):
        total, count, bound = R.metric_sums(kind, target, pred, voiced, sl, col0, width)
        got, got_count = emu_metric(kind, target, pred, voiced, sl, col0, width)
        assert got_count == count
        assert abs(got - total) <= bound
        _ratio('metric %s' % kind, abs(got - total), bound)


# =================================================================================================== 3. fault injection
def _caught(fault, checks):
    assert checks, 'fault %r is caught by no check' % fault
    CAUGHT.setdefault(fault, []).extend(c for c in checks if c not in CAUGHT.get(fault, []))


def _masked_failures(fault, cases):
    failed = []
    for (pred, target, seq_len, kind, vec4) in cases:
        ref = R.masked_loss(pred, target, seq_len, kind=kind)
        with np.errstate(all='ignore'):
            loss, grad = emu_masked_loss(pred, target, seq_len, kind, vec4=vec4, fault=fault)
        failed += _check_masked('masked_%s' % kind, ref, loss, grad, record=False)
    return sorted(set(failed))


def test_faults_of_the_masked_losses_are_caught():
    mse = R.masked_case(5000, 4, 'mse') + ('mse', True)
    mse_d1 = R.masked_case(8192, 1, 'mse') + ('mse', True)
    bce = R.masked_case(2049, 4, 'bce') + ('bce', True)
    for fault in ('mask off by one frame', 'one chunk partial dropped', 'n_b not clamped to T', 'coef without D'):
        _caught(fault, _masked_failures(fault, [mse]))
    # the edge inside a 16-byte vector needs D = 1 and a length that is no multiple of 4: with D = 4 the fault is invisible
    assert _masked_failures('mask edge per 4-vector', [mse]) == []
    _caught('mask edge per 4-vector', _masked_failures('mask edge per 4-vector', [mse_d1]))
    _caught('BCE gradient clamp removed', _masked_failures('BCE gradient clamp removed', [bce]))
    _caught('utterance 256 dropped by the finish',
            _masked_failures('utterance 256 dropped by the finish', [masked_finish_case() + ('mse', False)]))
    # one length above T is what shows a missing clamp: without it the fault is invisible
    pred, target, seq_len, kind, vec4 = mse
    assert _masked_failures('n_b not clamped to T', [(pred, target, np.minimum(seq_len, 5000), kind, vec4)]) == []


def test_faults_of_the_stream_loss_are_caught():
    for fault, name in (('stream col0 off by one', 'd5'), ('column walk not wrapped at D >= 256', 'd257'),
                        ('column walk not wrapped at D >= 256', 'd300')):
        pred, targets, kinds, seq_len = R.stream_case(name)
        ref = R.stream_loss(pred, targets, kinds, seq_len)
        with np.errstate(all='ignore'):
            loss, grad, _ = emu_stream_loss(pred, targets, kinds, seq_len, fault=fault)
        _caught(fault, [c + ' (%s)' % name for c in _check_masked('stream_loss', ref, loss, grad, record=False)])
    # at D = 256 the column never moves (256 % D = 0, a whole frame per trip): the fault is invisible there, D > 256 is what shows it
    pred, targets, kinds, seq_len = R.stream_case('d256')
    loss, grad, _ = emu_stream_loss(pred, targets, kinds, seq_len, fault='column walk not wrapped at D >= 256')
    assert _check_masked('stream_loss', R.stream_loss(pred, targets, kinds, seq_len), loss, grad, record=False) == []


def test_faults_of_the_row_movers_are_caught():
    rng = np.random.RandomState(5)
    rows = np.array([2, -1, 0, 4, -1], dtype=np.int64)
    for f, ld in ((12, 16), (7, 8), (20, 40)):
        src = R.fill_specials(rng.standard_normal((5, f)), rng)
        src[0, 0] = 1.5                                             # row 0 is no zero row
        want = R.gather_rows_bf16(src, rows, ld)
        assert R.bits_equal_bf16(emu_gather_rows_bf16(src, rows, ld), want)
        for fault in ('last partial bf16 chunk unwritten', 'last partial bf16 chunk unzeroed', '-1 row read as row 0'):
            assert not R.bits_equal_bf16(emu_gather_rows_bf16(src, rows, ld, fault), want)
            _caught(fault, ['gather_rows bf16 bits (F=%d)' % f])
    # F = 8: no partial chunk - the two chunk faults are invisible there
    src = rng.standard_normal((5, 8)).astype(F32)
    assert R.bits_equal_bf16(emu_gather_rows_bf16(src, rows, 8, 'last partial bf16 chunk unzeroed'), R.gather_rows_bf16(src, rows, 8))


def test_faults_of_the_index_maps_are_caught():
    dur = np.array([[0, 3, 0, 2, 4, 0], [1, 1, 1, 1, 1, 1]], dtype=np.int64)
    t_cap = 9
    want = R.upsample_index(dur, t_cap)
    assert np.array_equal(emu_upsample_index(dur, t_cap), want)
    bad = emu_upsample_index(dur, t_cap, 'one phone one frame short')
    assert not np.array_equal(bad, want)
    checks = ['upsample_index bits']
    # the same fault in the backward sum: one frame's gradient lands in the next phone - the exact check and the bound both fail
    g = np.random.RandomState(6).standard_normal((2, t_cap, 3)).astype(F32)
    ref = R.upsample_backward(g, dur, 6)
    got = np.zeros_like(ref['exact'])
    for b in range(2):
        for t in range(t_cap):
            if bad[b, t] >= 0:
                got[b, bad[b, t]] = (got[b, bad[b, t]] + g[b, t]).astype(F32)
    assert not R.bits_equal_f32(got, ref['exact'])
    assert not np.all(np.abs(got.astype(F64) - ref['sum']) <= ref['bound'])
    checks += ['upsample_backward bits', 'upsample_backward bound']
    _caught('one phone one frame short', checks)


def test_faults_of_the_metrics_are_caught():
    shape = R.METRIC_SHAPES[1]
    b, t, d, col0, width = shape
    target, pred, voiced, seq_len = R.metric_case(shape)
    for fault, field in (('padded frame counted in a metric', 'sum and count'), ('width counted in place of frames', 'count')):
        failed = []
        for kind in R.METRIC_KINDS:
            total, count, bound = R.metric_sums(kind, target, pred, voiced, seq_len, col0, width)
            got, got_count = emu_metric(kind, target, pred, voiced, seq_len, col0, width, fault)
            if got_count != count or abs(got - total) > bound:
                failed.append('metric %s %s' % (kind, field))
        _caught(fault, failed)


def test_a_wrong_order_fails_the_exact_check_alone_and_a_wrong_term_fails_both():
    rng = np.random.RandomState(7)
    g = rng.standard_normal((6, 700, 5)).astype(F32)
    seq_len = np.array([0, 700, 900, -3, 256, 300], dtype=np.int64)
    ref = R.pad_rows_colsum(g, seq_len)
    pad = np.arange(700)[None, :, None] >= np.clip(seq_len, 0, 700)[:, None, None]
    other_order = np.where(pad, g, F32(0)).reshape(-1, 5).sum(axis=0, dtype=F32)               # numpy's pairwise order
    assert not R.bits_equal_f32(other_order, ref['exact'])
    assert np.all(np.abs(other_order.astype(F64) - ref['sum']) <= ref['bound'])
    assert np.all(np.abs(ref['exact'].astype(F64) - ref['sum']) <= ref['bound'])
    _ratio('pad_rows_colsum sum', np.abs(ref['exact'].astype(F64) - ref['sum']), ref['bound'])
    pad_wrong = np.arange(700)[None, :, None] >= (np.clip(seq_len, 0, 700) + 1)[:, None, None]  # one padded frame missed per utterance
    wrong_term = np.where(pad_wrong, g, F32(0)).reshape(-1, 5).sum(axis=0, dtype=F32)
    assert not R.bits_equal_f32(wrong_term, ref['exact'])
    assert not np.all(np.abs(wrong_term.astype(F64) - ref['sum']) <= ref['bound'])


def test_bf16_rounding_on_the_bit_pattern():
    v = R.special_values()
    bits = R.bf16_bits(v)
    assert list(bits[:12]) == [0x0000, 0x8000, 0x7f80, 0xff80, 0x3f80, 0x3f82, 0xbf80, 0xbf82, 0x3f80, 0x3f81, 0x7f80, 0xff80]
    assert R.bf16_is_nan(bits[12]) and not np.any(R.bf16_is_nan(bits[:12]))
    x = np.random.RandomState(8).standard_normal(4096).astype(F32)
    back = R.bf16_to_f32(R.bf16_bits(x)).astype(F64)
    assert np.all(np.abs(back - x) <= 2.0 ** -8 * np.abs(x))                                    # half an ulp of 8 significant bits
    assert R.bits_equal_f32(R.cast_bf16_f32(R.cast_pad_bf16(x.reshape(64, 64), 72), 64), back.astype(F32).reshape(64, 64))


# ------------------------------------------------------------------------------------------------------------- the two tables
def test_zz_every_fault_is_caught_and_no_emulation_crowds_its_bound():
    """Runs last in this file (pytest keeps file order): prints the fault table and the worst emulation ratio per check."""
    if len(CAUGHT) < len(FAULTS):                            # selected alone: run the fault tests here
        for fn in (test_faults_of_the_masked_losses_are_caught, test_faults_of_the_stream_loss_are_caught,
                   test_faults_of_the_row_movers_are_caught, test_faults_of_the_index_maps_are_caught, test_faults_of_the_metrics_are_caught):
            fn()
    print('\nfault -> checks that caught it')
    for fault in FAULTS:
        print('  %-42s %s' % (fault, ', '.join(CAUGHT.get(fault, [])) or 'NOT CAUGHT'))
    print('check -> worst emulation error / bound')
    for check in sorted(RATIOS):
        print('  %-28s %.3f (ceiling %.1f)' % (check, RATIOS[check], R.ratio_ceiling(check)))
    assert [f for f in FAULTS if not CAUGHT.get(f)] == []
    # every reduction at or below half its bound, every element-wise check within it (datapath_ref.ratio_ceiling says why they differ)
    assert [c for c in RATIOS if RATIOS[c] > R.ratio_ceiling(c)] == []
