"""The data-path kernels (csrc/upsample.hip, loss_norm.hip, metrics.hip, the elementwise half of optim.hip) against
tests/datapath_ref.py at the shapes where their branches change: the exact family bit for bit, the bounded family element by element
within a derived float32 bound.  tests/test_datapath_ref_host.py shows on the CPU that the bounds admit a correct kernel and refuse a
broken one; DESIGN.md 4.23 has the case grid and the measured ratios.  Every check prints its worst error / bound."""
import functools

import numpy as np
import pytest
import torch

import datapath_ref as R
from morgana_amd import _lib, metrics, ops
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32 = np.float32
F64 = np.float64
RATIOS = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _off4(a):
    """The float32 array on the device as a contiguous view that starts 4 bytes into its (16-byte aligned) storage."""
    a = np.ascontiguousarray(a, dtype=F32)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _np(t):
    return t.detach().cpu().numpy()


def _bits16(t):
    return _np(t.view(torch.int16)).view(np.uint16)


def _report(check, got, want, bound):
    """Element-wise |got - want| <= bound (NaN exactly where wanted); prints and records the worst ratio."""
    got, want, bound = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64), np.asarray(bound, dtype=F64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), '%s: NaN pattern differs' % check
    with np.errstate(all='ignore'):
        err = np.where(np.isnan(want), 0.0, np.abs(got - want))
        ratio = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    RATIOS[check] = max(RATIOS.get(check, 0.0), worst)
    print('%-34s worst err / bound %.3f over %d elements' % (check, worst, ratio.size))
    assert worst <= R.ratio_ceiling(check), '%s: err / bound %.3f above its ceiling %.1f' % (check, worst, R.ratio_ceiling(check))


def _no_launch(call, match=None):
    calls = []
    _lib.CALL_LOG = calls
    try:
        with pytest.raises((ValueError, TypeError, _lib.MorganaHipError), match=match):
            call()
    finally:
        _lib.CALL_LOG = None
    assert calls == [], calls


# ===================================================================================================================== index maps
def _durations(p, seed=1):
    """B = 4: random 0..3 with leading, interior and trailing zeros; an all-zero utterance; one phone that owns every frame; random."""
    rng = np.random.RandomState(seed + p)
    dur = rng.randint(0, 4, size=(4, p)).astype(np.int64)
    if p >= 8:
        dur[0, :3] = 0
        dur[0, p // 2:p // 2 + 2] = 0
        dur[0, -3:] = 0
    dur[1] = 0
    dur[2] = 0
    dur[2, p // 2] = 11
    return dur


def _check_index(dur, t_cap):
    b, p = dur.shape
    d = _dev(dur)
    want = R.upsample_index(dur, t_cap)
    idx64, rows = ops.upsample_index(d, t_cap, want_idx64=True)
    assert np.array_equal(_np(idx64), want)
    want_rows, want_mapped, want_seg = R.upsample_index_maps(dur, t_cap)
    assert np.array_equal(_np(rows), want_rows)
    if t_cap > 0:
        rows2, mapped, seg = ops.upsample_index_maps(d, t_cap)
        assert np.array_equal(_np(rows2), want_rows) and np.array_equal(_np(mapped), want_mapped)
        assert np.array_equal(_np(seg), want_seg)
    n_frames, tmax = ops.upsample_lengths(d)
    want_n, want_tmax = R.upsample_lengths(dur)
    assert np.array_equal(_np(n_frames), want_n) and int(tmax.item()) == int(want_tmax)


@pytest.mark.parametrize('p', [1, 255, 256, 257, 513])
def test_index_maps_at_the_scan_edges(p):
    """P = 255 / 256 / 257: the scan's threads own 1, 1, 2 phones (trailing threads none at 257 and 513); t_cap below the total (inside
    a phone, whole phones dropped: seg = (0, 0)), equal, above (-1 fill, rows_mapped = pad_row) and 0."""
    dur = _durations(p)
    total = int(R.upsample_lengths(dur)[1])
    for t_cap in (total, max(total // 2 - 1, 1), total - 1 if total > 1 else 1, total + 5, 0):
        _check_index(dur, t_cap)


def test_index_maps_at_the_phone_limit():
    """P = MG_MAX_PHONES = 12 288: 50 KB of LDS, 48 phones per scan thread."""
    rng = np.random.RandomState(2)
    dur = rng.randint(0, 3, size=(2, R.MAX_PHONES)).astype(np.int64)
    dur[1, -1] = 4
    total = int(R.upsample_lengths(dur)[1])
    _check_index(dur, total)
    g = rng.standard_normal((2, 64, 3)).astype(F32)                    # the backward's scan at the limit; T clips almost every phone
    ref = R.upsample_backward(g, dur, R.MAX_PHONES)
    assert R.bits_equal_f32(_np(ops.upsample_backward(_dev(g), _dev(dur), R.MAX_PHONES)), ref['exact'])


def test_one_phone_too_many_is_refused_without_a_launch():
    dur = _dev(np.ones((1, R.MAX_PHONES + 1), dtype=np.int64))
    g = _dev(np.zeros((1, 4, 2), dtype=F32))
    _no_launch(lambda: ops.upsample_index(dur, 16), 'phones')
    _no_launch(lambda: ops.upsample_index_maps(dur, 16), 'phones')
    _no_launch(lambda: ops.segment_index(dur, 16, 2), 'phones')
    _no_launch(lambda: ops.upsample_backward(g, dur, R.MAX_PHONES + 1), 'phones')


def test_negative_durations_own_no_frame_in_any_of_the_three_outputs():
    dur = np.array([[3, -2, 0, 4, -7], [-1, -1, -1, -1, -1], [2, 2, -5, 2, 2]], dtype=np.int64)
    d = _dev(dur)
    n_frames, tmax = ops.upsample_lengths(d)
    idx64, _ = ops.upsample_index(d, 12, want_idx64=True)
    frames_in_map = (_np(idx64) >= 0).sum(axis=1)
    assert np.array_equal(_np(n_frames), frames_in_map) and int(tmax.item()) == int(frames_in_map.max())
    assert frames_in_map.tolist() == [7, 0, 8]
    _check_index(dur, 8)


@pytest.mark.parametrize('s', [1, 255, 256, 257, 513])
def test_segment_index(s):
    rng = np.random.RandomState(3 + s)
    lens = rng.randint(0, 4, size=(3, s)).astype(np.int64)              # zero-length segments among them
    lens[1] = 0
    lens[2, s // 2] = 6
    total = int(lens.sum(axis=1).max())
    longest = int(lens.max())
    d = _dev(lens)
    for t in (total, max(total // 2, 1)):                               # T below the sum: ends = -1 past T, the split clipped
        for max_len in (longest, max(longest - 2, 1), longest + 3):
            want_split, want_ends = R.segment_index(lens, t, max_len)
            split, ends = ops.segment_index(d, t, max_len)
            assert np.array_equal(_np(split), want_split) and np.array_equal(_np(ends), want_ends)
        split, ends = ops.segment_index(d, t, longest, want_ends=False)
        assert ends is None and np.array_equal(_np(split), R.segment_index(lens, t, longest)[0])
        split, ends = ops.segment_index(d, t, want_split=False)
        assert split is None and np.array_equal(_np(ends), R.segment_index(lens, t, 1)[1])


@pytest.mark.parametrize('b', [1, 256, 257, 600])
def test_frame_layout(b):
    """B = 256 / 257 / 600: one, two and three utterances per scan thread; lengths 0, negative and above T; a host total equal to,
    below and above what the device lengths add up to, and 0."""
    rng = np.random.RandomState(4 + b)
    t = 7
    seq_len = rng.randint(-2, 11, size=b).astype(np.int64)
    if b == 1:
        seq_len[0] = 3
    dev_sum = int(np.clip(seq_len, 0, t).sum())
    for total in (dev_sum, max(dev_sum - 2, 0), min(dev_sum + 3, b * t), 0):
        want = R.frame_layout(seq_len, t, total)
        got = ops.frame_layout(_dev(seq_len), t, total)
        for g, w, name in zip(got, want, ('offsets', 'rows', 'inverse')):
            assert np.array_equal(_np(g), w), (name, total)


@pytest.mark.parametrize('dtype', [torch.uint8, torch.bool, torch.int8, torch.float32, torch.int32, torch.int64, torch.float64])
def test_sequence_mask(dtype):
    seq_len = np.array([0, 3, 9, 12], dtype=np.int64)
    np_dtype = {torch.uint8: np.uint8, torch.bool: np.bool_, torch.int8: np.int8, torch.float32: np.float32, torch.int32: np.int32,
                torch.int64: np.int64, torch.float64: np.float64}[dtype]
    for max_len in (0, 1, 9):
        got = ops.sequence_mask(_dev(seq_len), max_len, dtype)
        assert got.dtype == dtype and np.array_equal(_np(got), R.sequence_mask(seq_len, max_len, np_dtype))


# ===================================================================================================================== row movers
def _source(rows, f, seed, subnormals=False):
    rng = np.random.RandomState(seed + 17 * f)
    return R.fill_specials(rng.standard_normal((rows, f)), rng, subnormals)


def _row_ids(m, n_src, seed):
    rng = np.random.RandomState(seed)
    rows = rng.randint(0, n_src, size=m).astype(np.int32)
    rows[rng.uniform(size=m) < 0.3] = -1
    if m > 1:
        rows[1] = -1
    return rows


@pytest.mark.parametrize('f', [1, 3, 4, 68, 260])
def test_gather_rows_f32(f):
    """F % 4 == 0 on an aligned base: the 16-byte template (two trips of its lane loop at F = 260... 65 vectors); the same values 4 bytes
    off alignment: the scalar template; F = 1, 3: scalar by shape.  A float32 row is moved bit for bit, subnormals and NaN included."""
    src = _source(9, f, 5, subnormals=True)
    rows = _row_ids(5, 9, 6)
    want = R.gather_rows(src, rows)
    for s in (_dev(src), _off4(src)):
        assert R.bits_equal_f32(_np(ops.gather_rows(s, _dev(rows))), want)


@pytest.mark.parametrize('m', [1, 5, 32768 + 5])
def test_gather_rows_f32_grid_stride(m):
    """M = 32 773 rows over 8192 workgroups of 4 waves: five rows take a second trip of the grid-stride loop."""
    src = _source(9, 4, 7)
    rows = _row_ids(m, 9, 8)
    want = R.gather_rows(src, rows)
    for s in (_dev(src), _off4(src)):
        assert R.bits_equal_f32(_np(ops.gather_rows(s, _dev(rows))), want)


@pytest.mark.parametrize('f', [1, 4, 7, 8, 12, 20, 516])
def test_gather_rows_bf16(f):
    """F = 8: whole chunks only; 12, 20: a partial last chunk on the 16-byte path; 1, 7: F % 4 != 0, the scalar path; ld = pad8(F) + 16: two
    whole zero chunks; 516: ld / 8 > 64, the lane loop's second trip.  A source 4 bytes off alignment is copied by the wrapper."""
    src = _source(9, f, 9)
    rows = _row_ids(5, 9, 10)
    for ld in (None, ops.pad8(f) + 16):
        want = R.gather_rows_bf16(src, rows, ld)
        for s in (_dev(src), _off4(src)):
            got = ops.gather_rows(s, _dev(rows), out_bf16=True, ld=ld)
            assert R.bits_equal_bf16(_bits16(got), want), (f, ld)


@pytest.mark.parametrize('f,c', [(1, 1), (4, 1), (7, 1), (8, 8), (12, 2), (20, 4), (516, 3)])
def test_gather_concat(f, c):
    """(12, 2): one 8-element chunk holds source, extra and padding columns together."""
    src = _source(9, f, 11)
    rows = _row_ids(5, 9, 12)
    extra = _source(5, c, 13)
    got = ops.gather_concat(_dev(src), _dev(rows), _dev(extra))
    assert R.bits_equal_f32(_np(got), R.gather_concat(src, rows, extra))
    want = R.gather_concat_bf16(src, rows, extra)
    for s in (_dev(src), _off4(src)):
        assert R.bits_equal_bf16(_bits16(ops.gather_concat(s, _dev(rows), _dev(extra), out_bf16=True)), want)


@pytest.mark.parametrize('f', [1, 65, 130])
def test_scatter_rows(f):
    src = _source(6, f, 14, subnormals=True)
    rows = np.array([7, -1, 0, 9, 3, -1], dtype=np.int32)
    got = ops.scatter_rows(_dev(src), _dev(rows), 10)
    want = R.scatter_rows(src, rows, 10)
    assert R.bits_equal_f32(_np(got), want)
    assert np.all(_np(got)[[1, 2, 4, 5, 6, 8]].view(np.uint32) == 0)           # untouched rows are +0
    # scatter(gather(x)) restores the gathered rows
    x = _source(10, f, 15)
    gathered = ops.gather_rows(_dev(x), _dev(rows))
    back = ops.gather_rows(ops.scatter_rows(gathered, _dev(rows), 10), _dev(rows))
    assert R.bits_equal_f32(_np(back), _np(gathered))


def test_scatter_rows_grid_stride():
    m = 32768 + 5
    rng = np.random.RandomState(16)
    rows = rng.permutation(m + 3)[:m].astype(np.int32)
    rows[rng.uniform(size=m) < 0.1] = -1
    src = rng.standard_normal((m, 1)).astype(F32)
    assert R.bits_equal_f32(_np(ops.scatter_rows(_dev(src), _dev(rows), m + 3)), R.scatter_rows(src, rows, m + 3))


@pytest.mark.parametrize('cols', [1, 7, 8, 12, 609, 620])
def test_cast_pad_bf16(cols):
    """cols % 4 == 0 on an aligned base: eight columns per thread; 4 bytes off, or any other width: one element per thread.  Both must
    return the same bits for the same values."""
    x = _source(5, cols, 17)
    for ld in (None, ops.pad8(cols) + 8):
        for extra_rows in (0, 3):
            want = R.cast_pad_bf16(x, ld, extra_rows)
            got = [_bits16(ops.cast_pad_bf16(s, ld, extra_rows)) for s in (_dev(x), _off4(x))]
            assert R.bits_equal_bf16(got[0], want) and R.bits_equal_bf16(got[1], want), (cols, ld, extra_rows)
            keep = ~R.bf16_is_nan(want)
            assert np.array_equal(got[0][keep], got[1][keep])


@pytest.mark.parametrize('rows,cols', [(1, 32), (31, 1), (33, 65), (64, 64)])
def test_cast_transpose_and_cast_params_bf16(rows, cols):
    x = _source(rows, cols, 18)
    want_t = R.cast_transpose_bf16(x)
    assert R.bits_equal_bf16(_bits16(ops.cast_transpose_bf16(_dev(x))), want_t)
    plain, trans = ops.cast_params_bf16([_dev(x)], want_t=(0,))
    assert R.bits_equal_bf16(_bits16(plain[0]), R.cast_pad_bf16(x))
    assert R.bits_equal_bf16(_bits16(trans[0]), want_t)


def test_cast_params_bf16_sixteen_matrices_and_one_too_many():
    shapes = [(1, 32), (31, 1), (33, 65), (64, 64)] * 4
    xs = [_source(r, c, 19 + i) for i, (r, c) in enumerate(shapes)]
    plain, trans = ops.cast_params_bf16([_dev(x) for x in xs], want_t=tuple(range(16)))
    for x, pb, tb in zip(xs, plain, trans):
        assert R.bits_equal_bf16(_bits16(pb), R.cast_pad_bf16(x)) and R.bits_equal_bf16(_bits16(tb), R.cast_transpose_bf16(x))
    _no_launch(lambda: ops.cast_params_bf16([_dev(x) for x in xs] + [_dev(xs[0])]), 'at most')


def test_cast_bf16_f32_with_a_padded_leading_dimension():
    x = _source(5, 12, 20)
    bits = R.cast_pad_bf16(x, 24)
    table = ops.cast_pad_bf16(_dev(x), 24)
    got = _np(ops.cast_bf16_f32(table, 12))
    want = R.cast_bf16_f32(bits, 12)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def test_every_bf16_kernel_returns_the_same_bits_for_float32_subnormals():
    """What the device makes of a float32 subnormal is recorded, not asserted; all bf16-producing kernels must agree on it."""
    sub = R.subnormal_values()
    row8 = np.concatenate([sub, np.array([1.5, -2.5], dtype=F32)])[None, :]      # F = 8: the 16-byte paths
    row7 = row8[:, :7].copy()                                                     # F = 7: the scalar paths
    ident = _dev(np.array([0], dtype=np.int32))
    extra = _dev(np.ones((1, 1), dtype=F32))
    outs = {
        'gather_rows x8': _bits16(ops.gather_rows(_dev(row8), ident, out_bf16=True))[0, :6],
        'gather_rows scalar': _bits16(ops.gather_rows(_dev(row7), ident, out_bf16=True))[0, :6],
        'gather_concat x8': _bits16(ops.gather_concat(_dev(row8), ident, extra, out_bf16=True))[0, :6],
        'gather_concat scalar': _bits16(ops.gather_concat(_dev(row7), ident, extra, out_bf16=True))[0, :6],
        'cast_pad x8': _bits16(ops.cast_pad_bf16(_dev(row8)))[0, :6],
        'cast_pad scalar': _bits16(ops.cast_pad_bf16(_dev(row7)))[0, :6],
        'cast_transpose': _bits16(ops.cast_transpose_bf16(_dev(row8)))[:6, 0],
    }
    plain, trans = ops.cast_params_bf16([_dev(row8)], want_t=(0,))
    outs['cast_params'] = _bits16(plain[0])[0, :6]
    outs['cast_params transposed'] = _bits16(trans[0])[:6, 0]
    # the operand table of pad_normalise: mean 0 / std 1 (1 + 1e-8f is 1.0f) and mmin 0 / mmax 1 leave every value as it is - x - 0 and
    # x / 1 are exact - so the float the kernel rounds to bf16 is the subnormal itself (norm_out is asserted to hold it)
    one_frame = _dev(np.array([0, 1], dtype=np.int64))
    zeros, ones = _dev(np.zeros(8, dtype=F32)), _dev(np.ones(8, dtype=F32))
    for kind in (R.NORM_MVN, R.NORM_MINMAX):
        _, norm, table = ops.pad_normalise(_dev(row8), one_frame, 1, zeros, ones, kind, bf16_extra_rows=0)
        assert R.bits_equal_f32(_np(norm).reshape(1, 8), row8)
        outs['pad_normalise table kind %d' % kind] = _bits16(table)[0, :6]
    first = outs['gather_rows x8']
    print('float32 subnormals %s -> bf16 bits %s (IEEE round-to-nearest-even: %s)'
          % ([hex(v) for v in sub.view(np.uint32)], [hex(v) for v in first], [hex(v) for v in R.bf16_bits(sub)]))
    for name, bits in outs.items():
        assert np.array_equal(bits, first), name


def _bytes(n, seed):
    return np.random.RandomState(seed).randint(0, 256, size=n).astype(np.uint8)


def test_copy_many_byte_counts_alignments_and_guards():
    """0, 1, 15, 16, 17 and 196 613 bytes in one call (small descriptors beside a large one: blockIdx.x beyond a small one's extent must
    copy nothing); source, destination and both 4 bytes off alignment (the byte path); 64 guard bytes either side stay untouched."""
    counts = (0, 1, 15, 16, 17, 16 * 4096 * 3 + 5)
    guard = 64
    for src_off, dst_off in ((0, 0), (4, 0), (0, 4), (4, 4)):
        pairs, checks = [], []
        for i, n in enumerate(counts):
            data = _bytes(n, 21 + i)
            sbuf = torch.zeros(n + 32, dtype=torch.uint8, device=DEV)
            src = sbuf[src_off:src_off + n]
            src.copy_(torch.from_numpy(data))
            dbuf = torch.full((n + 2 * guard + 16,), 0xAB, dtype=torch.uint8, device=DEV)
            dst = dbuf[guard + dst_off:guard + dst_off + n]
            pairs.append((dst, src))
            checks.append((dbuf, guard + dst_off, data))
        ops.copy_many(pairs)
        for dbuf, at, data in checks:
            got = _np(dbuf)
            assert np.array_equal(got[at:at + data.size], data), (src_off, dst_off, data.size)
            assert np.all(got[:at] == 0xAB) and np.all(got[at + data.size:] == 0xAB), (src_off, dst_off, data.size)


def test_copy_many_dtypes_in_seventeen_pairs():
    """int64, bool, float32 and bfloat16 tensors, 17 pairs: two launches."""
    pairs, wants = [], []
    for i in range(17):
        dtype, elem = [(torch.int64, 8), (torch.bool, 1), (torch.float32, 4), (torch.bfloat16, 2)][i % 4]
        n = 3 + 5 * i
        data = _bytes(n * elem, 40 + i)
        if dtype == torch.bool:
            data &= 1
        src = torch.from_numpy(data).to(DEV).view(dtype)
        dst = torch.zeros(n, dtype=dtype, device=DEV)
        pairs.append((dst, src))
        wants.append(data)
    ops.copy_many(pairs)
    for (dst, _), data in zip(pairs, wants):
        assert np.array_equal(_np(dst.view(torch.uint8)), data)


# ================================================================================================================ fixed-order sums
@pytest.mark.parametrize('f', [1, 65, 130])
@pytest.mark.parametrize('p', [1, 64, 65, 130])
def test_upsample_backward(p, f):
    """P = 64: one phone per wave of the launch; 65, 130: waves take a second and third phone; F > 64: the lane loop's next trips; T below
    the total clips inside a phone and drops the phones behind it (exact zeros, as for zero-duration phones)."""
    rng = np.random.RandomState(22 + p + f)
    dur = rng.randint(0, 4, size=(2, p)).astype(np.int64)
    dur[0, 0] = 3
    total = int(dur.sum(axis=1).max())
    for t in (total, max(total - 2, 1), max(total // 2, 1)):
        g = rng.standard_normal((2, t, f)).astype(F32)
        ref = R.upsample_backward(g, dur, p)
        got = _np(ops.upsample_backward(_dev(g), _dev(dur), p))
        assert R.bits_equal_f32(got, ref['exact']), (p, f, t)
        _report('upsample_backward sum', got, ref['sum'], ref['bound'])
        cum = np.minimum(np.cumsum(np.maximum(dur, 0), axis=1), t)
        empty = np.diff(np.concatenate([np.zeros((2, 1), dtype=np.int64), cum], axis=1), axis=1) == 0
        assert np.all(got[empty].view(np.uint32) == 0)


@pytest.mark.parametrize('d', [1, 63, 64, 65, 200])
@pytest.mark.parametrize('t', [1, 255, 256, 257, 700])
def test_pad_rows_colsum(t, d):
    """B = 6: T = 700 gives 18 partials (stage 2's waves 0 and 1 add two each); lengths 0, T, above T, negative, on a chunk edge, inside a
    chunk.  The result goes into one row of a larger tensor, as functional.UnpackRowsFn has it; its neighbours stay as they were."""
    rng = np.random.RandomState(23 + t + d)
    g = rng.standard_normal((6, t, d)).astype(F32)
    seq_len = np.array([0, t, t + 9, -3, min(256, t), min(300, max(t - 1, 0))], dtype=np.int64)
    ref = R.pad_rows_colsum(g, seq_len)
    out = torch.full((3, d), 7.0, dtype=torch.float32, device=DEV)
    ops.pad_rows_colsum(_dev(g), _dev(seq_len), out[1])
    got = _np(out)
    assert R.bits_equal_f32(got[1], ref['exact']), (t, d)
    assert np.all(got[0] == 7.0) and np.all(got[2] == 7.0)
    _report('pad_rows_colsum sum', got[1], ref['sum'], ref['bound'])


def test_unchecked_arguments_are_refused_before_any_launch():
    g = _dev(np.zeros((2, 3, 4), dtype=F32))
    out = torch.zeros(4, dtype=torch.float32, device=DEV)
    accum = torch.zeros(2, dtype=torch.float64, device=DEV)
    _no_launch(lambda: ops.pad_rows_colsum(g, _dev(np.array([1, 2], dtype=np.int32)), out), 'seq_len')
    _no_launch(lambda: ops.pad_rows_colsum(g, _dev(np.array([1], dtype=np.int64)), out), 'seq_len')
    _no_launch(lambda: ops.pad_rows_colsum(g, _dev(np.array([1, 2], dtype=np.int64)), torch.zeros(3, dtype=torch.float32, device=DEV)), 'out')
    _no_launch(lambda: ops.pad_rows_colsum(g, _dev(np.array([1, 2], dtype=np.int64)), torch.zeros(4, dtype=torch.float32)))
    _no_launch(lambda: ops.metric_accumulate(ops.METRIC_MEAN, accum, g, seq_len=_dev(np.array([1, 2], dtype=np.int32))), 'seq_len')
    _no_launch(lambda: ops.metric_accumulate(ops.METRIC_MEAN, accum, g, seq_len=_dev(np.array([1], dtype=np.int64))), 'seq_len')
    _no_launch(lambda: ops.metric_accumulate(ops.METRIC_MEAN, torch.zeros(2, dtype=torch.float32, device=DEV), g), 'accum')
    _no_launch(lambda: ops.metric_accumulate(ops.METRIC_MEAN, torch.zeros(1, dtype=torch.float64, device=DEV), g), 'accum')


# =================================================================================================================== masked losses
@functools.lru_cache(maxsize=None)
def _masked_inputs(t, d, kind):
    return R.masked_case(t, d, kind)


def _bits32(x):
    return _np(x).view(np.uint32) if isinstance(x, torch.Tensor) else None


@pytest.mark.parametrize('aligned', [True, False], ids=['aligned', 'off4'])
@pytest.mark.parametrize('kind', ['mse', 'bce'])
@pytest.mark.parametrize('shape', R.MASKED_SHAPES, ids=lambda s: 'T%dxD%d' % s)
def test_masked_loss(shape, kind, aligned):
    """T D = 8192, 8196, 20000 on an aligned base: masked_mse_stage1<VEC4>; the same 4 bytes off, and T D = 3, 8191, 8193: the scalar form.
    8193 / 8196: a second chunk of 1 / 4 elements; 20000: three chunks.  The lengths: datapath_ref.masked_lengths."""
    t, d = shape
    pred, target, seq_len = _masked_inputs(t, d, kind)
    put = _dev if aligned else _off4
    p, y, sl = put(pred), put(target), _dev(seq_len)
    name = 'masked_%s' % kind
    for lengths, dev_lengths, gs in ((seq_len, sl, 1.0), (seq_len, sl, 0.25), (None, None, 1.0)):
        ref = R.masked_loss(pred, target, lengths, gs, kind)
        loss, grad = ops.masked_mse(p, y, dev_lengths, want_grad=True, grad_scale=gs, kind=kind)
        _report(name + ' loss', loss.item(), ref['loss'], ref['loss_bound'])
        _report(name + ' grad', _np(grad), ref['grad'], ref['grad_bound'])
        assert np.all(_np(grad)[~ref['mask']] == 0.0)
        loss2, none = ops.masked_mse(p, y, dev_lengths, want_grad=False, grad_scale=gs, kind=kind)
        assert none is None and np.array_equal(_bits32(loss2), _bits32(loss))               # the same loss bits without the gradient
        loss3, grad3 = ops.masked_mse(p, y, dev_lengths, want_grad=True, grad_scale=gs, kind=kind)
        assert np.array_equal(_bits32(loss3), _bits32(loss)) and np.array_equal(_bits32(grad3), _bits32(grad))   # and on a second call


@pytest.mark.parametrize('kind', ['mse', 'bce'])
def test_masked_loss_with_empty_utterances(kind):
    """Lengths (0, -2, 4): a NaN loss, NaN on every gradient element of utterances 0 and 1, utterance 2 within its bound."""
    pred, target, seq_len = R.masked_nan_case(kind)
    ref = R.masked_loss(pred, target, seq_len, kind=kind)
    loss, grad = ops.masked_mse(_dev(pred), _dev(target), _dev(seq_len), want_grad=True, kind=kind)
    assert np.isnan(loss.item()) and np.isnan(ref['loss'])
    got = _np(grad)
    assert np.all(np.isnan(got[:2]))
    _report('masked_%s grad' % kind, got, ref['grad'], ref['grad_bound'])


def test_masked_loss_beyond_256_utterances():
    """B = 257: utterance 256 is the second one of the finish's thread 0 (what the host fault 'utterance 256 dropped' needs)."""
    rng = np.random.RandomState(20261027)
    pred, target = rng.standard_normal((257, 2, 1)).astype(F32), rng.standard_normal((257, 2, 1)).astype(F32)
    seq_len = (1 + np.arange(257) % 2).astype(np.int64)
    ref = R.masked_loss(pred, target, seq_len)
    loss, grad = ops.masked_mse(_dev(pred), _dev(target), _dev(seq_len), want_grad=True)
    _report('masked_mse loss', loss.item(), ref['loss'], ref['loss_bound'])
    _report('masked_mse grad', _np(grad), ref['grad'], ref['grad_bound'])


def test_bce_special_probabilities():
    """p in {0, 1, 2^-149, 1 - 2^-24} against y in {0, 1, 0.3}: the log terms clamp at -100, the gradient's denominator at 1e-12."""
    p = np.repeat(R.BCE_SPECIAL_P, 3).reshape(1, 12, 1)
    y = np.tile(R.BCE_SPECIAL_Y, 4).reshape(1, 12, 1)
    ref = R.masked_loss(p, y, None, kind='bce')
    loss, grad = ops.masked_mse(_dev(p), _dev(y), None, want_grad=True, kind='bce')
    _report('masked_bce loss', loss.item(), ref['loss'], ref['loss_bound'])
    _report('masked_bce grad', _np(grad), ref['grad'], ref['grad_bound'])
    got = _np(grad).reshape(-1).astype(F64) * 12
    c = float(F32(1e-12))
    assert got[1] == pytest.approx(-1.0 / c, rel=1e-6) and got[3] == pytest.approx(1.0 / c, rel=1e-6)      # (p, y) = (0, 1), (1, 0)
    assert got[0] == 0.0 and got[4] == 0.0                                                                    # (0, 0), (1, 1)
    assert ref['loss'] * 12 >= 200.0 and np.isfinite(loss.item())       # (0, 1) and (1, 0) alone: two log terms clamped at -100


@pytest.mark.parametrize('name', [c[0] for c in R.STREAM_CASES])
def test_stream_loss(name):
    """D = 255 / 256 / 257 / 300: the column walk with 256 / D = 1, 1, 0, 0 and 256 % D = 1, 0, 256, 256 (D >= 256 wraps on every trip);
    d257_t40: two chunks, the second starting in mid-row; single streams; an empty utterance (NaN loss, the other gradients in bound)."""
    pred, targets, kinds, seq_len = R.stream_case(name)
    p, ys, sl = _dev(pred), [_dev(y) for y in targets], _dev(seq_len)
    want_prob = 'sigmoid_bce' in kinds
    for gs in (1.0, 0.25):
        ref = R.stream_loss(pred, targets, kinds, seq_len, gs)
        loss, grad, prob = ops.stream_loss(p, ys, kinds, sl, want_grad=True, want_prob=want_prob, grad_scale=gs)
        _report('stream_loss loss', loss.item(), ref['loss'], ref['loss_bound'])
        _report('stream_loss grad', _np(grad), ref['grad'], ref['grad_bound'])
        if want_prob:
            _report('stream_loss prob', _np(prob), ref['prob'], ref['prob_bound'])
        loss2, none, _ = ops.stream_loss(p, ys, kinds, sl, want_grad=False, grad_scale=gs)
        assert none is None and np.array_equal(_bits32(loss2), _bits32(loss))


@pytest.mark.parametrize('kind', [R.NORM_MVN, R.DENORM_MVN, R.NORM_MINMAX, R.DENORM_MINMAX])
@pytest.mark.parametrize('shape', R.NORMALISE_SHAPES, ids=lambda s: '%dx%d' % s)
def test_normalise(shape, kind):
    """(1, 5000): D above the grid stride of 1280, so the running column index wraps on every trip; (513, 600): four trips; with D >= 3
    column 1 has mmax == mmin and column 2 |mmax - mmin| = 5e-9: the scale = 1 branch."""
    assert (ops.NORM_MVN, ops.DENORM_MVN, ops.NORM_MINMAX, ops.DENORM_MINMAX) == (R.NORM_MVN, R.DENORM_MVN, R.NORM_MINMAX, R.DENORM_MINMAX)
    x, p0, p1 = R.normalise_case(shape[0], shape[1], kind)
    want, bound = R.normalise(x, p0, p1, kind)
    got = _np(ops.normalise(_dev(x), _dev(p0), _dev(p1), kind))
    _report('normalise kind %d' % kind, got, want, bound)


@pytest.mark.parametrize('d', [3, 64, 70])
def test_pad_normalise(d):
    """Utterances of 0, 1, T and T + 3 frames (clipped); both kinds; want_raw=False; the bf16 operand table with 0 and 3 extra rows: bit for
    bit the bf16 rounding of the float32 tensor the same launch stored, zero in padding columns, pad frames and extra rows; T = 0."""
    t = 6
    packed, offsets, mvn, minmax = R.pad_normalise_case(d, t)
    pk, off = _dev(packed), _dev(offsets)
    for kind, (p0, p1) in ((R.NORM_MVN, mvn), (R.NORM_MINMAX, minmax)):
        want_raw, want, bound = R.pad_normalise(packed, offsets, t, p0, p1, kind)
        raw, norm = ops.pad_normalise(pk, off, t, _dev(p0), _dev(p1), kind)
        assert R.bits_equal_f32(_np(raw), want_raw)
        _report('pad_normalise kind %d' % kind, _np(norm), want, bound)
        assert np.all(_np(norm)[bound == 0].view(np.uint32) == 0)
        none, norm2 = ops.pad_normalise(pk, off, t, _dev(p0), _dev(p1), kind, want_raw=False)
        assert none is None and np.array_equal(_bits32(norm2), _bits32(norm))
        for extra_rows in (0, 3):
            raw3, norm3, table = ops.pad_normalise(pk, off, t, _dev(p0), _dev(p1), kind, bf16_extra_rows=extra_rows)
            assert R.bits_equal_f32(_np(raw3), want_raw)
            _report('pad_normalise kind %d' % kind, _np(norm3), want, bound)
            ld = ops.pad_ld(d)
            assert tuple(table.shape) == (4 * t + extra_rows, ld)
            bits = _bits16(table)
            assert np.array_equal(bits, R.cast_pad_bf16(_np(norm3).reshape(4 * t, d), ld, extra_rows))      # the very float it stored
            assert np.all(bits[:, d:] == 0) and np.all(bits[4 * t:] == 0)
            pad_frames = (bound == 0).all(axis=2).reshape(-1)
            assert np.all(bits[:4 * t][pad_frames] == 0)
    raw, none = ops.pad_normalise(pk, off, t)
    assert none is None and R.bits_equal_f32(_np(raw), R.pad_normalise(packed, offsets, t)[0])
    raw0, norm0 = ops.pad_normalise(pk, off, 0, _dev(mvn[0]), _dev(mvn[1]), R.NORM_MVN)
    assert tuple(raw0.shape) == (4, 0, d) and tuple(norm0.shape) == (4, 0, d)
    _, _, table0 = ops.pad_normalise(pk, off, 0, _dev(mvn[0]), _dev(mvn[1]), R.NORM_MVN, bf16_extra_rows=3)
    assert tuple(table0.shape) == (3, ops.pad_ld(d)) and np.all(_bits16(table0) == 0)


# ========================================================================================================================= metrics
@pytest.mark.parametrize('kind', R.METRIC_KINDS)
@pytest.mark.parametrize('shape', R.METRIC_SHAPES, ids=lambda s: 'B%dT%dD%d' % s[:3])
def test_metric_accumulate(shape, kind):
    """(3, 90000, 1): 270 000 frames over 1024 workgroups - stage 1's grid-stride loop takes a second trip, stage 2 reads 1024 > 256
    partials.  seq_len (T + 5, T / 2, 1): above T, inside, one frame.  Two calls into one accumulator add."""
    b, t, d, col0, width = shape
    target, pred, voiced, seq_len = R.metric_case(shape)
    code = R.METRIC_KINDS.index(kind)
    assert code == getattr(ops, 'METRIC_' + kind.upper())
    tg, pr, vo = _dev(target), _dev(pred), _dev(voiced)
    for lengths in (seq_len, None):
        total, count, bound = R.metric_sums(kind, target, pred, voiced, lengths, col0, width)
        accum = torch.zeros(2, dtype=torch.float64, device=DEV)
        args = dict(pred=None if kind == 'mean' else pr, voiced=vo if kind.startswith('sqdiff_voiced') else None,
                    seq_len=None if lengths is None else _dev(lengths), col0=col0, width=width)
        ops.metric_accumulate(code, accum, tg, **args)
        got = _np(accum)
        assert got[1] == count, (kind, shape)
        _report('metric %s' % kind, got[0], total, bound)
        ops.metric_accumulate(code, accum, tg, **args)
        twice = _np(accum)
        assert twice[1] == 2 * count and twice[0] == got[0] + got[0]
    if kind.startswith('sqdiff_voiced'):
        accum = torch.zeros(2, dtype=torch.float64, device=DEV)
        ops.metric_accumulate(code, accum, tg, pred=pr, voiced=torch.zeros_like(vo), seq_len=_dev(seq_len), col0=col0, width=width)
        assert _np(accum).tolist() == [0.0, 0.0]


def test_metric_classes_report_what_the_reference_sums_give():
    shape = R.METRIC_SHAPES[1]
    target, pred, voiced, seq_len = R.metric_case(shape)
    tg, pr, vo, sl = _dev(target), _dev(pred), _dev(voiced), _dev(seq_len)
    mcd = metrics.MelCepDistortion()
    mcd.accumulate(tg, pr, seq_len=sl)
    total, count, bound = R.metric_sums('sqdiff', target, pred, None, seq_len, col0=1)
    want = ref_cpu.metric_result('sqdiff', total, count)
    assert float(mcd.result()) == pytest.approx(want, abs=bound / (2 * want * count) + 1e-15)
    lf0 = metrics.LF0Distortion()
    lf0.accumulate(tg[:, :, :1].contiguous(), pr[:, :, :1].contiguous(), vo, seq_len=sl)
    total, count, bound = R.metric_sums('sqdiff_voiced_exp', target[:, :, :1], pred[:, :, :1], voiced, seq_len)
    want = ref_cpu.metric_result('sqdiff_voiced_exp', total, count)
    assert float(lf0.result()) == pytest.approx(want, abs=bound / (2 * want * count) + 1e-15)


# ======================================================================================================================= optimiser
@pytest.mark.parametrize('grad_scale', [1.0, 0.5])
@pytest.mark.parametrize('weight_decay', [0.0, 1e-2])
@pytest.mark.parametrize('n', R.ADAM_SIZES)
def test_adam_step(n, weight_decay, grad_scale):
    """Three steps; every step is held to one float64 update FROM THE DEVICE'S OWN previous state, so the bounds do not compound; the
    device-scalar form must give the same bits from the same inputs.  n = 10 007: ten workgroups, the last one partly idle."""
    param, grads = R.adam_case(n)
    p, m, v = _dev(param), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    for step, g in enumerate(grads, 1):
        before = [_np(x).copy() for x in (p, m, v)]
        gd = _dev(g)
        ops.adam_step(p, gd, m, v, R.ADAM_LR, R.ADAM_BETAS, R.ADAM_EPS, weight_decay, step, grad_scale)
        ss, bc = ops.adam_scalars(R.ADAM_LR, R.ADAM_BETAS, step)
        assert (F32(ss), F32(bc)) == R.adam_scalars(R.ADAM_LR, R.ADAM_BETAS, step)
        want = R.adam_step(before[0], g, before[1], before[2], ss, bc, R.ADAM_BETAS, R.ADAM_EPS, weight_decay, grad_scale)
        for name, got, w, bound in (('p', p, want[0], want[3]), ('m', m, want[1], want[4]), ('v', v, want[2], want[5])):
            _report('adam_step ' + name, _np(got), w, bound)
        scalars = _dev(np.array([ss, bc], dtype=F32))
        ops.adam_step_dev(p2, gd, m2, v2, R.ADAM_BETAS, R.ADAM_EPS, weight_decay, scalars, grad_scale)
        for a, b in ((p, p2), (m, m2), (v, v2)):
            assert np.array_equal(_bits32(a), _bits32(b)), (n, step)
    if weight_decay == 0.0:
        zero = slice(n // 3, n // 3 + n // 8 + 1)                      # gradients exactly 0 in every step: m = v = 0, denom = eps
        assert np.all(_np(m)[zero] == 0) and np.all(_np(v)[zero] == 0) and np.array_equal(_np(p)[zero], param[zero])


@pytest.mark.parametrize('decay', [0.0, 0.999, 1.0])
@pytest.mark.parametrize('n', R.ADAM_SIZES)
def test_ema_update(n, decay):
    rng = np.random.RandomState(n)
    s, p = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    want, bound = R.ema_update(s, p, decay)
    shadow = _dev(s)
    ops.ema_update(shadow, _dev(p), decay)
    _report('ema_update', _np(shadow), want, bound)
    if decay == 1.0:
        assert R.bits_equal_f32(_np(shadow), s)


def test_zz_worst_ratios():
    """Runs last in this file: the table DESIGN.md 4.23 is filled from."""
    print('\ncheck -> worst device error / bound')
    for check in sorted(RATIOS):
        print('  %-28s %.3f (ceiling %.1f)' % (check, RATIOS[check], R.ratio_ceiling(check)))
    # every reduction at or below half its bound, every element-wise check within it (datapath_ref.ratio_ceiling says why they differ)
    assert [c for c in RATIOS if RATIOS[c] > R.ratio_ceiling(c)] == []
