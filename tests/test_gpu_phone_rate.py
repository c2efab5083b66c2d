"""The phone-rate segment kernels (csrc/phone_rate.hip, csrc/phone_front.h) against tests/phone_rate_ref.py at the shapes where their
branches change: the exact family bit for bit, the bounded family element by element within a derived float32 bound.
tests/test_phone_rate_ref_host.py shows on the CPU that the bounds admit a correct kernel and refuse a broken one; DESIGN.md 4.31 has
the case grid and the measured ratios.  One launch per check; every output is poisoned (NaN, 0xffff for bf16, -77 for int32) before the
call, so a column or row the kernel must write is seen if skipped.  The launches go through the binding with buffers of the test's
own - the morgana_amd.ops wrappers allocate their outputs themselves and give ldg = ldo - and once per kernel through the wrapper,
which must return the same bits.  Every check prints its worst error / bound."""
import functools

import numpy as np
import pytest
import torch

import datapath_ref as D
import phone_rate_ref as R
from morgana_amd import _lib, ops
from morgana_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32 = np.float32
F64 = np.float64
RATIOS = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _bf16_dev(values):
    """float32 values that are bf16 numbers -> a bf16 device tensor of the same bits."""
    bits = D.bf16_bits(values)
    assert np.array_equal(D.bf16_to_f32(bits), np.asarray(values, dtype=F32))
    return _dev(bits.view(np.int16)).view(torch.bfloat16)


def _bits16(t):
    return _np(t.view(torch.int16)).view(np.uint16)


def _poison(shape, dtype=torch.float32):
    if dtype == torch.float32:
        return torch.full(shape, float('nan'), dtype=torch.float32, device=DEV)
    if dtype == torch.int32:
        return torch.full(shape, -77, dtype=torch.int32, device=DEV)
    return torch.full(tuple(shape[:-1]) + (2 * shape[-1],), 0xff, dtype=torch.uint8, device=DEV).view(torch.bfloat16)      # 0xffff: a NaN


def _report(check, got, want, bound, quiet=False):
    """Element-wise |got - want| <= bound (NaN exactly where wanted); prints (unless `quiet`) and records the worst ratio."""
    got, want, bound = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64), np.asarray(bound, dtype=F64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), '%s: NaN pattern differs' % check
    with np.errstate(all='ignore'):
        err = np.where(np.isnan(want), 0.0, np.abs(got - want))
        ratio = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    RATIOS[check] = max(RATIOS.get(check, 0.0), worst)
    if not quiet:
        print('%-28s worst err / bound %.3f over %d elements' % (check, worst, ratio.size))
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


# ================================================================================================================ segment_bounds
def _segment_bounds(rows, n_rows, pad_row, joined):
    m = rows.numel()
    if joined:
        seg = _poison((2, n_rows), torch.int32)
        s0, s1 = seg[0], seg[1]
    else:
        s0, s1 = _poison((n_rows + 4,), torch.int32)[:n_rows], _poison((n_rows,), torch.int32)
    mapped = _poison((m,), torch.int32) if pad_row is not None else None
    _lib.check(_lib.load().mg_segment_bounds(_p(rows), m, n_rows, _p(s0), _p(s1), _p(mapped), -1 if pad_row is None else pad_row,
                                             _stream()), 'mg_segment_bounds')
    return torch.stack([s0, s1]), mapped


@pytest.mark.parametrize('kind', R.BOUNDS_KINDS)
@pytest.mark.parametrize('m', R.BOUNDS_M)
def test_segment_bounds(m, kind):
    """M = 255 / 256 / 257 / 700: the last frame of a workgroup reads `next` from the following one, the first `prev` from the one
    before (a run ends on frame 255, the next starts on 256); frame 0 and frame M - 1 read the -2 sentinels; ids >= R and -1 own no
    run; the joined (2, R) buffer (one memset) and two separate buffers (two)."""
    rows, n_rows = R.bounds_map(m, kind)
    want_seg, want_mapped = R.segment_bounds(rows, n_rows, n_rows)
    if kind == 'runs' and m > 257:                                     # at M = 257 frame 256 is the last frame: a pad frame
        assert 256 in want_seg[0] and 256 in want_seg[1]
    for joined in (True, False):
        seg, mapped = _segment_bounds(_dev(rows), n_rows, n_rows, joined)
        assert np.array_equal(_np(seg), want_seg), (m, kind, joined)
        assert np.array_equal(_np(mapped), want_mapped), (m, kind, joined)
    seg, none = _segment_bounds(_dev(rows), n_rows, None, True)
    assert none is None and np.array_equal(_np(seg), want_seg)
    seg2, mapped2 = ops.segment_bounds(_dev(rows), n_rows, pad_row=n_rows)
    assert np.array_equal(_np(seg2), want_seg) and np.array_equal(_np(mapped2), want_mapped)


# =================================================================================================================== segment_sum
def _segment_sum(g, ldg, rows, seg, n_rows, extra, n, ldo, bf16):
    out = _poison((n_rows + extra, ldo), torch.bfloat16 if bf16 else torch.float32)
    _lib.check(_lib.load().mg_segment_sum(_p(g), ldg, int(bf16), _p(rows), rows.numel(), _p(seg[0]), _p(seg[1]), n_rows, extra, n, _p(out),
                                          ldo, _stream()), 'mg_segment_sum')
    return out


def _check_sums(check, out, ref, n, bf16):
    if bf16:
        bits = _bits16(out)
        assert D.bits_equal_bf16(bits, ref['bits']), check
        assert not np.any(D.bf16_is_nan(bits)) and np.all(bits[:, n:] == 0), check
        got = D.bf16_to_f32(bits)
    else:
        got = _np(out)
        assert D.bits_equal_f32(got, ref['exact']), check
        assert np.all(got[:, n:].view(np.uint32) == 0), check
    _report(check, got, ref['sum'], ref['bound'])


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('case', R.SEGSUM_CASES, ids=lambda c: 'M%d_N%d_%s_x%d_%s' % (c[0], c[1], 'ld' if c[2] else 'tight', c[3], c[4]))
def test_segment_sum(case, bf16):
    """Segments of 0, 1, 3, 4, 5, 7, 8, 9 and 21 frames: the 4-unrolled body with and without the remainder loop.  N = 520: a second
    blockIdx.y whose lanes 1 .. 63 are idle; ldo = N + 8: a zero chunk; ldg = N + 16 holds values the sum must not read.  extra = 5
    with a share that has no pad frame, 3 over 7 frames (the last share short), 12 over 7 (empty shares), 1 over 63 / 64 / 65 / 130
    frames (the ballot loop's trips), 0.  Pad frames as -1 and as the id R."""
    m, n, padded, extra, pad = case
    g, rows, n_rows, ldg, ldo = R.segsum_case(m, n, padded, extra, pad, bf16)
    seg, _ = R.segment_bounds(rows, n_rows)
    ref = R.segment_sum(g, rows, seg, n_rows, extra, n, ldo, bf16)
    if (m, extra) == (130, 5):
        assert min(s.size for s in R.pad_shares(rows, n_rows, extra)) == 0          # a share with no pad frame
    gd = _bf16_dev(g) if bf16 else _dev(g)
    assert gd.data_ptr() % 16 == 0
    name = 'segment_sum %s sum' % ('bf16' if bf16 else 'f32')
    out = _segment_sum(gd, ldg, _dev(rows), _dev(seg), n_rows, extra, n, ldo, bf16)
    _check_sums(name, out, ref, n, bf16)
    if not padded:
        out2 = ops.segment_sum(gd, _dev(rows), _dev(seg), n_rows, n, extra=extra)
        assert torch.equal(out2.view(torch.int16 if bf16 else torch.int32), out.view(torch.int16 if bf16 else torch.int32))


def test_a_gradient_off_its_16_byte_boundary_is_refused_without_a_launch():
    g, rows, n_rows, _, _ = R.segsum_case(7, 8, False, 3, 'minus1', False)
    seg, _ = R.segment_bounds(rows, n_rows)
    buf = torch.zeros(g.size + 1, dtype=torch.float32, device=DEV)
    off = buf[1:].view(g.shape)
    off.copy_(torch.from_numpy(g))
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    _no_launch(lambda: ops.segment_sum(off, _dev(rows), _dev(seg), n_rows, 8, extra=3), '16-byte')
    with pytest.raises(ValueError, match='16-byte'):                      # and the entry point itself
        _segment_sum(off, 8, _dev(rows), _dev(seg), n_rows, 3, 8, 8, False)


# ========================================================================================== segment_sum_feat + feat_wgrad_reduce
@pytest.mark.parametrize('case', R.FEAT_CASES, ids=lambda c: 'R%d_x%d_N%d_C%d_col%d_%s' % (c[:5] + ('acc' if c[5] else 'set',)))
def test_segment_sum_feat_and_feat_wgrad_reduce(case):
    """C = 1 / 16: one live lane of the feature load, the readlane loop's last slot; N = 520: a second column block in `red` and the
    slabs; R + extra = 5: all but five waves idle (their slabs must be written as zeros), 2048: one row per wave, 2049 / 4500: two
    and three, the last wave short, wave 1000 of R = 2001 crossing from the phone rows into the extra rows; segment_map(130): rows of
    7, 8, 9 and 21 frames through the frame loop's unrolled body, against the exact replay.  dW outside
    [col0, col0 + C) keeps its bits."""
    n_rows, extra, n, c, col0, accumulate = case
    g, rows, feat, prior = R.feat_case(*case)
    seg, _ = R.segment_bounds(rows, n_rows)
    ref = R.segment_sum(g, rows, seg, n_rows, extra, n, n, True)
    want, bound, _ = R.feat_wgrad(g, feat, rows, seg, n_rows, extra, n, prior if accumulate else None, col0)
    lib = _lib.load()
    gd, rd, sd, fd = _bf16_dev(g), _dev(rows), _dev(seg), _dev(feat)
    out = _poison((n_rows + extra, n), torch.bfloat16)
    nbytes = lib.mg_segment_sum_feat_workspace_bytes(c, n)
    slabs = _poison((nbytes // 4,))
    _lib.check(lib.mg_segment_sum_feat_bf16(_p(gd), n, _p(rd), rows.size, _p(sd[0]), _p(sd[1]), n_rows, extra, n, _p(out), n, _p(fd), c, _p(slabs),
                                            nbytes, _stream()), 'mg_segment_sum_feat_bf16')
    _check_sums('segment_sum_feat sum', out, ref, n, True)
    assert not np.any(np.isnan(_np(slabs)))
    dw = _dev(prior)
    ops.feat_wgrad_reduce(slabs, c, n, n, dw, col0, accumulate=accumulate)
    got = _np(dw)
    keep = np.ones(prior.shape[1], dtype=bool)
    keep[col0:col0 + c] = False
    assert D.bits_equal_f32(got[:, keep], prior[:, keep])
    if accumulate:
        _report('feat_wgrad dW', got, want, bound)
    else:
        _report('feat_wgrad dW', got[:, col0:col0 + c], want, bound)
    out2, slabs2 = ops.segment_sum_feat(gd, rd, sd, n_rows, n, fd, extra=extra)
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16)) and torch.equal(slabs2.view(torch.int32), slabs.view(torch.int32))


# ============================================================================================================ phone_concat_layer
def _concat_layer(p, rows, feat, w, col0, bias, n, act, ldy, out_f32):
    m, c = feat.shape
    y = _poison((m, ldy), torch.float32 if out_f32 else torch.bfloat16)
    _lib.check(_lib.load().mg_phone_concat_layer_bf16(_p(p), p.shape[1], _p(rows), m, _p(feat), c, _p(w), w.shape[1], col0, _p(bias), n, act,
                                                      _p(y), ldy, int(out_f32), _stream()), 'mg_phone_concat_layer_bf16')
    return y


def _check_concat(case, n, act, ldy, out_f32, with_bias=True, quiet=False):
    p, rows, feat, w, bias = case
    want, bound = R.phone_concat_layer(p, rows, feat, w, 600, bias if with_bias else None, n, act, ldy, out_f32)
    y = _concat_layer(_dev(p), _dev(rows), _dev(feat), _dev(w), 600, _dev(bias) if with_bias else None, n, act, ldy, out_f32)
    got = _np(y) if out_f32 else D.bf16_to_f32(_bits16(y))
    assert np.all(got[:, n:].view(np.uint32) == 0), (n, act, ldy)
    _report('phone_concat_layer %s' % ('f32' if out_f32 else 'bf16'), got, want, bound, quiet=quiet)


@pytest.mark.parametrize('out_f32', [True, False], ids=['f32', 'bf16'])
@pytest.mark.parametrize('n', R.PCL_N)
def test_phone_concat_layer(n, out_f32):
    """The binding with a P of the test's own, so the bound is this kernel's alone.  ldy = pad8(N) and pad8(N) + 8: N = 250 and 256 run
    the 4-column template at ldy = 256 and the 8-column one at 264, on the same values; N = 257, 512, 520 the 8-column one, 520 with a
    second blockIdx.y; N = 1, 20, 250, 257: a lane whose columns straddle N (`c0 + e >= N`), lanes with none (`has_p`, `live`).
    C = 1, 9, 16; M = 1, 15, 16, 17, 100: a partial chunk, one chunk, a second; the map changes its row on a chunk edge, inside a chunk,
    and holds one row over three chunks and pad frames.  Four activations; without a bias at C = 9."""
    for c, m in R.PCL_CM:
        case = R.concat_case(m, n, c)
        for act in (R.ACT_NONE, R.ACT_SIGMOID, R.ACT_TANH, R.ACT_RELU):
            for ldy in (R.pad8(n), R.pad8(n) + 8):
                _check_concat(case, n, act, ldy, out_f32, quiet=True)
        if c == 9:
            _check_concat(case, n, R.ACT_SIGMOID, R.pad8(n), out_f32, with_bias=False, quiet=True)
    name = 'phone_concat_layer %s' % ('f32' if out_f32 else 'bf16')
    print('%-28s worst err / bound so far %.3f (N = %d: 50 launches)' % (name, RATIOS[name], n))


def test_phone_concat_layer_grid_stride():
    """M = 262 144 + 21 frames: 16 386 chunks want 1025 workgroups and the grid stops at 1024, so the first waves take five trips of the
    grid-stride loop and the others four (M = 100 already has a second trip: 7 chunks on one workgroup's 4 waves)."""
    m, n, c = 262144 + 21, 8, 9
    _check_concat(R.concat_case(m, n, c), n, R.ACT_SIGMOID, 8, True)


def test_phone_concat_layer_through_the_wrapper():
    """ops.phone_concat_layer puts the phone-rate GEMM in front: with exact operands (a 0 / 1 table, weights on a 2^-6 grid) its P is
    exact and the wrapper's output obeys the same bound."""
    m, n, c, k = 100, 20, 9, 16
    rng = np.random.RandomState(20261108)
    table = (rng.uniform(size=(R.PCL_TABLE_ROWS, k)) < 0.5).astype(F32)
    w = np.concatenate([rng.randint(-32, 33, size=(n, k)) / 64.0, rng.uniform(-0.5, 0.5, (n, c))], axis=1).astype(F32)
    _, rows, feat, _, bias = R.concat_case(m, n, c)
    p = (table.astype(F64) @ w[:, :k].astype(F64).T).astype(F32)
    want, bound = R.phone_concat_layer(np.pad(p, ((0, 0), (0, 4))), rows, feat, w, k, bias, n, R.ACT_TANH, R.pad8(n), True)
    (w_bf,), _ = ops.cast_params_bf16([_dev(w)], want_plain=True, want_t=())
    y = ops.phone_concat_layer(ops.cast_pad_bf16(_dev(table)), k, _dev(rows), _dev(feat), _dev(w), w_bf, _dev(bias), n, ops.ACT_TANH, out_f32=True)
    _report('phone_concat_layer f32', _np(y), want, bound)


# ============================================================================================= phone_target_stats / phone_front
@functools.lru_cache(maxsize=None)
def _stats_inputs(case, lengths):
    b, p, t, extra = case
    dur, target, seq = R.stats_case(b, p, t, extra, lengths)
    rows, mapped, seg = R.stats_map(dur, t)
    ref = {front: R.phone_target_stats(target, rows, seg, seq, b, t, b * p, extra, p, front) for front in (False, True)}
    return dur, target, seq, rows, mapped, seg, ref


def _check_stats(name, ref, ybar, weight, partials):
    _report(name + ' weight', _np(weight), ref['weight'], ref['weight_bound'])
    _report(name + ' ybar', _np(ybar), ref['ybar'], ref['ybar_bound'])
    slots = _np(partials.view(torch.float32)).astype(F64)
    _report(name + ' const', slots.sum(), ref['const'], ref['const_bound'])


@pytest.mark.parametrize('lengths', R.STATS_LENGTHS)
@pytest.mark.parametrize('case', R.STATS_CASES, ids=lambda c: 'B%d_P%d_T%d_x%d' % c)
def test_phone_target_stats_and_phone_front(case, lengths):
    """R = 1, 15, 16, 17, 100: a short last block of 16-lane rows; extra = 1, 3, 4, 5, 8: a short last block of extra-row waves; phones of 0,
    1, 15, 16, 17 and 40 frames: the 16-lane loop's second and third trip; seq_len inside a phone, on its edge, before it, above T, 0,
    negative, None; pad frames inside and outside seq_len; 'empty': utterance 0 owns frames and has n_b = 0 - NaN weights, ybar 0, a NaN
    constant.  The map with -1 and with the pad row give the same bits.  phone_front wherever ops.phone_front_ok holds: the same
    reference, its own depth for the constant; its maps against datapath_ref."""
    b, p, t, extra = case
    dur, target, seq, rows, mapped, seg, ref = _stats_inputs(case, lengths)
    n_rows = b * p
    lib = _lib.load()
    td, sd, ld = _dev(target), _dev(seg), _dev(seq) if seq is not None else None
    got = []
    for frame_map in (_dev(rows), _dev(mapped)):
        stats = _poison((2, n_rows + extra))
        nbytes = lib.mg_phone_target_stats_workspace_bytes(n_rows, extra)
        assert nbytes == 4 * R.n_partials(n_rows, extra)
        ws = _poison((nbytes // 4,))
        const = _poison((1,))
        _lib.check(lib.mg_phone_target_stats(_p(td), _p(frame_map), b * t, _p(sd[0]), _p(sd[1]), _p(ld), b, t, n_rows, extra, _p(stats[0]),
                                             _p(stats[1]), _p(const), _p(ws), nbytes, _stream()), 'mg_phone_target_stats')
        _check_stats('stats', ref[False], stats[0], stats[1], ws)
        want_const = R.loss_const_add(_np(ws))                              # the constant without accumulation: its own replay
        assert np.isnan(want_const) == np.isnan(_np(const)[0]) and (np.isnan(want_const) or D.bits_equal_f32(_np(const), [want_const]))
        got.append((_np(stats), _np(ws)))
    assert np.array_equal(got[0][0], got[1][0], equal_nan=True) and np.array_equal(got[0][1], got[1][1], equal_nan=True)
    ybar2, weight2, ws2 = ops.phone_target_stats(td, _dev(mapped), sd, ld, b, t, n_rows, extra)
    assert np.array_equal(_np(ybar2), got[0][0][0], equal_nan=True) and np.array_equal(_np(weight2), got[0][0][1], equal_nan=True)
    assert ops.phone_front_ok(b, p, t, extra) == R.front_ok(b, p, t, extra)
    if R.front_ok(b, p, t, extra):
        dd = _dev(dur)
        maps_f, seg_f, stats_f = _poison((2, b * t), torch.int32), _poison((2, n_rows), torch.int32), _poison((2, n_rows + extra))
        ws_f = _poison((R.n_partials(n_rows, extra),))
        _lib.check(lib.mg_phone_front(_p(dd), b, p, t, _p(td), _p(ld), extra, _p(maps_f[0]), _p(maps_f[1]), n_rows, _p(seg_f[0]), _p(seg_f[1]),
                                      _p(stats_f[0]), _p(stats_f[1]), _p(ws_f), 4 * ws_f.numel(), _stream()), 'mg_phone_front')
        assert np.array_equal(_np(maps_f[0]), rows) and np.array_equal(_np(maps_f[1]), mapped)
        assert np.array_equal(_np(seg_f), seg)
        assert not np.any(np.isnan(_np(ws_f))) or np.isnan(ref[True]['const'])       # every slot written, the ones no job owns as zeros
        _check_stats('front', ref[True], stats_f[0], stats_f[1], ws_f)
        wrapped = ops.phone_front(dd, td, ld, t, extra)                       # the wrapper: the same bits
        for ours, theirs in zip((maps_f[0], maps_f[1], seg_f, stats_f[0], stats_f[1], ws_f), wrapped):
            assert np.array_equal(_np(ours).reshape(-1), _np(theirs.view(ours.dtype)).reshape(-1), equal_nan=True)


def test_phone_front_cases_exist():
    assert sum(R.front_ok(*c) for c in R.STATS_CASES) >= 3


def test_phone_target_stats_without_an_extra_row_is_refused_without_a_launch():
    """extra = 0 would leave the pad frames' loss terms nowhere: refused (csrc/phone_rate.hip, mg_phone_target_stats)."""
    b, p, t, extra = R.STATS_CASES[1]
    dur, target, seq, rows, mapped, seg, _ = _stats_inputs(R.STATS_CASES[1], 'cut')
    _no_launch(lambda: ops.phone_target_stats(_dev(target), _dev(mapped), _dev(seg), _dev(seq), b, t, b * p, 0), 'extra')
    lib = _lib.load()
    stats, ws = _poison((2, b * p)), _poison((8,))
    td, md, sd, ld = _dev(target), _dev(mapped), _dev(seg), _dev(seq)
    with pytest.raises(ValueError, match='extra'):                          # and the entry point itself
        _lib.check(lib.mg_phone_target_stats(_p(td), _p(md), b * t, _p(sd[0]), _p(sd[1]), _p(ld), b, t, b * p, 0, _p(stats[0]), _p(stats[1]), None,
                                             _p(ws), 32, _stream()), 'mg_phone_target_stats')
    assert np.all(np.isnan(_np(stats))) and np.all(np.isnan(_np(ws)))


# ================================================================================================================ phone_mse_rows
@pytest.mark.parametrize('ldp', [1, 8])
@pytest.mark.parametrize('n', R.MSE_ROWS_N)
def test_phone_mse_rows(n, ldp):
    """n = 1025, 2500: rows 1024 .. take a second and third trip of the 1024 threads; every fifth weight an exact zero beside a
    prediction of 1e30 (the `w > 0` guard: dpred is 0, the loss finite); one NaN weight: NaN dpred in that row alone, a NaN loss -
    and the same rows with that weight set to 1 / n: the loss within its bound."""
    pred, ybar, weight = R.mse_rows_case(n, ldp)
    for with_nan in (True, False):
        w = weight.copy()
        if not with_nan and n >= 4:
            w[3] = F32(1.0 / n)
        want_d, bound_d, want_l, bound_l = R.phone_mse_rows(pred[:, 0], ybar, w)
        out = _poison((n + 1,))
        pd, yd, wd = _dev(pred), _dev(ybar), _dev(w)                        # named: a temporary's memory is handed to the next one
        _lib.check(_lib.load().mg_phone_mse_rows_f32(_p(pd), ldp, _p(yd), _p(wd), n, _p(out[n:]), _p(out), _stream()), 'mg_phone_mse_rows_f32')
        got = _np(out)
        _report('phone_mse_rows dpred', got[:n], want_d, bound_d)
        _report('phone_mse_rows loss', got[n], want_l, bound_l)
        assert np.all(got[:n][w == 0].view(np.uint32) == 0)
        loss2, dpred2 = ops.phone_mse_rows(pd, yd, wd)
        assert np.array_equal(_np(dpred2), got[:n], equal_nan=True) and np.array_equal(_np(loss2), got[n:], equal_nan=True)


# ================================================================================================== expand_column, the constant
@pytest.mark.parametrize('slots', R.PARTIAL_SLOTS, ids=lambda s: '%dslots' % R.n_partials(*s))
@pytest.mark.parametrize('m', R.EXPAND_M)
def test_expand_column_and_the_loss_constant(m, slots):
    """M = 255 / 256 / 257 / 700: a ragged last workgroup, which is also the one that adds the constant; 1, 255, 256, 257, 300 partial
    slots: threads without a slot, one slot each, a second trip for thread 0, for 44 threads.  The constant is added to a loss the
    test wrote; mg_phone_loss_const_add gives the same bits."""
    n_rows, extra = slots
    table, rows, partial, loss = R.expand_case(m, n_rows, extra)
    want = R.expand_column(table, rows)
    want_loss = R.loss_const_add(partial, loss)
    lib = _lib.load()
    td, rd, pd = _dev(table), _dev(rows), _dev(partial)
    out = _poison((m,))
    _lib.check(lib.mg_expand_column_f32(_p(td), _p(rd), m, _p(out), _stream()), 'mg_expand_column_f32')
    assert D.bits_equal_f32(_np(out), want)
    out = _poison((m,))
    ld = _dev(np.array([loss, 7.0], dtype=F32))
    _lib.check(lib.mg_expand_column_loss_f32(_p(td), _p(rd), m, _p(out), _p(pd), n_rows, extra, _p(ld), _stream()), 'mg_expand_column_loss_f32')
    assert D.bits_equal_f32(_np(out), want)
    assert D.bits_equal_f32(_np(ld), [want_loss, 7.0])
    ld2 = _dev(np.array([loss, 7.0], dtype=F32))
    ops.phone_loss_const_add(pd, n_rows, extra, ld2[0])
    assert D.bits_equal_f32(_np(ld2), [want_loss, 7.0])
    ld3 = _dev(np.array([loss], dtype=F32))
    assert D.bits_equal_f32(_np(ops.expand_column(td, rd, loss_const=(pd, n_rows, extra, ld3[0]))), want)
    assert D.bits_equal_f32(_np(ld3), [want_loss]) and D.bits_equal_f32(_np(ops.expand_column(td, rd)), want)


def test_zz_worst_ratios():
    """Runs last in this file: the table DESIGN.md 4.31 is filled from."""
    print('\ncheck -> worst device error / bound')
    for check in sorted(RATIOS):
        print('  %-28s %.3f (ceiling %.1f)' % (check, RATIOS[check], R.ratio_ceiling(check)))
    assert [c for c in RATIOS if RATIOS[c] > R.ratio_ceiling(c)] == []
