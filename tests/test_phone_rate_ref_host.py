"""What tests/phone_rate_ref.py is worth, shown without a GPU:

1. its masked-MSE algebra agrees with oracle/ref_cpu.py: weight, ybar and the constant reassemble the frame-by-frame loss of a
   prediction that is constant per table row;
2. a float32 numpy EMULATION of each kernel, in the kernel's own order of operations (the lanes, the xor butterfly, the wave order,
   the slab partitions; an fma is the float64 result rounded once; the hardware exp2 and reciprocal perturbed by their charged error),
   passes its check on the cases of the GPU test (tests/test_gpu_phone_rate.py) - the worst ratio per check is recorded and printed;
3. each fault of FAULTS, planted in the emulation, makes the matching check fail.

The emulations restate csrc/phone_rate.hip operation by operation.  They are not references: they exist to show that the bounds admit
a correct kernel and refuse a broken one."""
import numpy as np
import pytest

import datapath_ref as D
import phone_rate_ref as R
from oracle import ref_cpu

F32 = np.float32
F64 = np.float64
U = R.U
RATIOS = {}            # check -> worst error / bound of the emulation
CAUGHT = {}            # fault -> checks that failed under it

FAULTS = ('remainder frames of a 5-frame phone dropped', 'pad frame on a share edge credited to the other share',
          'truncation instead of round-to-nearest-even', 'nonzero columns past N', 'mask edge as <=', 'weight over B T',
          'ybar over masked frames too', 'extra rows left out of the constant', 'P kept from the previous chunk',
          'two counter columns swapped', 'bias missing on pad frames', 'slabs 252 to 255 dropped', 'row 1024 dropped from the row loss',
          'last partial slot dropped')


# fault -> exactly the checks that fail under it (asserted by the last test)
_SEG32, _SEG16 = ['segment_sum f32 exact', 'segment_sum f32 sum'], ['segment_sum bf16 exact', 'segment_sum bf16 sum']
_PCL = ['phone_concat_layer f32', 'phone_concat_layer bf16']
FAULT_TABLE = dict(zip(FAULTS, (_SEG32, _SEG32, _SEG16, _SEG16, ['stats weight', 'stats ybar', 'stats const'], ['stats weight', 'stats const'],
                                ['stats ybar', 'stats const'], ['stats const'], _PCL, _PCL, _PCL, ['feat_wgrad dW'],
                                ['phone_mse_rows dpred', 'phone_mse_rows loss'],
                                ['loss constant exact (%d slots)' % n for n in (1, 255, 256, 257, 300)])))


def _ratio(got, want, bound):
    """Worst |got - want| / bound; inf where the NaN patterns differ or an error meets a zero bound."""
    got, want, bound = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64), np.asarray(bound, dtype=F64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return np.inf
    with np.errstate(all='ignore'):
        err = np.where(np.isnan(want), 0.0, np.abs(got - want))
        r = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def _record(check, got, want, bound):
    r = _ratio(got, want, bound)
    RATIOS[check] = max(RATIOS.get(check, 0.0), r)
    assert r <= R.ratio_ceiling(check), '%s: the emulation is at %.3f of its bound' % (check, r)
    return r


def _fails(check, got, want, bound):
    return _ratio(got, want, bound) > R.ratio_ceiling(check)


def _caught(fault, checks):
    assert fault in FAULTS
    CAUGHT.setdefault(fault, []).extend(c for c in checks if c not in CAUGHT.get(fault, []))


def _fma(a, b, c):
    return (np.asarray(a, dtype=F64) * np.asarray(b, dtype=F64) + np.asarray(c, dtype=F64)).astype(F32)


def _butterfly(v, steps):
    v = np.array(v, dtype=F32)
    idx = np.arange(v.size)
    for d in steps:
        v = (v + v[idx ^ d]).astype(F32)
    return v


# ============================================================================================================== the emulations
def emu_segment_sum(g, rows, seg, n_rows, extra, n, ldo, bf16, fault=None):
    """segment_sum_kernel: four frames per trip added as (((acc + t0) + t1) + t2) + t3, then the remainder loop; an extra row walks
    its share 64 ids at a time and adds the pad frames in bit order.  -> float32 (R + extra, ldo), or bf16 bits."""
    g = np.asarray(g, dtype=F32)
    m = g.shape[0]
    out = np.zeros((n_rows + extra, ldo), dtype=F32)
    wide = ldo if fault == 'nonzero columns past N' else n
    for r in range(n_rows):
        f, f1 = int(seg[0, r]), int(seg[1, r])
        acc = np.zeros(wide, dtype=F32)
        while f + 4 <= f1:
            for u in range(4):
                acc = (acc + g[f + u, :wide]).astype(F32)
            f += 4
        if fault != 'remainder frames of a 5-frame phone dropped':
            for ff in range(f, f1):
                acc = (acc + g[ff, :wide]).astype(F32)
        out[r, :wide] = acc
    pad = (rows < 0) | (rows >= n_rows)
    chunk = -(-m // extra) if extra else 0
    for j in range(extra):
        lo, hi = min(j * chunk, m), min((j + 1) * chunk, m)
        if fault == 'pad frame on a share edge credited to the other share':
            lo, hi = (min(lo + 1, m) if j else 0), min(hi + 1, m)
        acc = np.zeros(wide, dtype=F32)
        for base in range(lo, hi, 64):
            for f in range(base, min(base + 64, hi)):
                if pad[f]:
                    acc = (acc + g[f, :wide]).astype(F32)
        out[n_rows + j, :wide] = acc
    if not bf16:
        return out
    if fault == 'truncation instead of round-to-nearest-even':
        return (out.view(np.uint32) >> 16).astype(np.uint16)
    return D.bf16_bits(out)


def _frame_weight(f, nb, b, t, fault=None):
    """pf_frame_weight, and the phone rows' (t0 + (f - lo) < nb ? 1 : 0) * inv: the same float32 operations."""
    u, tt = f // t, f % t
    n = int(nb[u])
    with np.errstate(all='ignore'):
        inv = F32(1.0) / (F32(t if fault == 'weight over B T' else n) * F32(b))
        live = tt <= n if fault == 'mask edge as <=' else tt < n
        return F32(1.0 if live else 0.0) * inv, inv


def emu_stats(target, rows, seg, seq_len, b, t, n_rows, extra, fault=None, front_p=None):
    """phone_target_stats_kernel (front_p None) or phone_front_kernel's grouping of the constant (front_p = P).  16 lanes per phone row,
    frame f on lane (f - lo) mod 16, the xor butterfly 8, 4, 2, 1; a wave per extra row, frame f on lane (f - lo) mod 64, the butterfly
    32 .. 1.  -> (ybar, weight, partial slots) float32."""
    y = np.asarray(target, dtype=F32).reshape(-1)
    rows = np.asarray(rows).reshape(-1)
    m = rows.size
    nb = R.valid_frames(seq_len, b, t)
    nr = n_rows + extra
    ybar, weight = np.zeros(nr, dtype=F32), np.zeros(nr, dtype=F32)
    phone_blocks = -(-n_rows // 16)
    threads = np.zeros((phone_blocks + -(-extra // 4), 256), dtype=F32)        # c per thread of phone_target_stats_kernel
    jobs = np.zeros((b + -(-extra // 4), 256), dtype=F32) if front_p else None  # c per thread of phone_front_kernel
    with np.errstate(all='ignore'):
        for r in range(n_rows):
            lo, hi = int(seg[0, r]), int(seg[1, r])
            ws, wy, c = np.zeros(16, dtype=F32), np.zeros(16, dtype=F32), np.zeros(16, dtype=F32)
            ws_all, wy_all = np.zeros(16, dtype=F32), np.zeros(16, dtype=F32)
            for f in range(lo, hi):
                w, inv = _frame_weight(f, nb, b, t, fault)
                s = (f - lo) % 16
                ws[s] = ws[s] + w
                wy[s] = wy[s] + F32(w * y[f])
                ws_all[s] = ws_all[s] + inv
                wy_all[s] = wy_all[s] + F32(inv * y[f])
            w_sum, wy_sum = _butterfly(ws, (8, 4, 2, 1))[0], _butterfly(wy, (8, 4, 2, 1))[0]
            mean = F32(wy_sum / w_sum) if w_sum > 0 else F32(0)
            if fault == 'ybar over masked frames too' and w_sum > 0:
                mean = F32(_butterfly(wy_all, (8, 4, 2, 1))[0] / _butterfly(ws_all, (8, 4, 2, 1))[0])
            for f in range(lo, hi):
                w, _ = _frame_weight(f, nb, b, t, fault)
                d = F32(y[f] - mean)
                s = (f - lo) % 16
                c[s] = c[s] + F32(F32(w * d) * d)
                if front_p:                                                 # one accumulator per thread over the utterance's passes
                    tid = (r % front_p) % 16 * 16 + s
                    jobs[r // front_p, tid] = jobs[r // front_p, tid] + F32(F32(w * d) * d)
            ybar[r], weight[r] = mean, w_sum
            threads[r // 16, (r % 16) * 16:(r % 16) * 16 + 16] = c
        pad = (rows < 0) | (rows >= n_rows)
        chunk = -(-m // extra)
        for j in range(extra):
            lo, hi = min(j * chunk, m), min((j + 1) * chunk, m)
            ws, wy, c = np.zeros(64, dtype=F32), np.zeros(64, dtype=F32), np.zeros(64, dtype=F32)
            fr = [f for f in range(lo, hi) if pad[f]]
            for f in fr:
                w, _ = _frame_weight(f, nb, b, t, fault)
                s = (f - lo) % 64
                ws[s] = ws[s] + w
                wy[s] = wy[s] + F32(w * y[f])
            w_sum, wy_sum = _butterfly(ws, (32, 16, 8, 4, 2, 1))[0], _butterfly(wy, (32, 16, 8, 4, 2, 1))[0]
            mean = F32(wy_sum / w_sum) if w_sum > 0 else F32(0)
            for f in fr:
                w, _ = _frame_weight(f, nb, b, t, fault)
                d = F32(y[f] - mean)
                s = (f - lo) % 64
                c[s] = c[s] + F32(F32(w * d) * d)
            ybar[n_rows + j], weight[n_rows + j] = mean, w_sum
            if fault == 'extra rows left out of the constant':
                c[:] = 0
            threads[phone_blocks + j // 4, (j % 4) * 64:(j % 4) * 64 + 64] = c
            if front_p:                                                     # wave 0 works the job's four rows off one after the other
                jobs[b + j // 4, :64] = jobs[b + j // 4, :64] + c
        if not front_p:
            return ybar, weight, np.array([R.tree256_f32(v) for v in threads], dtype=F32)
        partial = np.zeros(R.n_partials(n_rows, extra), dtype=F32)
        for job, v in enumerate(jobs):
            tot = F32(0)
            for wv in range(4):
                tot = tot + _butterfly(v[64 * wv:64 * wv + 64], (32, 16, 8, 4, 2, 1))[0]
            partial[job if job < b else phone_blocks + job - b] = tot
        return ybar, weight, partial


def emu_mse_rows(pred, ybar, weight, fault=None):
    """phone_mse_rows_kernel: thread r mod 1024 adds its rows in double, the 1024-entry halving tree, one cast."""
    n = ybar.size
    dpred = np.zeros(n, dtype=F32)
    part = np.zeros(1024, dtype=F64)
    with np.errstate(all='ignore'):
        for r in range(n):
            if fault == 'row 1024 dropped from the row loss' and r == 1024:
                continue
            w = weight[r]
            d = F32(pred[r] - ybar[r]) if w > 0 else F32(0)
            dpred[r] = F32(F32(2) * w) * d
            part[r % 1024] += F64(F32(w * d)) * F64(d)
        s = 512
        while s > 0:
            part[:s] += part[s:2 * s]
            s >>= 1
    return dpred, F32(part[0])


def emu_concat(p, rows, feat, w, col0, bias, n, act, ldy, out_f32, fault=None, sign=1.0):
    """phone_concat_layer_kernel: pz = b + P[row], then the counters by fmaf in ascending c; mg_sigmoid_fast as rcp(1 + exp2(-z log2 e))
    with exp2 and rcp moved by `sign` times one unit in the last place, their charged error; tanhf as the rounded float64 tanh."""
    rows = np.asarray(rows).reshape(-1)
    m, c = feat.shape
    src = rows.copy()
    if fault == 'P kept from the previous chunk':
        for f in range(R.PCL_CHUNK, m, R.PCL_CHUNK):                        # the first run of a chunk reads the row the last chunk ended on
            k = f
            while k < min(f + R.PCL_CHUNK, m) and rows[k] == rows[f]:
                src[k] = rows[f - 1]
                k += 1
    x = np.asarray(feat, dtype=F32)
    if fault == 'two counter columns swapped':
        x = x.copy()
        x[:, [0, 1]] = x[:, [1, 0]]
    bv = np.zeros(n, dtype=F32) if bias is None else np.asarray(bias, dtype=F32)[:n]
    bv = np.broadcast_to(bv, (m, n))
    if fault == 'bias missing on pad frames':
        bv = np.where((rows == R.PCL_TABLE_ROWS - 1)[:, None], F32(0), bv)
    z = (bv + np.asarray(p, dtype=F32)[src, :n]).astype(F32)
    for k in range(c):
        z = _fma(x[:, k:k + 1], np.asarray(w, dtype=F32)[None, :n, col0 + k], z)
    with np.errstate(all='ignore'):
        if act == R.ACT_SIGMOID:
            e = (np.exp2((z * F32(-1.4426950408889634)).astype(F32).astype(F64)) * (1 + sign * 2 * U)).astype(F32)
            z = ((1.0 / (F32(1) + e).astype(F32).astype(F64)) * (1 - sign * 2 * U)).astype(F32)
        elif act == R.ACT_TANH:
            z = np.tanh(z.astype(F64)).astype(F32)
        elif act == R.ACT_RELU:
            z = np.where(z < 0, F32(0), z)
    out = np.zeros((m, ldy), dtype=F32)
    out[:, :n] = z if out_f32 else D.bf16_to_f32(D.bf16_bits(z))
    return out


def emu_feat_wgrad(g, feat, rows, seg, n_rows, extra, n, prior, col0, accumulate, fault=None):
    """segment_sum_feat_kernel's feature half and feat_wgrad_reduce_kernel: a wave keeps one fmaf accumulator per (c, column) over the
    frames of its row range; the 8 waves of a workgroup are added in wave order from zero; the reduce adds slabs q, q + 4, ... per
    partition q and then ((p0 + p1) + p2) + p3."""
    g, x = np.asarray(g, dtype=F32)[:, :n], np.asarray(feat, dtype=F32)
    c = x.shape[1]
    frames = R.row_frames(rows, seg, n_rows, extra)
    nr = n_rows + extra
    per = -(-nr // (R.SSF_BLOCKS * R.SSF_WAVES))
    slabs = np.zeros((R.SSF_BLOCKS, c, n), dtype=F32)
    for blk in range(R.SSF_BLOCKS):
        for wave in range(R.SSF_WAVES):
            r_lo = (blk * R.SSF_WAVES + wave) * per
            cacc = np.zeros((c, n), dtype=F32)
            for r in range(r_lo, min(r_lo + per, nr)):
                for f in frames[r]:
                    cacc = _fma(x[f][:, None], g[f][None, :], cacc)
            slabs[blk] = cacc if wave == 0 else (slabs[blk] + cacc).astype(F32)
    if fault == 'slabs 252 to 255 dropped':
        slabs[252:] = 0
    part = np.zeros((4, c, n), dtype=F32)
    for q in range(4):
        for blk in range(q, R.SSF_BLOCKS, 4):
            part[q] = (part[q] + slabs[blk]).astype(F32)
    total = (((part[0] + part[1]).astype(F32) + part[2]).astype(F32) + part[3]).astype(F32).T
    if not accumulate:
        return total
    dw = np.array(prior, dtype=F32)
    dw[:, col0:col0 + c] = (dw[:, col0:col0 + c] + total).astype(F32)
    return dw


# ================================================================================================== the reference and the oracle
@pytest.mark.parametrize('lengths', ['none', 'cut', 'over'])
@pytest.mark.parametrize('case', R.STATS_CASES, ids=lambda c: 'B%d_P%d_T%d_x%d' % c)
def test_the_statistics_reassemble_the_oracles_masked_mse(case, lengths):
    """sum_r weight[r] (p_r - ybar[r])^2 + const equals the frame-by-frame masked MSE (oracle.ref_cpu.mse, float32: to 1e-5; the same
    formula in float64: to 1e-12) for a prediction that is constant per table row."""
    b, p, t, extra = case
    dur, target, seq = R.stats_case(b, p, t, extra, lengths)
    rows, mapped, seg = R.stats_map(dur, t)
    ref = R.phone_target_stats(target, mapped, seg, seq, b, t, b * p, extra)
    pred_rows = np.random.RandomState(3).standard_normal(b * p + extra)
    want, pred_frames = R.frame_loss(pred_rows, target, rows, seg, seq, b, t, b * p, extra)
    got = float((ref['weight'] * (pred_rows - ref['ybar']) ** 2).sum() + ref['const'])
    assert abs(got - want) <= 1e-12 * abs(want)
    oracle = ref_cpu.mse(pred_frames.reshape(b, t, 1).astype(F32), target.reshape(b, t, 1), seq)
    assert abs(float(oracle) - want) <= 1e-5 * abs(want)
    _, _, loss, _ = R.phone_mse_rows(pred_rows.astype(F32), ref['ybar'].astype(F32), ref['weight'].astype(F32))
    assert abs(loss + ref['const'] - want) <= 1e-6 * abs(want)


def test_an_empty_utterance_that_owns_frames_gives_nan_as_the_oracle_does():
    b, p, t, extra = R.STATS_CASES[1]
    dur, target, seq = R.stats_case(b, p, t, extra, 'empty')
    rows, mapped, seg = R.stats_map(dur, t)
    ref = R.phone_target_stats(target, rows, seg, seq, b, t, b * p, extra)
    owns = (seg[1] - seg[0])[:p] > 0
    assert np.all(np.isnan(ref['weight'][:p][owns])) and np.all(ref['ybar'][:p] == 0) and np.isnan(ref['const'])
    assert np.all(ref['weight'][:p][~owns] == 0) and not np.any(np.isnan(ref['weight'][2 * p:b * p]))
    with np.errstate(all='ignore'):
        assert np.isnan(ref_cpu.mse(np.zeros((b, t, 1), dtype=F32), target.reshape(b, t, 1), seq))


def test_segment_bounds_reference_on_a_hand_made_map():
    rows = np.array([-1, 0, 0, 9, 2, 2, 2, -1], dtype=np.int32)
    seg, mapped = R.segment_bounds(rows, 4, 4)
    assert seg.tolist() == [[1, 0, 4, 0], [3, 0, 7, 0]] and mapped.tolist() == [4, 0, 0, 9, 2, 2, 2, 4]
    assert [s.tolist() for s in R.pad_shares(rows, 4, 3)] == [[0], [3], [7]]
    assert [s.tolist() for s in R.pad_shares(rows, 4, 12)] == [[0], [], [], [3], [], [], [], [7], [], [], [], []]
    for m in R.BOUNDS_M:
        for kind in R.BOUNDS_KINDS:
            r, n_rows = R.bounds_map(m, kind)
            assert r.size == m
            R.segment_bounds(r, n_rows)                                    # asserts consecutive runs


# ======================================================================================================= emulations within bounds
def _segsum_checks(case, bf16, fault=None):
    m, n, padded, extra, pad = case
    g, rows, n_rows, ldg, ldo = R.segsum_case(m, n, padded, extra, pad, bf16)
    seg, _ = R.segment_bounds(rows, n_rows)
    ref = R.segment_sum(g, rows, seg, n_rows, extra, n, ldo, bf16)
    got = emu_segment_sum(g, rows, seg, n_rows, extra, n, ldo, bf16, fault)
    name = 'segment_sum %s' % ('bf16' if bf16 else 'f32')
    exact = D.bits_equal_bf16(got, ref['bits']) if bf16 else D.bits_equal_f32(got, ref['exact'])
    value = D.bf16_to_f32(got) if bf16 else got
    return name, exact, value, ref


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('case', R.SEGSUM_CASES, ids=lambda c: 'M%d_N%d_%s_x%d_%s' % (c[0], c[1], 'ld' if c[2] else 'tight', c[3], c[4]))
def test_emulated_segment_sum_equals_the_replay(case, bf16):
    name, exact, value, ref = _segsum_checks(case, bf16)
    assert exact
    _record(name + ' sum', value, ref['sum'], ref['bound'])


@pytest.mark.parametrize('lengths', R.STATS_LENGTHS)
@pytest.mark.parametrize('case', R.STATS_CASES, ids=lambda c: 'B%d_P%d_T%d_x%d' % c)
def test_emulated_statistics_are_within_their_bounds(case, lengths):
    b, p, t, extra = case
    dur, target, seq = R.stats_case(b, p, t, extra, lengths)
    rows, mapped, seg = R.stats_map(dur, t)
    for front in ([False, True] if R.front_ok(b, p, t, extra) else [False]):
        ref = R.phone_target_stats(target, rows, seg, seq, b, t, b * p, extra, p, front)
        ybar, weight, partial = emu_stats(target, mapped, seg, seq, b, t, b * p, extra, front_p=p if front else None)
        name = 'front' if front else 'stats'
        _record(name + ' weight', weight, ref['weight'], ref['weight_bound'])
        _record(name + ' ybar', ybar, ref['ybar'], ref['ybar_bound'])
        _record(name + ' const', partial.astype(F64).sum(), ref['const'], ref['const_bound'])


@pytest.mark.parametrize('ldp', [1, 8])
@pytest.mark.parametrize('n', R.MSE_ROWS_N)
def test_emulated_row_loss_is_within_its_bounds(n, ldp):
    pred, ybar, weight = R.mse_rows_case(n, ldp)
    for with_nan in (True, False):
        w = weight.copy()
        if not with_nan and n >= 4:
            w[3] = F32(1.0 / n)
        want_d, bound_d, want_l, bound_l = R.phone_mse_rows(pred[:, 0], ybar, w)
        dpred, loss = emu_mse_rows(pred[:, 0], ybar, w)
        _record('phone_mse_rows dpred', dpred, want_d, bound_d)
        _record('phone_mse_rows loss', loss, want_l, bound_l)
        assert np.isnan(want_l) == (with_nan and n >= 4)
        assert np.all(want_d[w == 0] == 0)


@pytest.mark.parametrize('out_f32', [True, False], ids=['f32', 'bf16'])
@pytest.mark.parametrize('n', R.PCL_N)
def test_emulated_concat_layer_is_within_its_bound(n, out_f32):
    name = 'phone_concat_layer %s' % ('f32' if out_f32 else 'bf16')
    for c, m in R.PCL_CM:
        p, rows, feat, w, bias = R.concat_case(m, n, c)
        for act in (R.ACT_NONE, R.ACT_SIGMOID, R.ACT_TANH, R.ACT_RELU):
            want, bound = R.phone_concat_layer(p, rows, feat, w, 600, bias, n, act, R.pad8(n) + 8, out_f32)
            for sign in ((1.0, -1.0) if act == R.ACT_SIGMOID else (1.0,)):
                _record(name, emu_concat(p, rows, feat, w, 600, bias, n, act, R.pad8(n) + 8, out_f32, sign=sign), want, bound)
        want, bound = R.phone_concat_layer(p, rows, feat, w, 600, None, n, R.ACT_SIGMOID, R.pad8(n), out_f32)
        _record(name, emu_concat(p, rows, feat, w, 600, None, n, R.ACT_SIGMOID, R.pad8(n), out_f32), want, bound)


def test_the_concat_map_has_the_edges_the_case_grid_names():
    rows = R.concat_map(100)
    assert rows[15] != rows[16] and rows[20] != rows[21] and len(set(rows[30:70])) == 1 and rows[29] != rows[30] != rows[70]
    assert (rows == R.PCL_TABLE_ROWS - 1).any() and rows.max() < R.PCL_TABLE_ROWS


@pytest.mark.parametrize('case', R.FEAT_CASES, ids=lambda c: 'R%d_x%d_N%d_C%d_col%d_%s' % (c[:5] + ('acc' if c[5] else 'set',)))
def test_emulated_feat_wgrad_is_within_its_bound(case):
    n_rows, extra, n, c, col0, accumulate = case
    if n_rows > 3 and n > 8:
        n = 16                                                             # the emulation's cost is its columns; the row ranges are the case
    g, rows, feat, prior = R.feat_case(n_rows, extra, n, c, col0, accumulate)
    seg, _ = R.segment_bounds(rows, n_rows)
    want, bound, depth = R.feat_wgrad(g, feat, rows, seg, n_rows, extra, n, prior[:n] if accumulate else None, col0)
    got = emu_feat_wgrad(g, feat, rows, seg, n_rows, extra, n, prior[:n], col0, accumulate)
    _record('feat_wgrad dW', got, want, bound)
    per = -(-(n_rows + extra) // 2048)
    assert per == {R.SEG130_ROWS + 5: 1, 5: 1, 2048: 1, 2049: 2, 4500: 3}[n_rows + extra] and depth >= 8 + 64 + 3 + 1
    ref = R.segment_sum(g, rows, seg, n_rows, extra, n, n, True)
    assert D.bits_equal_bf16(emu_segment_sum(g, rows, seg, n_rows, extra, n, n, True), ref['bits'])


@pytest.mark.parametrize('slots', R.PARTIAL_SLOTS, ids=lambda s: '%dslots' % R.n_partials(*s))
def test_the_constants_replay_is_a_float32_sum_of_the_slots(slots):
    _, _, partial, loss = R.expand_case(257, *slots)
    assert partial.size == R.n_partials(*slots)
    got = float(R.loss_const_add(partial, loss))
    want = float(loss) + partial.astype(F64).sum()
    assert abs(got - want) <= (partial.size // 256 + 10) * U * want


# =========================================================================================================== the planted faults
def test_faults_of_the_segment_sums_are_caught():
    for fault, case, bf16 in (('remainder frames of a 5-frame phone dropped', R.SEGSUM_CASES[0], False),
                              ('pad frame on a share edge credited to the other share', R.SEGSUM_CASES[5], False),
                              ('truncation instead of round-to-nearest-even', R.SEGSUM_CASES[0], True),
                              ('nonzero columns past N', R.SEGSUM_CASES[1], True)):
        name, exact, value, ref = _segsum_checks(case, bf16, fault)
        failed = ([name + ' exact'] if not exact else []) + ([name + ' sum'] if _fails(name + ' sum', value, ref['sum'], ref['bound']) else [])
        assert len(failed) == 2, (fault, failed)                          # bits and float64 side: a wrong term fails both
        _caught(fault, failed)


def test_faults_of_the_statistics_are_caught():
    for fault in ('mask edge as <=', 'weight over B T', 'ybar over masked frames too', 'extra rows left out of the constant'):
        failed = []
        lengths = 'over' if fault.startswith('extra rows') else 'cut'      # the pad frames' terms are nonzero only below seq_len
        for case in R.STATS_CASES:
            b, p, t, extra = case
            dur, target, seq = R.stats_case(b, p, t, extra, lengths)
            rows, mapped, seg = R.stats_map(dur, t)
            ref = R.phone_target_stats(target, rows, seg, seq, b, t, b * p, extra)
            ybar, weight, partial = emu_stats(target, mapped, seg, seq, b, t, b * p, extra, fault)
            for name, got, key in (('weight', weight, 'weight'), ('ybar', ybar, 'ybar'), ('const', partial.astype(F64).sum(), 'const')):
                if _fails('stats ' + name, got, ref[key], ref[key + '_bound']):
                    failed.append('stats ' + name)
        _caught(fault, failed)


def test_faults_of_the_row_loss_and_the_constant_are_caught():
    pred, ybar, weight = R.mse_rows_case(1025, 1)
    weight[3] = F32(1.0 / 1025)
    want_d, bound_d, want_l, bound_l = R.phone_mse_rows(pred[:, 0], ybar, weight)
    dpred, loss = emu_mse_rows(pred[:, 0], ybar, weight, 'row 1024 dropped from the row loss')
    _caught('row 1024 dropped from the row loss', [name for name, bad in (('phone_mse_rows dpred', _fails('phone_mse_rows dpred', dpred, want_d, bound_d)),
                                                                         ('phone_mse_rows loss', _fails('phone_mse_rows loss', loss, want_l, bound_l))) if bad])
    for slots in R.PARTIAL_SLOTS:
        _, _, partial, loss = R.expand_case(257, *slots)
        if not D.bits_equal_f32([R.loss_const_add(partial[:-1], loss)], [R.loss_const_add(partial, loss)]):
            _caught('last partial slot dropped', ['loss constant exact (%d slots)' % partial.size])


def test_faults_of_the_concat_layer_are_caught():
    for fault in ('P kept from the previous chunk', 'two counter columns swapped', 'bias missing on pad frames'):
        failed = []
        for out_f32 in (True, False):
            p, rows, feat, w, bias = R.concat_case(100, 20, 9)
            want, bound = R.phone_concat_layer(p, rows, feat, w, 600, bias, 20, R.ACT_SIGMOID, 24, out_f32)
            name = 'phone_concat_layer %s' % ('f32' if out_f32 else 'bf16')
            if _fails(name, emu_concat(p, rows, feat, w, 600, bias, 20, R.ACT_SIGMOID, 24, out_f32, fault), want, bound):
                failed.append(name)
        _caught(fault, failed)


def test_faults_of_the_feature_gradient_are_caught():
    n_rows, extra, n, c, col0, accumulate = [k for k in R.FEAT_CASES if k[0] + k[1] == 2048 and k[5]][0]
    g, rows, feat, prior = R.feat_case(n_rows, extra, n, c, col0, accumulate)
    seg, _ = R.segment_bounds(rows, n_rows)
    assert sum(fr.size for fr in R.row_frames(rows, seg, n_rows, extra)[252 * 8:]) > 0
    want, bound, _ = R.feat_wgrad(g, feat, rows, seg, n_rows, extra, n, prior[:n], col0)
    got = emu_feat_wgrad(g, feat, rows, seg, n_rows, extra, n, prior[:n], col0, True, 'slabs 252 to 255 dropped')
    _caught('slabs 252 to 255 dropped', ['feat_wgrad dW'] if _fails('feat_wgrad dW', got, want, bound) else [])


def test_a_wrong_order_fails_the_exact_check_alone_and_a_wrong_term_fails_both():
    g, rows, n_rows, _, ldo = R.segsum_case(130, 72, False, 5, 'minus1', False)
    seg, _ = R.segment_bounds(rows, n_rows)
    ref = R.segment_sum(g, rows, seg, n_rows, 5, 72, ldo)
    frames = R.row_frames(rows, seg, n_rows, 5)
    other_order = np.stack([D._serial_sum_f32(g[fr[::-1]]) if fr.size else np.zeros(72, dtype=F32) for fr in frames])     # descending frames
    assert not D.bits_equal_f32(other_order, ref['exact'])
    assert not _fails('segment_sum f32 sum', other_order, ref['sum'], ref['bound'])
    wrong_term = np.stack([D._serial_sum_f32(g[fr[:-1]]) if fr.size else np.zeros(72, dtype=F32) for fr in frames])        # the last frame dropped
    assert not D.bits_equal_f32(wrong_term, ref['exact'])
    assert _fails('segment_sum f32 sum', wrong_term, ref['sum'], ref['bound'])


# ------------------------------------------------------------------------------------------------------------- the two tables
def test_zz_every_fault_is_caught_and_no_emulation_crowds_its_bound():
    """Runs last in this file (pytest keeps file order): prints the fault table and the worst emulation ratio per check."""
    if len(CAUGHT) < len(FAULTS):                            # selected alone: run the fault tests here
        for fn in (test_faults_of_the_segment_sums_are_caught, test_faults_of_the_statistics_are_caught,
                   test_faults_of_the_row_loss_and_the_constant_are_caught, test_faults_of_the_concat_layer_are_caught,
                   test_faults_of_the_feature_gradient_are_caught):
            fn()
    print('\nfault -> checks that caught it')
    for fault in FAULTS:
        print('  %-58s %s' % (fault, ', '.join(CAUGHT.get(fault, [])) or 'NOT CAUGHT'))
    print('check -> worst emulation error / bound')
    for check in sorted(RATIOS):
        print('  %-28s %.3f (ceiling %.1f)' % (check, RATIOS[check], R.ratio_ceiling(check)))
    assert [f for f in FAULTS if not CAUGHT.get(f)] == []
    assert {f: sorted(c) for f, c in CAUGHT.items()} == {f: sorted(c) for f, c in FAULT_TABLE.items()}      # the table of DESIGN.md 4.31
    assert [c for c in RATIOS if RATIOS[c] > R.ratio_ceiling(c)] == []
