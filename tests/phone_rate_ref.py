"""References of the phone-rate segment kernels (csrc/phone_rate.hip, csrc/phone_front.h), in the two families of tests/datapath_ref.py.
Plain numpy; no torch, no import of the package.

EXACT family - the device equals the replay bit for bit: segment_bounds (np.flatnonzero on the map), segment_sum and the `sums` of
segment_sum_feat (float32 additions in ascending frame order from zero, bf16 by round-to-nearest-even on the bit pattern),
expand_column (table[rows]) and the constant added by expand_column_loss / phone_loss_const_add (256 strided sums, the halving tree,
one last addition).  Only additions are involved, so no fused multiply-add can change a bit.  segment_sum also returns the float64 sum
and an n U sum|terms| bound: a wrong ORDER fails the exact check alone, a wrong TERM fails both.

BOUNDED family - float64 from the float32 / bf16 inputs and a first-order bound of U = 2^-24 per float32 operation (the UNFUSED count
where hipcc may contract), ETA where a result can underflow.  A reduction is charged DEPTH U sum|terms| with DEPTH counted from the
kernel; the count of each result stands in its function's docstring and in DESIGN.md 4.31.  phone_target_stats / phone_front (weight,
ybar, the constant), phone_mse_rows, phone_concat_layer, feat_wgrad_reduce behind segment_sum_feat.

`ratio_ceiling`: 1.0 for the element-wise checks, 0.5 for every reduction (datapath_ref says why they differ)."""
import numpy as np

import linear_ref64 as L
from datapath_ref import ETA, F32, F64, U, _serial_sum_f32, bf16_bits, bf16_to_f32, upsample_index_maps

ACT_NONE, ACT_SIGMOID, ACT_TANH, ACT_RELU = L.ACT_NONE, L.ACT_SIGMOID, L.ACT_TANH, L.ACT_RELU
SSF_WAVES, SSF_BLOCKS = 8, 256          # segment_sum_feat_kernel: waves per workgroup, workgroups (= slabs)
PCL_CHUNK = 16                          # phone_concat_layer_kernel: consecutive frames per wave and trip

ELEMENTWISE_CHECKS = frozenset(['segment_sum f32 sum', 'segment_sum bf16 sum', 'segment_sum_feat sum', 'phone_mse_rows dpred',
                                'phone_concat_layer f32', 'phone_concat_layer bf16'])
REDUCTION_CHECKS = frozenset(['stats weight', 'stats ybar', 'stats const', 'front weight', 'front ybar', 'front const',
                              'phone_mse_rows loss', 'feat_wgrad dW'])


def ratio_ceiling(check):
    """1.0 for an element-wise check, 0.5 for a reduction.  The float64 side of a segment sum counts as element-wise, as
    upsample_backward's does: a phone of n <= 3 frames has n - 1 roundings and is charged n."""
    assert check in ELEMENTWISE_CHECKS or check in REDUCTION_CHECKS, check
    return 1.0 if check in ELEMENTWISE_CHECKS else 0.5


def pad8(n):
    return (n + 7) // 8 * 8


# ================================================================================================================ segment_bounds
def segment_bounds(rows, n_rows, pad_row=-1):
    """(seg (2, R) int32, rows_mapped): the run [first, last + 1) of the frames whose id is r, (0, 0) for a row without frames; ids
    >= R own no run; rows_mapped = rows with every negative id replaced by pad_row (ids >= R stay)."""
    rows = np.asarray(rows, dtype=np.int32).reshape(-1)
    seg = np.zeros((2, int(n_rows)), dtype=np.int32)
    for r in range(int(n_rows)):
        at = np.flatnonzero(rows == r)
        if at.size:
            assert at[-1] - at[0] + 1 == at.size, 'the frames of row %d are not consecutive' % r
            seg[0, r], seg[1, r] = at[0], at[-1] + 1
    return seg, np.where(rows < 0, np.int32(pad_row), rows).astype(np.int32)


def pad_shares(rows, n_rows, extra):
    """[frame ids] per extra row j: the pad frames (id < 0 or >= R) of [j chunk, min((j + 1) chunk, M)), ascending,
    chunk = ceil(M / extra)."""
    rows = np.asarray(rows).reshape(-1)
    m = rows.size
    pad = (rows < 0) | (rows >= n_rows)
    if extra == 0:
        return []
    chunk = -(-m // extra)
    return [np.arange(min(j * chunk, m), min((j + 1) * chunk, m))[pad[min(j * chunk, m):min((j + 1) * chunk, m)]] for j in range(extra)]


def row_frames(rows, seg, n_rows, extra):
    """[frame ids] per table row, the R phone rows and then the extra rows."""
    return [np.arange(seg[0, r], seg[1, r]) for r in range(n_rows)] + pad_shares(rows, n_rows, extra)


# =================================================================================================================== segment_sum
def segment_sum(g, rows, seg, n_rows, extra, n, ldo, bf16=False):
    """g (M, ldg) float32 (for bf16: the float32 values of the bf16 input).  Row r: the frames of its run added per column in
    ascending frame order from a float32 zero - the kernel's (((acc + t0) + t1) + t2) + t3 and its remainder loop are that order;
    extra row j: the pad frames of its share, ascending.  Columns n .. ldo - 1 zero.
    Returns {'exact' float32 (R + extra, ldo), 'bits' uint16 (bf16 only), 'sum' float64, 'bound'}: bound = k U sum|terms| for a row
    of k frames (k - 1 roundings); for bf16 the store adds 2^-8 (|sum| + bound), half a spacing of 8 significant bits."""
    g = np.asarray(g, dtype=F32)
    frames = row_frames(rows, seg, n_rows, extra)
    exact = np.zeros((n_rows + extra, ldo), dtype=F32)
    total = np.zeros((n_rows + extra, ldo), dtype=F64)
    bound = np.zeros((n_rows + extra, ldo), dtype=F64)
    for r, fr in enumerate(frames):
        if fr.size:
            run = g[fr, :n]
            exact[r, :n] = _serial_sum_f32(run)
            total[r, :n] = run.astype(F64).sum(axis=0)
            bound[r, :n] = fr.size * U * np.abs(run.astype(F64)).sum(axis=0)
    out = {'exact': exact, 'sum': total, 'bound': bound}
    if bf16:
        out['bits'] = bf16_bits(exact)
        out['bound'] = bound + 2.0 ** -8 * (np.abs(total) + bound)
    return out


# ============================================================================================================ feat_wgrad_reduce
def feat_wgrad(g, feat, rows, seg, n_rows, extra, n, prior=None, col0=0):
    """dW[:, col0 : col0 + C] = sum over ALL frames of g[f, :n]^T feat[f, :], pad frames included (they lie in the extra rows' shares;
    needs extra > 0), + the prior contents with accumulate.  g: the float32 values of the bf16 gradient.
    DEPTH, the longest chain of additions a product passes through: the frames of one wave's row range (the wave keeps ONE
    accumulator per (c, column) over all its rows), the 8 waves of a workgroup in wave order, the 64 slabs of one of the reduce's
    four partitions, the 3 additions of the partitions; one more with accumulate, which also rounds the prior: + U |prior|.  The
    kernel accumulates with an explicit fmaf, so a product has no rounding of its own and none is charged.
    Returns (dW float64 (n, ldw) - prior or zeros outside the C columns -, bound, depth)."""
    g64 = np.asarray(g, dtype=F32).astype(F64)[:, :n]
    f64 = np.asarray(feat, dtype=F32).astype(F64)
    c = f64.shape[1]
    frames = row_frames(rows, seg, n_rows, extra)
    covered = np.sort(np.concatenate(frames)) if frames else np.zeros(0, dtype=np.int64)
    assert np.array_equal(covered, np.arange(g64.shape[0])), 'every frame must lie in a run or in a share'
    per = -(-(n_rows + extra) // (SSF_BLOCKS * SSF_WAVES))
    counts = np.array([fr.size for fr in frames])
    wave_frames = max(int(counts[w * per:(w + 1) * per].sum()) for w in range(-(-(n_rows + extra) // per)))
    depth = wave_frames + SSF_WAVES + SSF_BLOCKS // 4 + 3 + (1 if prior is not None else 0)
    val = g64.T @ f64
    mag = np.abs(g64).T @ np.abs(f64)
    if prior is None:
        return val, depth * U * mag + ETA, depth
    dw = np.asarray(prior, dtype=F32).astype(F64).copy()
    bound = np.zeros_like(dw)
    bound[:, col0:col0 + c] = depth * U * mag + U * np.abs(dw[:, col0:col0 + c]) + ETA
    dw[:, col0:col0 + c] += val
    return dw, bound, depth


# ============================================================================================================ phone_concat_layer
def phone_concat_layer(p, rows, feat, w, col0, bias, n, act, ldy, out_f32):
    """Y[f, e] = act(P[rows[f], e] + b[e] + sum_c feat[f, c] W[e, col0 + c]), e < n, the counters in ascending c; columns n .. ldy - 1
    exactly zero.  Roundings of the pre-activation z: one for P + b (none without a bias), then ONE per counter - the kernel adds
    each with an explicit fmaf, which hipcc cannot split, so the product has no rounding of its own and charging one would only hide
    a missed one: U |P + b| + sum_c U |s_c| + C ETA with s_c the partial sums.  Then the activation's own charge from linear_ref64 (mg_sigmoid_fast: b_sigmoid(fast=True); tanhf: b_tanh; ReLU exact, zero
    where every value within the bound is negative) and its store rule for a bf16 output.  Returns (value (M, ldy), bound)."""
    rows = np.asarray(rows).reshape(-1)
    x = np.asarray(feat, dtype=F32).astype(F64)
    wc = np.asarray(w, dtype=F32).astype(F64)[:n, col0:col0 + x.shape[1]]
    z = np.asarray(p, dtype=F32).astype(F64)[rows, :n]
    e = np.zeros_like(z)
    if bias is not None:
        z = z + np.asarray(bias, dtype=F32).astype(F64)[:n]
        e = U * np.abs(z)
    for c in range(x.shape[1]):
        t = x[:, c:c + 1] * wc[None, :, c]
        z = z + t
        e = e + U * np.abs(z) + ETA
    b = L.Bounded(z, e)
    if act == ACT_SIGMOID:
        b = L.b_sigmoid(b, fast=True)
    elif act == ACT_TANH:
        b = L.b_tanh(b)
    elif act == ACT_RELU:
        b = L.Bounded(np.where(b.v < 0, 0.0, b.v), np.where(b.v + b.e < 0, 0.0, b.e))
    b, _ = L._store(b, out_f32)
    val, bound = np.zeros((rows.size, ldy), dtype=F64), np.zeros((rows.size, ldy), dtype=F64)
    val[:, :n], bound[:, :n] = b.v, b.e
    return val, bound


# ============================================================================================= phone_target_stats / phone_front
def valid_frames(seq_len, b, t):
    if seq_len is None:
        return np.full(b, t, dtype=np.int64)
    return np.clip(np.asarray(seq_len, dtype=np.int64).reshape(-1), 0, t)


def frame_weights(seq_len, b, t):
    """(B t,) float64: [t' < n_b] / (n_b B); every frame of an utterance with n_b = 0 is NaN (0 * inf)."""
    nb = valid_frames(seq_len, b, t).astype(F64)
    with np.errstate(all='ignore'):
        w = (np.arange(t)[None, :] < nb[:, None]).astype(F64) * (1.0 / (nb[:, None] * b))
    return w.reshape(-1)


def stats_depths(rows, seg, n_rows, extra, b, p=None, front=False):
    """(depth of weight / ybar per table row, depth of the constant).  A phone row of k frames: ceil(k / 16) additions per lane and 4
    butterfly levels; an extra row with a share of `chunk` frames: ceil(chunk / 64) per lane and 6 levels.  The constant,
    phone_target_stats_kernel: a thread's own row, then the 8 levels of the 256-thread tree (the slots are summed in float64 by the
    test).  phone_front_kernel: a thread adds its phones of ceil(P / 16) passes, or wave 0 the four extra rows of its job, then 6
    levels of the wave sum and 4 additions over the waves."""
    m = np.asarray(rows).size
    counts = (seg[1] - seg[0]).astype(np.int64)
    chunk = -(-m // extra) if extra else 0
    lane = np.concatenate([-(-counts // 16) + 4, np.full(extra, -(-chunk // 64) + 6, dtype=np.int64)])
    kmax = int(-(-counts.max() // 16)) if counts.size else 0
    if front:
        const = max(-(-p // 16) * kmax, 4 * -(-chunk // 64)) + 6 + 4
    else:
        const = max(kmax, -(-chunk // 64)) + 8
    return lane, const


def phone_target_stats(target, rows, seg, seq_len, b, t, n_rows, extra, p=None, front=False):
    """Per table row r (the R phone rows, then the extra rows with the pad frames of their shares), w_f = frame_weights:
        weight[r] = sum_f w_f                        w_f: the product n_b B and the division, 2U; DEPTH_r additions:
                                                     (2 + DEPTH_r) U weight
        ybar[r]   = sum_f w_f y_f / weight[r]        the products 3U, the sum DEPTH_r U, over the weight: (3 + DEPTH_r) U sum|w y| / W;
                    0 where weight is not > 0        the weight's own error and the division: (3 + DEPTH_r) U |ybar|;  + ETA
        const     = sum_r sum_f w_f (y_f - ybar[r])^2   per term: w 2U, the difference U twice, two products: 6U |term|, the device's
                                                     own ybar 2 w |y - ybar| dybar, then DEPTH_c U |term|
    A row that owns a frame of an utterance with n_b = 0 has a NaN weight (ybar 0) and makes the constant NaN.
    Returns dict weight, weight_bound, ybar, ybar_bound (R + extra,), const, const_bound."""
    y = np.asarray(target, dtype=F32).astype(F64).reshape(-1)
    w = frame_weights(seq_len, b, t)
    frames = row_frames(rows, seg, n_rows, extra)
    lane, depth_c = stats_depths(rows, seg, n_rows, extra, b, p, front)
    nr = n_rows + extra
    weight, wb, ybar, yb = np.zeros(nr), np.zeros(nr), np.zeros(nr), np.zeros(nr)
    const = const_bound = 0.0
    for r, fr in enumerate(frames):
        if not fr.size:
            continue
        wf, yf, d = w[fr], y[fr], float(lane[r])
        weight[r] = wf.sum()
        if not weight[r] > 0:                                       # 0, or NaN: the guard leaves ybar 0
            const += float((wf * yf * yf).sum())
            continue
        wb[r] = (2 + d) * U * weight[r]
        ybar[r] = (wf * yf).sum() / weight[r]
        yb[r] = (3 + d) * U * np.abs(wf * yf).sum() / weight[r] + (3 + d) * U * abs(ybar[r]) + ETA
        term = wf * (yf - ybar[r]) ** 2
        const += float(term.sum())
        const_bound += float(((6 + depth_c) * U * term + 2 * wf * np.abs(yf - ybar[r]) * yb[r]).sum())
    return {'weight': weight, 'weight_bound': wb, 'ybar': ybar, 'ybar_bound': yb, 'const': const, 'const_bound': const_bound + ETA}


def frame_loss(pred_rows, target, rows, seg, seq_len, b, t, n_rows, extra):
    """The masked MSE over the frames (D = 1) of a prediction that is constant per table row, in float64: sum_f w_f (p_row(f) - y_f)^2."""
    y = np.asarray(target, dtype=F32).astype(F64).reshape(-1)
    w = frame_weights(seq_len, b, t)
    pr = np.zeros(y.size)
    for r, fr in enumerate(row_frames(rows, seg, n_rows, extra)):
        pr[fr] = pred_rows[r]
    return float((w * (pr - y) ** 2).sum()), pr


# ================================================================================================================ phone_mse_rows
def phone_mse_rows(pred, ybar, weight):
    """d_r = pred[r] - ybar[r] where weight[r] > 0, else 0;  dpred[r] = 2 w d (so 0 for a zero weight whatever the prediction holds, NaN
    for a NaN weight: 0 * NaN, the NaN of the reference's 0 * inf);  loss = sum_r (w d) d.
    THIS DEPARTS FROM THE WORDING OF THE ISSUE that asked for this reference, "dpred = 0 where w is not > 0": taken literally a NaN
    weight would give dpred = 0.  The kernel's guard zeroes d, not the product, and the NaN it leaves is what the reference
    project's gradient holds for every frame of an empty utterance, so the NaN is what is asserted here - in that row alone.
    dpred: the difference and the product (2 w is exact): 2U |dpred| + ETA.  loss: the difference twice and the float32 product w d:
    3U per term; the products with d and the sum over n rows are in float64 on the device: 2^-53 (n + 11) sum|terms|; the result is
    stored as float32: U |loss|.  Returns (dpred, dpred_bound, loss, loss_bound)."""
    p, yb, w = (np.asarray(a, dtype=F32).astype(F64).reshape(-1) for a in (pred, ybar, weight))
    with np.errstate(all='ignore'):
        d = np.where(w > 0, p - yb, 0.0)
        dpred = 2.0 * w * d
        term = w * d * d
    loss = float(term.sum())
    mag = float(np.abs(term[~np.isnan(term)]).sum())
    return dpred, 2 * U * np.abs(np.nan_to_num(dpred)) + ETA, loss, 3 * U * mag + 2.0 ** -53 * (p.size + 11) * mag + U * abs(np.nan_to_num(loss)) + ETA


# ================================================================================================== expand_column, the constant
def expand_column(table, rows):
    return np.asarray(table, dtype=F32).reshape(-1)[np.asarray(rows).reshape(-1)]


def tree256_f32(v):
    v = np.array(v, dtype=F32)
    s = 128
    while s > 0:
        v[:s] = (v[:s] + v[s:2 * s]).astype(F32)
        s >>= 1
    return v[0]


def loss_const_sum(partial):
    """Thread i adds partial[i], partial[i + 256], ... from a float32 zero; then the 256-entry halving tree."""
    partial = np.asarray(partial, dtype=F32).reshape(-1)
    v = np.zeros(256, dtype=F32)
    for i in range(min(256, partial.size)):
        v[i] = _serial_sum_f32(partial[i::256])
    return tree256_f32(v)


def loss_const_add(partial, loss=None):
    """loss + loss_const_sum(partial) in float32; without `loss` the sum alone (mg_phone_target_stats' loss_const output)."""
    s = loss_const_sum(partial)
    return s if loss is None else F32(F32(loss) + s)


def n_partials(n_rows, extra):
    return -(-n_rows // 16) + -(-extra // 4)


# ================================================================================================ the inputs the tests share
# Each generator is seeded by its arguments alone, so the host test and the GPU test see the same data.
SEG_LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 21)


def segment_map(m, pad='minus1'):
    """(rows (m,) int32, R): frame 0 a pad frame; then phones of SEG_LENGTHS frames in that order, again and again, with two or three
    pad frames behind every phone of 1 frame and one or two behind every phone of 5; cut at m frames, the last frame a pad frame
    (m > 1); two more rows behind the last phone own no frame.  With m = 130 frames 24 .. 61 hold the phones of 8, 9 and 21 frames
    and no pad frame.  pad: 'minus1', or 'mapped' = the id R."""
    ids, r, k = [-1], 0, 0
    while len(ids) < m:
        ids += [r] * SEG_LENGTHS[k % 9]
        r += 1
        if k % 9 == 1:
            ids += [-1] * (2 + (k // 9) % 2)
        elif k % 9 == 4:
            ids += [-1] * (1 + (k // 9) % 2)
        k += 1
    ids = ids[:m]
    if m > 1:
        ids[-1] = -1
    rows = np.array(ids, dtype=np.int32)
    n_rows = r + 2
    if pad == 'mapped':
        rows[rows < 0] = n_rows
    return rows, n_rows


BOUNDS_M = (1, 255, 256, 257, 700)
BOUNDS_KINDS = ('runs', 'big_ids', 'all_pad')


def bounds_map(m, kind):
    """(rows (m,) int32, R).  'runs': frame 0 and the last frame pad frames (-1), runs of 1, 3, 4, 5, 7, 2 frames in turn with a pad
    frame behind every fourth, one run cut so that it ends on frame 255 and the next starts on frame 256; the last row owns no
    frame.  'big_ids': the same with every other pad frame as an id >= R.  'all_pad': -1 everywhere."""
    if kind == 'all_pad':
        return np.full(m, -1, dtype=np.int32), 3
    ids, r, k = [-1], 0, 0
    while len(ids) < m:
        n = (1, 3, 4, 5, 7, 2)[k % 6]
        if len(ids) < 256 < len(ids) + n:
            n = 256 - len(ids)
        ids += [r] * n
        r, k = r + 1, k + 1
        if k % 4 == 0 and len(ids) != 256:
            ids.append(-1)
    ids = ids[:m]
    if m > 1:
        ids[-1] = -1
    rows = np.array(ids, dtype=np.int32)
    n_rows = r + 1
    if kind == 'big_ids':
        pads = np.flatnonzero(rows < 0)
        rows[pads[::2]] = n_rows + 5
    return rows, n_rows


# (M, N, padded leading dimensions (ldg = N + 16, ldo = N + 8), extra, pad)
SEGSUM_CASES = ((130, 8, False, 5, 'minus1'), (130, 72, True, 1, 'mapped'), (130, 512, False, 5, 'mapped'), (130, 520, True, 5, 'minus1'),
                (130, 520, False, 0, 'minus1'), (7, 8, False, 3, 'minus1'), (7, 72, True, 12, 'mapped'), (63, 8, True, 1, 'minus1'),
                (64, 8, False, 1, 'mapped'), (65, 72, False, 1, 'minus1'), (63, 72, False, 0, 'mapped'))


def segsum_case(m, n, padded, extra, pad, bf16, seed=20261101):
    """(g float32 (M, ldg) - bf16 values for bf16, the padding columns NOT zero -, rows, R, ldg, ldo)."""
    rng = np.random.RandomState(seed + 3 * m + n + extra + (500 if bf16 else 0))
    rows, n_rows = segment_map(m, pad)
    ldg, ldo = (n + 16, n + 8) if padded else (n, n)
    g = rng.standard_normal((m, ldg)).astype(F32)
    if bf16:
        g = bf16_to_f32(bf16_bits(g))
    return g, rows, n_rows, ldg, ldo


def feat_map(n_rows, extra, seed=20261102):
    """(rows (M,) int32 with pad frames mapped to R): phone rows of 0 to 3 frames (5, 0 and 3 for R = 3), a run of 1 to 2 pad frames
    behind every seventh row, one at the very start and one at the very end.  R = SEG130_ROWS: segment_map(130), the phones of 0, 1,
    3, 4, 5, 7, 8, 9 and 21 frames that segment_sum is held to."""
    if n_rows == SEG130_ROWS:
        return segment_map(130, 'mapped')[0]
    rng = np.random.RandomState(seed + n_rows + extra)
    lens = np.array([5, 0, 3]) if n_rows == 3 else rng.randint(0, 4, size=n_rows)
    ids = [n_rows]
    for r in range(n_rows):
        ids += [r] * int(lens[r])
        if r % 7 == 6:
            ids += [n_rows] * (1 + r % 2)
    ids.append(n_rows)
    return np.array(ids, dtype=np.int32)


SEG130_ROWS = segment_map(130)[1]

# (R, extra, N, C, col0, accumulate): R + extra = 5 (most waves idle), 2048 (one row per wave), 2049 and 4500 (2 and 3, the last wave
# short; with R = 2001 wave 1000 crosses from the phone rows into the extra rows); segment_map(130) with five shares, one of them empty
FEAT_CASES = ((SEG130_ROWS, 5, 72, 9, 600, True), (SEG130_ROWS, 5, 8, 16, 0, False), (3, 2, 8, 1, 0, False), (3, 2, 104, 9, 600, True), (3, 2, 520, 16, 0, True), (3, 2, 520, 9, 600, False),
              (2000, 48, 8, 9, 600, True), (2000, 48, 104, 16, 0, False), (2001, 48, 8, 16, 0, True), (2001, 48, 8, 1, 600, False),
              (4400, 100, 8, 9, 600, False), (4400, 100, 104, 1, 0, True))


def feat_case(n_rows, extra, n, c, col0, accumulate, seed=20261103):
    """(g float32 of bf16 values (M, N), rows, feat (M, C), prior dW (N, 600 + 16 + 3) - not a constant)."""
    rows = feat_map(n_rows, extra)
    rng = np.random.RandomState(seed + n_rows + 7 * n + c + col0)
    m = rows.size
    g = bf16_to_f32(bf16_bits(rng.standard_normal((m, n)).astype(F32)))
    feat = rng.uniform(0, 1, (m, c)).astype(F32)
    prior = rng.standard_normal((n, 619)).astype(F32)
    return g, rows, feat, prior


PCL_N = (1, 20, 250, 256, 257, 512, 520)
PCL_CM = ((1, 100), (9, 17), (16, 100), (9, 1), (16, 15), (1, 16))          # (C, M)
PCL_TABLE_ROWS = 12


def concat_map(m):
    """Table rows per frame, 0 .. 11, row 11 the pad row: frames 0 .. 15 one row (the change falls exactly on the chunk edge), then a
    row of 5 frames and a change inside the chunk, pad frames, one row spanning three chunks (frames 30 .. 69), then runs of 1 to 7."""
    ids = [0] * 16 + [1] * 5 + [2] * 6 + [11] * 3 + [3] * 40
    r, k = 4, 0
    while len(ids) < m:
        ids += [r % 11 if k % 5 else 11] * (1 + (3 * k) % 7)
        r, k = r + 1, k + 1
    return np.array(ids[:m], dtype=np.int32)


def concat_case(m, n, c, seed=20261104):
    """(P (12, pad8(n) + 8) float32, rows, feat (m, C), W (n, 600 + C + 2), bias (n,)); col0 = 600.  The columns of P beyond n hold
    values, not zeros: the kernel must not let them through."""
    rng = np.random.RandomState(seed + 5 * (m % 1000) + 11 * n + c)
    p = rng.standard_normal((PCL_TABLE_ROWS, pad8(n) + 8)).astype(F32) * F32(1.5)
    feat = rng.uniform(0, 1, (m, c)).astype(F32)
    w = rng.uniform(-0.5, 0.5, (n, 600 + c + 2)).astype(F32)
    bias = rng.uniform(-0.5, 0.5, n).astype(F32)
    return p, concat_map(m), feat, w, bias


STATS_DURS = (0, 1, 15, 16, 17, 40, 3, 2)
# (B, P, T, extra): R = B P in 1, 15, 16, 17, 100 (and 96, which phone_front takes with two utterances)
STATS_CASES = ((1, 1, 24, 1), (3, 5, 60, 3), (2, 8, 100, 4), (1, 17, 150, 5), (4, 25, 300, 8), (2, 48, 520, 5))
STATS_LENGTHS = ('none', 'cut', 'over', 'empty')


def stats_case(b, p, t, extra, lengths, seed=20261105):
    """(dur (B, P) int64, target (B t,), seq_len or None).  Durations: STATS_DURS in turn, shifted per utterance (17 for R = 1); an
    utterance whose phones overrun t is cut, one that ends before t has pad frames.  lengths: 'none'; 'cut' - in turn inside a
    phone, on a phone's edge, and before most phones (4); 'over' - above t, or two frames behind the last phone (pad frames
    inside seq_len); 'empty' - utterance 0 has 0 (it owns frames: NaN), utterance 1 a negative length, the others are cut."""
    rng = np.random.RandomState(seed + 13 * b + p + t)
    dur = np.array([[STATS_DURS[(i + 3 * u) % 8] for i in range(p)] for u in range(b)], dtype=np.int64)
    if b * p == 1:
        dur[0, 0] = 17
    target = rng.standard_normal(b * t).astype(F32)
    if lengths == 'none':
        return dur, target, None
    cum = np.minimum(np.cumsum(dur, axis=1), t)
    total = cum[:, -1]
    seq = np.zeros(b, dtype=np.int64)
    for u in range(b):
        big = int(np.argmax(dur[u]))                                       # the longest phone of the utterance
        inside = max(int(cum[u, big]) - max(int(dur[u, big]) // 2, 1), 1)
        edge = max(int(cum[u, big]), 1)
        cut = (inside, edge, 4)[u % 3] if lengths != 'over' else (t + 5 if u % 2 == 0 else min(int(total[u]) + 2, t + 5))
        seq[u] = cut
    if lengths == 'empty':
        seq[0] = 0
        if b > 1:
            seq[1] = -3
    return dur, target, seq


def stats_map(dur, t):
    """(rows (B t,) with -1, rows_mapped with the pad row R, seg (2, R)) of a duration table, from datapath_ref."""
    rows, mapped, seg = upsample_index_maps(dur, t)
    return rows.reshape(-1), mapped.reshape(-1), seg


def front_ok(b, p, t, extra):
    """ops.phone_front_ok, restated."""
    if not (b > 0 and p > 0 and t > 0 and extra > 0 and p <= 12288 and b <= -(-(b * p) // 16)):
        return False
    chunk = -(-(b * t) // extra)
    return 512 + max(p + t + 1, -(-(4 * chunk) // t) + 2) <= 16000


MSE_ROWS_N = (1, 1023, 1024, 1025, 2500)


def mse_rows_case(n, ldp, seed=20261106):
    """(pred (n, ldp), ybar, weight): weights uniform / n with every fifth an exact zero (its prediction huge: the guard must keep it
    out) and, from n = 4 on, one NaN at row 3; the last row is live and heavy."""
    rng = np.random.RandomState(seed + n + ldp)
    pred = rng.standard_normal((n, ldp)).astype(F32)
    ybar = rng.standard_normal(n).astype(F32)
    weight = (rng.uniform(0.1, 1.0, n) / n).astype(F32)
    weight[4::5] = 0.0
    pred[4::5, 0] = 1e30
    ybar[4::5] = 0.0
    if n >= 4:
        weight[3] = np.nan
    weight[n - 1], pred[n - 1, 0] = F32(2.0 / n), F32(0.75)
    return pred, ybar, weight


EXPAND_M = (1, 255, 256, 257, 700)
PARTIAL_SLOTS = ((16, 0), (16 * 254, 4), (16 * 255, 3), (16 * 255 + 1, 4), (16 * 298, 8))      # (R, extra): 1, 255, 256, 257, 300 slots


def expand_case(m, n_rows, extra, seed=20261107):
    """(table (64,), rows (m,) in 0 .. 63, partial slots, loss)."""
    rng = np.random.RandomState(seed + m + n_rows + extra)
    table = rng.standard_normal(64).astype(F32)
    rows = rng.randint(0, 64, size=m).astype(np.int32)
    partial = (rng.uniform(0, 1, n_partials(n_rows, extra)) * 1e-3).astype(F32)
    return table, rows, partial, F32(rng.uniform(0.5, 1.5))
