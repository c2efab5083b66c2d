"""References of the data-path kernels (csrc/upsample.hip, loss_norm.hip, metrics.hip and the elementwise half of optim.hip), in two
families.  Plain numpy; no torch, no import of the package.

EXACT family - the device result must equal the reference bit for bit:
  * index maps from np.cumsum / np.repeat (no binary search is restated here);
  * row movers: copies, and float32 -> bf16 as round-to-nearest-even ON THE BIT PATTERN (`bf16_bits`);
  * fixed-order float32 sums: the kernel's documented order of additions is replayed in np.float32.  Only additions are involved,
    so no fused multiply-add can change a bit.  These also return the float64 sum and a bound, so that a wrong ORDER fails the exact
    check alone while a wrong TERM fails both.

BOUNDED family - float64 values from the float32 inputs and a per-element bound that is derived, not fitted.  U = 2^-24 is the unit
roundoff: every float32 operation returns its exact result times (1 + d), |d| <= U; first order (products of error terms are
dropped); ETA = 2^-149 is added wherever a result can underflow to the subnormal grid.  Library calls are charged twice their
documented error, as ce_ref64 / mdn_ref64 do: expf and logf are documented at 1 ulp = 2U relative, 4U is charged (EXP_ULPS = LOG_ULPS = 2);
`/` and sqrtf are correctly rounded in this build (hipcc's default), U each.  Where hipcc may or may not contract a multiply and an
add into one fma, the count is that of the UNFUSED form: the fused form drops a rounding and so lies inside the same bound.  The
count of each result is stated in its function's docstring.

A reduction is charged DEPTH * U * sum|terms|: a term that passes through k additions (or divisions) picks up at most k U relative."""
import numpy as np

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24
ETA = 2.0 ** -149
EXP_ULPS = 2.0
LOG_ULPS = 2.0
MSE_CHUNK = 8192          # elements of one utterance per workgroup of the masked losses (csrc/loss_norm.hip)
PAD_CHUNK = 256           # frames per stage-1 workgroup of pad_rows_colsum (csrc/upsample.hip)
MAX_PHONES = 12288

NORM_MVN, DENORM_MVN, NORM_MINMAX, DENORM_MINMAX = 0, 1, 2, 3
METRIC_KINDS = ('mean', 'sqdiff', 'absdiff', 'root_sq', 'sqdiff_voiced', 'sqdiff_voiced_exp')      # in the order of MG_METRIC_*


def pad_ld(n):
    """Leading dimension of a bf16 operand with n columns: a multiple of 64 from 64 columns on, of 8 below."""
    return (n + 63) // 64 * 64 if n >= 64 else (n + 7) // 8 * 8


# =================================================================================================================== bf16
def bf16_bits(x):
    """float32 -> the uint16 bit pattern of its bf16 rounding, round to nearest, ties to even, on the bit pattern:
    (u + 0x7fff + bit 16 of u) >> 16.  +-0 and +-Inf map to themselves, the largest finite float32 carries into Inf, a float32
    subnormal rounds on the same grid (IEEE; what a device returns for one is recorded by the tests, not asserted).  A NaN gives
    0x7fc0 with its sign: compare NaNs with `bf16_is_nan`, not by bits."""
    x = np.ascontiguousarray(x, dtype=F32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x)
    return np.where(nan, ((u >> 16) & 0x8000).astype(np.uint16) | np.uint16(0x7fc0), r).astype(np.uint16)


def bf16_is_nan(bits):
    bits = np.asarray(bits, dtype=np.uint16)
    return ((bits & 0x7f80) == 0x7f80) & ((bits & 0x007f) != 0)


def bf16_to_f32(bits):
    """bf16 bit patterns -> the float32 they denote (exact: 16 zero bits behind)."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def bits_equal_bf16(got, want):
    """Equal uint16 patterns, NaN positions compared by is-NaN alone."""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    gn, wn = bf16_is_nan(got), bf16_is_nan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(got[~wn], want[~wn])


def bits_equal_f32(got, want):
    """Equal float32 bit patterns (a moved NaN keeps its payload, -0 stays -0)."""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def special_values():
    """The float32 values every row mover is fed: +-0, +-Inf, both parities of an exact bf16 tie (0x3f808000 lies half-way between
    0x3f80 and 0x3f81 and goes DOWN to the even 0x3f80, 0x3f818000 goes UP to the even 0x3f82), their negatives, one bit to either
    side of a tie, the largest finite float32 (rounds to Inf), and a NaN."""
    u = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f807fff,
                  0x3f808001, 0x7f7fffff, 0xff7fffff, 0x7fc00000, 0x40490fdb], dtype=np.uint32)
    return u.view(F32).copy()


def subnormal_values():
    """float32 subnormals (and the smallest normal): what a bf16-producing kernel returns for them is recorded, and all such kernels
    must agree."""
    return np.array([0x00000001, 0x00008000, 0x00018000, 0x007fffff, 0x807fffff, 0x00800000], dtype=np.uint32).view(F32).copy()


def fill_specials(x, rng, subnormals=False):
    """Scatter the special values over a copy of float32 array x (at least one of each where x is large enough)."""
    x = np.array(x, dtype=F32, copy=True)
    flat = x.reshape(-1)
    vals = np.concatenate([special_values(), subnormal_values()]) if subnormals else special_values()
    pos = rng.permutation(flat.size)[:min(flat.size, 3 * vals.size)]
    flat[pos] = vals[np.arange(pos.size) % vals.size]
    return x


# ============================================================================================================== index maps
def _durations(dur):
    d = np.asarray(dur, dtype=np.int64)
    return np.maximum(d.reshape(d.shape[0], -1), 0)           # a negative duration owns no frame


def upsample_lengths(dur):
    """(n_frames (B,) int64, tmax int64): frames per utterance and their maximum (0 at least)."""
    n = _durations(dur).sum(axis=1)
    return n, np.int64(max(int(n.max()), 0))


def upsample_index(dur, t_cap):
    """idx (B, t_cap) int64: the phone of frame t, -1 behind the utterance's last frame.  np.repeat per utterance, cut at t_cap."""
    d = _durations(dur)
    idx = -np.ones((d.shape[0], int(t_cap)), dtype=np.int64)
    for b in range(d.shape[0]):
        run = np.repeat(np.arange(d.shape[1]), d[b])[:int(t_cap)]
        idx[b, :run.size] = run
    return idx


def upsample_index_maps(dur, t_cap):
    """rows (B, t_cap) int32 = b P + phone or -1; rows_mapped: the same with -1 -> pad_row = B P; seg (2, B P): the frame run
    [start, end) of every phone row in flat frame ids b t_cap + t, (0, 0) for a phone without a frame below t_cap."""
    d = _durations(dur)
    b, p = d.shape
    idx = upsample_index(d, t_cap)
    flat = idx + (np.arange(b) * p)[:, None]
    rows = np.where(idx < 0, -1, flat).astype(np.int32)
    mapped = np.where(idx < 0, b * p, flat).astype(np.int32)
    cum = np.minimum(np.cumsum(d, axis=1), int(t_cap))
    start = np.concatenate([np.zeros((b, 1), dtype=np.int64), cum[:, :-1]], axis=1)
    base = (np.arange(b) * int(t_cap))[:, None]
    some = cum > start
    seg = np.stack([np.where(some, base + start, 0), np.where(some, base + cum, 0)]).reshape(2, b * p).astype(np.int32)
    return rows, mapped, seg


def segment_index(seg_lens, t, max_len):
    """split (B, S, L) int32: flat row b T + start_s + j for j < len_s and start_s + j < T, else -1; ends (B, S): b T + cumsum_s - 1 for
    len_s > 0 and cumsum_s <= T, else -1."""
    d = _durations(seg_lens)
    b, s = d.shape
    cum = np.cumsum(d, axis=1)
    start = cum - d
    base = (np.arange(b) * int(t))[:, None]
    ends = np.where((d > 0) & (cum <= t), base + cum - 1, -1).astype(np.int32)
    j = np.arange(int(max_len))[None, None, :]
    pos = start[:, :, None] + j
    split = np.where((j < d[:, :, None]) & (pos < t), base[:, :, None] + pos, -1).astype(np.int32)
    return split, ends


def frame_layout(seq_len, t, total):
    """(offsets (B+1,), rows (total+1,), inverse (B t,)) int32 of the packed-frame form.  n_b = seq_len clipped to [0, t]; packed row
    offsets[b] + j holds dense row b t + j for j < n_b; rows[total] = -1; a packed row in [sum n_b, total) names no frame (-1); a frame
    whose packed row would be >= total counts as padding; inverse of a padded frame = total."""
    n = np.clip(np.asarray(seq_len, dtype=np.int64).reshape(-1), 0, int(t))
    b = n.size
    offsets = np.concatenate([[0], np.cumsum(n)])
    rows = -np.ones(int(total) + 1, dtype=np.int64)
    inverse = np.full(b * int(t), int(total), dtype=np.int64)
    dense = np.concatenate([np.arange(b_ * t, b_ * t + n[b_]) for b_ in range(b)]) if b else np.zeros(0, dtype=np.int64)
    packed = np.arange(dense.size)
    keep = packed < total
    rows[packed[keep]] = dense[keep]
    inverse[dense[keep]] = packed[keep]
    return offsets.astype(np.int32), rows.astype(np.int32), inverse.astype(np.int32)


def sequence_mask(seq_len, max_len, dtype):
    """(B, max_len, 1) of `dtype`: 1 where t < seq_len[b]."""
    n = np.asarray(seq_len, dtype=np.int64).reshape(-1)
    return (np.arange(int(max_len))[None, :] < n[:, None])[:, :, None].astype(dtype)


# ============================================================================================================== row movers
def gather_rows(src, rows):
    """out[m] = src[rows[m]], a zero row for rows[m] < 0.  float32, moved bit for bit."""
    src = np.asarray(src, dtype=F32)
    rows = np.asarray(rows).reshape(-1)
    out = src[np.maximum(rows, 0)].copy()
    out[rows < 0] = 0.0
    return out


def _pad_bits(bits, ld, extra_rows=0):
    out = np.zeros((bits.shape[0] + extra_rows, ld), dtype=np.uint16)
    out[:bits.shape[0], :bits.shape[1]] = bits
    return out


def gather_rows_bf16(src, rows, ld=None):
    """bf16 bits (M, ld) of gather_rows, columns F .. ld-1 zero; ld defaults to pad_ld(F)."""
    f = np.asarray(src).shape[1]
    return _pad_bits(bf16_bits(gather_rows(src, rows)), pad_ld(f) if ld is None else int(ld))


def gather_concat(src, rows, extra):
    """[src[rows] | extra] per row, float32 (M, F + C)."""
    return np.concatenate([gather_rows(src, rows), np.asarray(extra, dtype=F32)], axis=1)


def gather_concat_bf16(src, rows, extra):
    """bf16 bits (M, pad_ld(F + C)) of gather_concat, zero padded."""
    cat = gather_concat(src, rows, extra)
    return _pad_bits(bf16_bits(cat), pad_ld(cat.shape[1]))


def scatter_rows(src, rows, n_dst_rows):
    """zeros (n_dst_rows, F) with dst[rows[m]] = src[m] for rows[m] >= 0 (distinct targets)."""
    src = np.asarray(src, dtype=F32)
    rows = np.asarray(rows).reshape(-1)
    dst = np.zeros((int(n_dst_rows), src.shape[1]), dtype=F32)
    dst[rows[rows >= 0]] = src[rows >= 0]
    return dst


def cast_pad_bf16(x, ld=None, extra_rows=0):
    """(rows, cols) float32 -> bf16 bits (rows + extra_rows, ld), padding columns and extra rows zero."""
    x = np.asarray(x, dtype=F32)
    return _pad_bits(bf16_bits(x), pad_ld(x.shape[1]) if ld is None else int(ld), extra_rows)


def cast_transpose_bf16(x, ld=None):
    """(rows, cols) float32 -> bf16 bits (cols, ld) of the transpose; ld defaults to pad_ld(rows)."""
    x = np.asarray(x, dtype=F32)
    return _pad_bits(bf16_bits(x.T), pad_ld(x.shape[0]) if ld is None else int(ld))


def cast_bf16_f32(bits, cols):
    """bf16 bits (rows, ld) -> float32 (rows, cols): the first `cols` columns, exact."""
    return bf16_to_f32(np.asarray(bits, dtype=np.uint16)[:, :int(cols)])


# ====================================================================================================== fixed-order sums
def _serial_sum_f32(terms):
    """acc = 0; acc += terms[k] for k ascending, in float32; terms (K, ...) -> (...)."""
    acc = np.zeros(terms.shape[1:], dtype=F32)
    for k in range(terms.shape[0]):
        acc = (acc + terms[k]).astype(F32)
    return acc


def upsample_backward(grad_out, dur, n_phones):
    """grad_src[b, p, :] = sum of grad_out[b, t, :] over the frames of phone p below T, ascending t from a float32 zero.
    Returns {'exact' float32 (B, P, F), 'sum' float64, 'bound'}: bound = n U sum|terms| for a run of n frames (n - 1 roundings)."""
    g = np.asarray(grad_out, dtype=F32)
    b, t, f = g.shape
    d = _durations(dur)
    assert d.shape == (b, n_phones)
    cum = np.minimum(np.cumsum(d, axis=1), t)
    start = np.concatenate([np.zeros((b, 1), dtype=np.int64), cum[:, :-1]], axis=1)
    exact = np.zeros((b, n_phones, f), dtype=F32)
    total = np.zeros((b, n_phones, f), dtype=F64)
    bound = np.zeros((b, n_phones, f), dtype=F64)
    for i in range(b):
        for p in range(n_phones):
            run = g[i, start[i, p]:cum[i, p]]
            if run.shape[0]:
                exact[i, p] = _serial_sum_f32(run)
                total[i, p] = run.astype(F64).sum(axis=0)
                bound[i, p] = run.shape[0] * U * np.abs(run.astype(F64)).sum(axis=0)
    return {'exact': exact, 'sum': total, 'bound': bound}


def pad_rows_colsum(g, seq_len):
    """out[d] = sum over the padded frames (t >= n_b, n_b = seq_len[b] clipped to [0, T]) of g[b, t, d], in the kernel's order:
    stage 1, per (b, 256-frame chunk c): wave w adds t = t_lo + w, t_lo + w + 4, ... below t_hi (t_lo = max(256 c, n_b),
    t_hi = min(256 c + 256, T)) from zero, then partial = (r0 + r1) + (r2 + r3);
    stage 2, over the B * chunks partials in (b, c) order: wave w adds partials w, w + 16, ... from zero, then the 16 wave sums are
    added ascending from zero.
    Returns {'exact' (D,) float32, 'sum' float64, 'bound'}; bound = (ceil(256 / 4) + 2 + ceil(n_partials / 16) + 16) U sum|terms|."""
    g = np.asarray(g, dtype=F32)
    b, t, d = g.shape
    n = np.clip(np.asarray(seq_len, dtype=np.int64).reshape(-1), 0, t)
    n_chunks = (t + PAD_CHUNK - 1) // PAD_CHUNK
    partial = np.zeros((b * n_chunks, d), dtype=F32)
    for i in range(b):
        for c in range(n_chunks):
            t_lo, t_hi = max(c * PAD_CHUNK, int(n[i])), min(c * PAD_CHUNK + PAD_CHUNK, t)
            r = [_serial_sum_f32(g[i, t_lo + w:t_hi:4]) if t_lo + w < t_hi else np.zeros(d, dtype=F32) for w in range(4)]
            partial[i * n_chunks + c] = ((r[0] + r[1]).astype(F32) + (r[2] + r[3]).astype(F32)).astype(F32)
    waves = np.stack([_serial_sum_f32(partial[w::16]) for w in range(16)])
    exact = _serial_sum_f32(waves)
    pad = np.arange(t)[None, :, None] >= n[:, None, None]
    terms = np.where(pad, g.astype(F64), 0.0)
    depth = PAD_CHUNK // 4 + 2 + (b * n_chunks + 15) // 16 + 16
    return {'exact': exact, 'sum': terms.sum(axis=(0, 1)), 'bound': depth * U * np.abs(terms).sum(axis=(0, 1))}


# =========================================================================================================== masked losses
def valid_frames(seq_len, b, t):
    if seq_len is None:
        return np.full(b, t, dtype=np.int64)
    return np.clip(np.asarray(seq_len, dtype=np.int64).reshape(-1), 0, t)


def loss_depth(b, chunks):
    """Additions / divisions a term of a masked loss passes through on the way into the scalar: 32 per thread of a chunk (8192
    elements over 256 threads), 6 levels of the wave butterfly, 2 for the four wave sums, `chunks` serial additions in the finish,
    the division by n_b, ceil(B / 256) utterances per finish thread, 8 levels of the 256-thread tree, the final division."""
    return 32 + 6 + 2 + chunks + 1 + (b + 255) // 256 + 8 + 1


def _bce_elem(p, y, dp=None):
    """Float64 loss and gradient factor of one BCE element from a probability p, and their float32 bounds.  dp: the absolute error
    the kernel's own p already carries (the sigmoid of stream_loss), None for an input p (exact).

    loss  l = -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)).  Charged: logf 2 LOG_ULPS U |log|; q = 1 - p one rounding, which
    log turns into U absolute (dq / q); 1 - y one rounding; the two products and the sum one rounding each.  A clamped log is exact
    (-100 on both sides; the clamp is 1-Lipschitz, so a log within its error of -100 is covered by the unclamped charge):
        bound_l = |y| ((2 LOG_ULPS + 1) U |lp| + dp / p) + |1 - y| ((2 LOG_ULPS + 2) U |lq| + U + dq / q) + U |l|
    with dq = dp; where q <= 2 (dq + U q) the kernel's log(1 - p) may be anything in [-100, 0] and 100 is charged in place of
    dq / q (only reachable through a sigmoid that saturates).
    gradient factor  f = (p - y) / max((1 - p) p, 1e-12f), the constant being the float32 one.  Charged: p - y, 1 - p, the product,
    the division: 4U relative, plus dp on the numerator and on each factor of the denominator:
        bound_f = |f| 4U + (dp / max(den, c)) (1 + |f| (p + q))        (dp = 0 for an input p)
    Returns (l, bound_l, f, bound_f, den)."""
    c = float(F32(1e-12))
    dp = np.zeros_like(p) if dp is None else dp
    with np.errstate(all='ignore'):
        q = 1.0 - p
        lp = np.maximum(np.log(p), -100.0)
        lq = np.maximum(np.log(q), -100.0)
        l = -(y * lp + (1.0 - y) * lq)
        l = np.where(np.isnan(l), np.where(y == 0, -lq, -lp), l)          # 0 * -100 never arises (the clamp), guard all the same
        dq = dp + U * q
        lq_err = np.where(q > 2 * dq, (2 * LOG_ULPS + 2) * U * np.abs(lq) + U + dp / np.maximum(q, 1e-300), 100.0)
        lq_err = np.where(dp == 0, (2 * LOG_ULPS + 2) * U * np.abs(lq) + np.where(lq > -100.0, U, 0.0), lq_err)
        lp_err = (2 * LOG_ULPS + 1) * U * np.abs(lp) + np.where(lp > -100.0, dp / np.maximum(p, 1e-300), 0.0)
        bound_l = np.abs(y) * lp_err + np.abs(1.0 - y) * lq_err + U * np.abs(l)
        den = np.maximum(q * p, c)
        f = (p - y) / den
        bound_f = np.abs(f) * 4 * U + dp / den * (1.0 + np.abs(f) * (p + q))
    return l, bound_l, f, bound_f, den


def masked_loss(pred, target, seq_len=None, grad_scale=1.0, kind='mse'):
    """losses.mse / losses.bce under the sequence mask: L = mean_{b,d}( sum_{t < n_b} l[b,t,d] / n_b ), g = grad_scale l' m / (n_b B D).
    pred / target (B, T, D) float32.  n_b = 0 gives a NaN loss and NaN on every gradient element of that utterance (0 * inf).

    mse: l = (p - y)^2: the difference and the square, 3U |l|.  g = 2 (p - y) coef, coef = grad_scale / (float(n_b) * float(B D)): the
    difference (U), coef's product and quotient (2U), the last product (U): 4U |g| + ETA.
    bce: `_bce_elem`; g = f coef adds coef (2U) and the product (U): (bound_f + 3U |f|) |coef| + ETA.
    loss_bound = sum_b sum_e (bound_l + loss_depth U |l|) / (n_b B D) over the utterances with n_b > 0.

    Returns a dict: loss, loss_bound, grad, grad_bound (B, T, D), nan_rows (B,) bool (utterances whose gradient is all NaN), mask."""
    p = np.asarray(pred, dtype=F32).astype(F64)
    y = np.asarray(target, dtype=F32).astype(F64)
    b, t, d = p.shape
    n = valid_frames(seq_len, b, t)
    mask = np.broadcast_to((np.arange(t)[None, :] < n[:, None])[:, :, None], p.shape)
    if kind == 'mse':
        l = (p - y) ** 2
        bound_l = 3 * U * l
        f = 2.0 * (p - y)
        bound_f = U * np.abs(f)
    else:
        l, bound_l, f, bound_f, _ = _bce_elem(p, y)
    chunks = (t * d + MSE_CHUNK - 1) // MSE_CHUNK
    depth = loss_depth(b, chunks)
    nf = n.astype(F64)
    with np.errstate(all='ignore'):
        w = 1.0 / (nf * b * d)
        lm, blm = np.where(mask, l, 0.0), np.where(mask, bound_l, 0.0)
        loss = np.where(n > 0, lm.sum(axis=(1, 2)) * w, np.nan).sum()
        loss_bound = np.where(n > 0, (blm + depth * U * np.abs(lm)).sum(axis=(1, 2)) * w, 0.0).sum()
        coef = (float(grad_scale) * w)[:, None, None]
        grad = np.where(mask, f * coef, 0.0)
        grad_bound = np.where(mask, (bound_f + 3 * U * np.abs(f)) * np.abs(coef) + ETA, 0.0)
    nan_rows = n == 0
    grad[nan_rows] = np.nan
    grad_bound[nan_rows] = 0.0
    return {'loss': float(loss), 'loss_bound': float(loss_bound), 'grad': grad, 'grad_bound': grad_bound, 'nan_rows': nan_rows,
            'mask': mask, 'n': n}


def stream_loss(pred, targets, kinds, seq_len=None, grad_scale=1.0):
    """The multi-stream loss: the columns of pred (B, T, D) are split into streams in column order, stream k of width w_k scored against
    targets[k] (B, T, w_k) with kind 'mse' or 'sigmoid_bce'; L = mean over streams of the masked stream losses.  An element of stream k
    weighs colw_k = 1 / (B w_k n_streams) in the loss; its gradient is grad_scale l' m colw_k / n_b.

    Float32 count.  colw_k: two exact integer products and a division, U.  mse: l 3U (difference, square), the weighted term
    (l m) colw_k one more product: 5U |term|; g = (l' m) (inv_nb colw_k), inv_nb = grad_scale / n_b (U): difference, inv_nb, colw, their
    product, the last product: 5U |g| + ETA.
    sigmoid_bce: p = 1 / (1 + expf(-x)): expf 2 EXP_ULPS U on e = exp(-x), which reaches p weighted by e / (1 + e) = 1 - p; the sum and
    the reciprocal U each: dp = p ((1 - p) 2 EXP_ULPS U + 2U) + ETA - this is `prob`'s bound.  The loss and the gradient factor follow
    `_bce_elem` with that dp.  The gradient multiplies the factor by the kernel's own (1 - p) p again: where the denominator is not
    clamped (den >= 2 c) the two cancel to p - y up to the division and the product (2U) and the numerator's dp + U |p - y|; where it is
    clamped, r = (1 - p) p / c is in [0, 1] with absolute error min(1, (dp (p + q) + 2U q p) / c).  Then the four roundings of the
    coefficient as for mse:
        bound_g = |coef| ((dp + U |p - y|) r + |p - y| dr + 6U |p - y| r) + ETA,   g = coef (p - y) r,   r = (1 - p) p / max((1 - p) p, c)
    loss_bound = sum over elements of (bound_term + loss_depth U |term|) / n_b.

    Returns a dict: loss, loss_bound, grad, grad_bound, prob, prob_bound (None without a sigmoid stream), nan_rows, mask."""
    x = np.asarray(pred, dtype=F32).astype(F64)
    b, t, d = x.shape
    n = valid_frames(seq_len, b, t)
    mask2 = np.arange(t)[None, :] < n[:, None]
    n_streams = len(targets)
    c = float(F32(1e-12))
    term = np.zeros_like(x)
    bound_term = np.zeros_like(x)
    gfac = np.zeros_like(x)               # d loss / d x before the 1 / n_b and grad_scale
    bound_gfac = np.zeros_like(x)
    prob = prob_bound = None
    col = 0
    for yk, kind in zip(targets, kinds):
        yk = np.asarray(yk, dtype=F32).astype(F64)
        w = yk.shape[2]
        xs = x[:, :, col:col + w]
        colw = 1.0 / (b * w * n_streams)
        if kind == 'mse':
            l = (xs - yk) ** 2
            term[:, :, col:col + w] = l * colw
            bound_term[:, :, col:col + w] = 5 * U * l * colw
            gf = 2.0 * (xs - yk) * colw
            gfac[:, :, col:col + w] = gf
            bound_gfac[:, :, col:col + w] = 5 * U * np.abs(gf)
        else:
            with np.errstate(all='ignore'):
                p = 1.0 / (1.0 + np.exp(-xs))
                dp = p * ((1.0 - p) * 2 * EXP_ULPS * U + 2 * U) + ETA
                l, bound_l, _, _, _ = _bce_elem(p, yk, dp)
                q = 1.0 - p
                den = q * p
                r = den / np.maximum(den, c)
                dr = np.where(den >= 2 * c, 0.0, np.minimum(1.0, (dp * (p + q) + 2 * U * den) / c))
                py = np.abs(p - yk)
            term[:, :, col:col + w] = l * colw
            bound_term[:, :, col:col + w] = (bound_l + 2 * U * np.abs(l)) * colw
            gfac[:, :, col:col + w] = (p - yk) * r * colw
            bound_gfac[:, :, col:col + w] = colw * ((dp + U * py) * r + py * dr + 6 * U * py * r)
            prob, prob_bound = p, dp
        col += w
    assert col == d
    chunks = (t * d + MSE_CHUNK - 1) // MSE_CHUNK
    depth = loss_depth(b, chunks)
    m3 = np.broadcast_to(mask2[:, :, None], x.shape)
    nf = n.astype(F64)
    with np.errstate(all='ignore'):
        tm, btm = np.where(m3, term, 0.0), np.where(m3, bound_term, 0.0)
        loss = np.where(n > 0, tm.sum(axis=(1, 2)) / nf, np.nan).sum()
        loss_bound = np.where(n > 0, (btm + depth * U * np.abs(tm)).sum(axis=(1, 2)) / nf, 0.0).sum()
        inv = (float(grad_scale) / nf)[:, None, None]
        grad = np.where(m3, gfac * inv, 0.0)
        grad_bound = np.where(m3, bound_gfac * np.abs(inv) + ETA, 0.0)
    nan_rows = n == 0
    grad[nan_rows] = np.nan
    grad_bound[nan_rows] = 0.0
    return {'loss': float(loss), 'loss_bound': float(loss_bound), 'grad': grad, 'grad_bound': grad_bound, 'prob': prob,
            'prob_bound': prob_bound, 'nan_rows': nan_rows, 'mask': m3, 'n': n}


# ============================================================================================================== normalisers
def normalise(x, p0, p1, kind):
    """(value float64, bound) of the four normalisers on x (..., D) with per-column parameters.
    NORM_MVN    r = (x - mean) / (std + 1e-8f): a difference, a sum, a quotient: 3U |r| + ETA.
    DENORM_MVN  r = x std + mean: a product and a sum (or one fma): U |x std| + U |r| + ETA.
    MINMAX      scale = mmax - mmin (U), replaced by 1 where |scale| <= 1e-8f; NORM r = (x - mmin) / scale: 3U |r| + ETA;
                DENORM r = x scale + mmin: 2U |x scale| + U |r| + ETA.  With scale replaced by 1 the scale's own rounding is gone but
                the same formula is kept (it is then an over-count by U).
    The constants are the float32 ones.  A column whose |mmax - mmin| lies within U of the threshold is ambiguous: the tests have none."""
    x = np.asarray(x, dtype=F32).astype(F64)
    a = np.asarray(p0, dtype=F32).astype(F64).reshape(-1)
    b = np.asarray(p1, dtype=F32).astype(F64).reshape(-1)
    eps = float(F32(1e-8))
    if kind == NORM_MVN:
        r = (x - a) / (b + eps)
        return r, 3 * U * np.abs(r) + ETA
    if kind == DENORM_MVN:
        r = x * b + a
        return r, U * np.abs(x * b) + U * np.abs(r) + ETA
    scale = b - a
    scale = np.where(np.abs(scale) <= eps, 1.0, scale)
    if kind == NORM_MINMAX:
        r = (x - a) / scale
        return r, 3 * U * np.abs(r) + ETA
    r = x * scale + a
    return r, 2 * U * np.abs(x * scale) + U * np.abs(r) + ETA


def pad_normalise(packed, offsets, t, p0=None, p1=None, kind=None):
    """Packed utterances (sum len, D) + offsets (B + 1) -> (raw (B, t, D) float32, moved bit for bit; normalised value float64; its
    bound) - pad frames zero in all three, an utterance longer than t clipped.  kind None: no normalised output (None, None)."""
    packed = np.asarray(packed, dtype=F32)
    offsets = np.asarray(offsets, dtype=np.int64)
    b, d = offsets.size - 1, packed.shape[1]
    raw = np.zeros((b, int(t), d), dtype=F32)
    live = np.zeros((b, int(t), 1), dtype=bool)
    for i in range(b):
        n = int(min(offsets[i + 1] - offsets[i], t))
        if n > 0:
            raw[i, :n] = packed[offsets[i]:offsets[i] + n]
            live[i, :n] = True
    if kind is None:
        return raw, None, None
    r, bound = normalise(raw, p0, p1, kind)
    return raw, np.where(live, r, 0.0), np.where(live, bound, 0.0)


# ================================================================================================================ optimiser
def ema_update(shadow, param, decay):
    """shadow - w (shadow - param) with w = float32(1 - decay), the weight torch forms (a Python float cast to the tensor's type).
    The kernel forms w' = 1.0f - float32(decay) instead: |w' - w| <= U |decay| + 2U w (the cast of decay, the two roundings to
    float32).  Then the difference (U), the product (U) and the last difference (U, alone if fused):
        bound = (U |decay| + 4U w) |shadow - param| + U |r| + ETA."""
    s = np.asarray(shadow, dtype=F32).astype(F64)
    p = np.asarray(param, dtype=F32).astype(F64)
    w = float(F32(1.0 - float(decay)))
    r = s - w * (s - p)
    return r, (U * abs(float(decay)) + 4 * U * w) * np.abs(s - p) + U * np.abs(r) + ETA


def adam_scalars(lr, betas, step):
    """(step_size, bc2_sqrt) as float32, as mg_adam_step_f32 / mg_adam_scalars form them: in double, but from lr and the betas as the C
    ABI receives them - float32.  torch forms them from Python doubles; with lr = 0.01 and betas (0.9, 0.999) the float32 arguments move
    step_size by up to 5U relative (0.09999997 for 0.1 at step 1).  The update itself is held to the scalars the kernel is handed."""
    bc1 = 1.0 - float(F32(betas[0])) ** int(step)
    bc2 = 1.0 - float(F32(betas[1])) ** int(step)
    return F32(float(F32(lr)) / bc1), F32(np.sqrt(bc2))


def adam_step(p, g, m, v, step_size, bc2_sqrt, betas, eps, weight_decay=0.0, grad_scale=1.0):
    """One Adam update in float64 from float32 state, with the scalars the kernel is handed (beta1, beta2, eps, weight_decay,
    grad_scale, step_size, bc2_sqrt: float32 values, exact here).  1 - beta is exact in float32 for beta >= 0.5 (Sterbenz).

        g1 = g grad_scale                          U |g1|
        g2 = g1 + weight_decay p                   U |g2|  (one fma)             dg = U |g1| + U |g2|   (U |g1| alone without decay)
        m' = m + (g2 - m)(1 - beta1)               the difference U, the fma U:  dm = (1 - beta1)(dg + U |g2 - m|) + U |m'|
        v' = ((1 - beta2) g2) g2 + v beta2         two products U each, the fma U:
                                                   dv = (1 - beta2)(U g2^2 + 2 |g2| dg) + U |v beta2| + U |v'|
        den = sqrtf(v') / bc2_sqrt + eps           sqrt carries dv / (2 sqrt v') and its own U; the division U; the sum U:
                                                   dden = (dv / (2 sqrt v') + 2U sqrt v') / bc2_sqrt + U den
        p' = p - step_size (m' / den)              quotient: dm / den + |q| dden / den + U |q|; product U; difference U:
                                                   dp = step_size (dq + U |q|) + U |p'|
    ETA is added to each.  Returns (p', m', v', bound_p, bound_m, bound_v), all float64."""
    p, g, m, v = (np.asarray(a, dtype=F32).astype(F64) for a in (p, g, m, v))
    b1, b2 = float(F32(betas[0])), float(F32(betas[1]))
    eps, wd, gs = float(F32(eps)), float(F32(weight_decay)), float(F32(grad_scale))
    ss, bc = float(step_size), float(bc2_sqrt)
    g1 = g * gs
    g2 = g1 + wd * p if wd != 0.0 else g1
    dg = U * np.abs(g1) + (U * np.abs(g2) if wd != 0.0 else 0.0)
    m2 = m + (g2 - m) * (1.0 - b1)
    dm = (1.0 - b1) * (dg + U * np.abs(g2 - m)) + U * np.abs(m2)
    v2 = (1.0 - b2) * g2 * g2 + v * b2
    dv = (1.0 - b2) * (U * g2 * g2 + 2 * np.abs(g2) * dg) + U * np.abs(v * b2) + U * np.abs(v2)
    root = np.sqrt(v2)
    den = root / bc + eps
    with np.errstate(all='ignore'):
        droot = np.where(root > 0, dv / (2 * np.maximum(root, 1e-300)), 0.0)
    dden = (droot + 2 * U * root) / bc + U * den
    q = m2 / den
    dq = dm / den + np.abs(q) * dden / den + U * np.abs(q)
    p2 = p - ss * q
    dp = abs(ss) * (dq + U * np.abs(q)) + U * np.abs(p2)
    return p2, m2, v2, dp + ETA, dm + ETA, dv + ETA


# ================================================================================================================== metrics
def metric_sums(kind, target, pred=None, voiced=None, seq_len=None, col0=0, width=None):
    """(sum, count, sum_bound) that one accumulate call adds.  kind: a name of METRIC_KINDS.  Frames t < seq_len[b] take part (all
    without seq_len; seq_len is NOT clipped: above T every frame is live); columns [col0, col0 + width).
    count (exact): sum of the voiced flags over live frames for the voiced kinds; live frames with seq_len or for root_sq; else live
    frames * width (the reference's unmasked count is in elements).
    sum: per frame a float32 accumulation over `width` columns from zero, then float64 across frames.  Per-frame charge, W = width:
      mean       W U sum|x|                              absdiff   (1 + W) U sum|d|
      sqdiff, sqdiff_voiced   (3 + W) U sum d^2          root_sq   ((3 + W) / 2 + 1) U root   (sqrt halves the relative error)
      sqdiff_voiced_exp       d = expf(t) - expf(p): 2 EXP_ULPS U (e^t + e^p) + U |d| absolute, squared: 2 |d| dd + (1 + W) U d^2
    one more U for the product with the voiced flag, and 2^-53 * frames of the total for the float64 reduction."""
    tg = np.asarray(target, dtype=F32).astype(F64)
    b, t, d = tg.shape
    width = d - col0 if width is None else int(width)
    tg = tg[:, :, col0:col0 + width]
    live = np.ones((b, t), dtype=bool)
    if seq_len is not None:
        live = np.arange(t)[None, :] < np.asarray(seq_len, dtype=np.int64).reshape(-1)[:, None]
    w = width
    if kind == 'mean':
        frame = tg.sum(axis=2)
        fb = w * U * np.abs(tg).sum(axis=2)
    else:
        pr = np.asarray(pred, dtype=F32).astype(F64)[:, :, col0:col0 + width]
        if kind == 'sqdiff_voiced_exp':
            et, ep = np.exp(tg), np.exp(pr)
            diff = et - ep
            dd = 2 * EXP_ULPS * U * (et + ep) + U * np.abs(diff)
            frame = (diff ** 2).sum(axis=2)
            fb = (2 * np.abs(diff) * dd + (1 + w) * U * diff ** 2).sum(axis=2)
        elif kind == 'absdiff':
            frame = np.abs(tg - pr).sum(axis=2)
            fb = (1 + w) * U * frame
        else:
            frame = ((tg - pr) ** 2).sum(axis=2)
            fb = (3 + w) * U * frame
            if kind == 'root_sq':
                frame = np.sqrt(frame)
                fb = ((3 + w) / 2.0 + 1) * U * frame
    if kind.startswith('sqdiff_voiced'):
        vf = np.asarray(voiced, dtype=F32).astype(F64).reshape(b, t)
        count = float(np.where(live, vf, 0.0).sum())
        fb = np.abs(vf) * (fb + U * np.abs(frame))
        frame = frame * vf
    elif seq_len is not None or kind == 'root_sq':
        count = float(live.sum())
    else:
        count = float(live.sum() * width)
    total = float(np.where(live, frame, 0.0).sum())
    mag = float(np.where(live, np.abs(frame), 0.0).sum())
    bound = float(np.where(live, fb, 0.0).sum()) + 2.0 ** -53 * (b * t + 2048) * mag + ETA
    return total, count, bound


def metric_result(kind, total, count):
    """The value a metric class reports from its sums: mean = total / (count + 1e-8); its root for the squared kinds; in dB for root_sq."""
    mean = total / (count + 1e-8)
    if kind in ('sqdiff', 'sqdiff_voiced', 'sqdiff_voiced_exp'):
        return mean ** 0.5
    if kind == 'root_sq':
        return mean * (10.0 / np.log(10.0) * np.sqrt(2.0))
    return mean


# ============================================================================================ how close a check may come to its bound
# A REDUCTION (a loss, a metric sum, the float64 side of pad_rows_colsum) is charged the worst case of every addition on a term's way;
# the roundings of a correct kernel do not line up, so it stays far below (0.06 at most, emulated and measured) and is held to HALF its
# bound: a reduction that climbs towards 1 has lost or gained a term.  An ELEMENT-WISE result passes through one to seven roundings
# and its bound is their sum: where one rounding dominates (the last subtraction of adam_step p, ema_update and the denormalisers next
# to an update or a product that nearly cancels) the bound is ATTAINED when the result lies just above a power of two, and over 10^5
# elements 0.9 - 0.99 is reached by a correct kernel.  Charging those a rounding that does not exist would only hide a missed one, so
# they are held to the bound itself.  upsample_backward's float64 side counts here too: a phone of n <= 3 frames has n - 1 roundings and
# is charged n.
ELEMENTWISE_CHECKS = frozenset(
    ['masked_mse grad', 'masked_bce grad', 'stream_loss grad', 'stream_loss prob', 'ema_update', 'adam_step p', 'adam_step m',
     'adam_step v', 'upsample_backward sum'] + ['normalise kind %d' % k for k in range(4)] + ['pad_normalise kind %d' % k for k in (0, 2)])


def ratio_ceiling(check):
    """The largest worst-case error / bound a check may show: 1 for the element-wise checks, 0.5 for every reduction."""
    return 1.0 if check in ELEMENTWISE_CHECKS else 0.5


# ================================================================================================ the inputs the tests share
# Each generator is seeded by its arguments alone, so the host test (emulation against the bounds) and the GPU test see the same data.
MASKED_SHAPES = ((3, 1), (8191, 1), (8192, 1), (2731, 3), (2049, 4), (5000, 4))      # (T, D): T D in {3, 8191, 8192, 8193, 8196, 20000}
BCE_SPECIAL_P = np.array([0x00000000, 0x3f800000, 0x00000001, 0x3f7fffff], dtype=np.uint32).view(F32)     # 0, 1, 2^-149 (1e-45), 1 - 2^-24
BCE_SPECIAL_Y = np.array([0.0, 1.0, 0.3], dtype=F32)


def masked_lengths(t, d):
    """One length per branch: every frame; one frame; an odd count (with D = 1 the mask edge falls inside a 16-byte vector); exactly on
    the first chunk's edge where the row is longer than a chunk (else T - 1); so short that every later chunk is wholly padding; above T."""
    edge = MSE_CHUNK // d if MSE_CHUNK % d == 0 and MSE_CHUNK // d < t else max(t - 1, 1)
    odd = max(1, (t // 2) | 1) if t > 1 else 1
    return np.array([t, 1, min(odd, t), edge, min(5, t), t + 7], dtype=np.int64)


def masked_case(t, d, kind, seed=20261020):
    """(pred, target, seq_len) of one masked-loss case, B = 6.  mse: N(0, 1) against N(0, 1).  bce: p uniform in (0.02, 0.98) against targets
    drawn from {0, 1, 0.3}; utterance 0 (every frame valid) carries the twelve special pairs p in {0, 1, 2^-149, 1 - 2^-24} x y in
    {0, 1, 0.3} at its start and, where the row has more than one chunk, again at the start of its last chunk."""
    rng = np.random.RandomState(seed + 7 * t + d + (1000 if kind == 'bce' else 0))
    b = 6
    if kind == 'mse':
        pred = rng.standard_normal((b, t, d)).astype(F32)
        target = rng.standard_normal((b, t, d)).astype(F32)
    else:
        pred = rng.uniform(0.02, 0.98, size=(b, t, d)).astype(F32)
        target = BCE_SPECIAL_Y[rng.randint(0, 3, size=(b, t, d))]
        sp = np.repeat(BCE_SPECIAL_P, 3)
        sy = np.tile(BCE_SPECIAL_Y, 4)
        n = min(12, t * d)
        flat_p, flat_y = pred[0].reshape(-1), target[0].reshape(-1)
        flat_p[:n], flat_y[:n] = sp[:n], sy[:n]
        if t * d > MSE_CHUNK + 12:
            lo = (t * d - 1) // MSE_CHUNK * MSE_CHUNK
            k = min(12, t * d - lo)
            flat_p[lo:lo + k], flat_y[lo:lo + k] = sp[:k], sy[:k]
    return pred, target, masked_lengths(t, d)


def masked_nan_case(kind, seed=20261021):
    """B = 3, T = 5, D = 3 with lengths (0, -2, 4): the loss is NaN, the gradient of utterances 0 and 1 all NaN, utterance 2 as usual."""
    rng = np.random.RandomState(seed)
    shape = (3, 5, 3)
    if kind == 'mse':
        return rng.standard_normal(shape).astype(F32), rng.standard_normal(shape).astype(F32), np.array([0, -2, 4], dtype=np.int64)
    return (rng.uniform(0.02, 0.98, size=shape).astype(F32), BCE_SPECIAL_Y[rng.randint(0, 3, size=shape)],
            np.array([0, -2, 4], dtype=np.int64))


STREAM_CASES = (('d5', 5, 9, 'mixed'), ('d255', 255, 9, 'mixed'), ('d256', 256, 9, 'mixed'), ('d257', 257, 9, 'mixed'),
                ('d300', 300, 9, 'mixed'), ('d257_t40', 257, 40, 'mixed'), ('d5_single_mse', 5, 9, 'mse'),
                ('d5_single_bce', 5, 9, 'sigmoid_bce'), ('d5_empty', 5, 9, 'mixed_empty'))


def stream_case(name, seed=20261022):
    """(pred, targets, kinds, seq_len) of one multi-stream case, B = 3.  'mixed': streams of widths (3, 1, D - 4) and kinds (mse,
    sigmoid_bce, mse); the lengths are (T, 4, T + 3) - 'mixed_empty' has (T, 0, 5).  The sigmoid stream's logits are 2 N(0, 1), with
    +40 against target 1 and -40 against target 0 in utterance 0 (the saturated ends: p rounds to 1 on one side)."""
    _, d, t, form = [c for c in STREAM_CASES if c[0] == name][0]
    rng = np.random.RandomState(seed + 13 * d + t + len(name))
    b = 3
    pred = rng.standard_normal((b, t, d)).astype(F32)
    if form.startswith('mixed'):
        widths, kinds = (3, 1, d - 4), ('mse', 'sigmoid_bce', 'mse')
    else:
        widths, kinds = (d,), (form,)
    targets, col = [], 0
    for w, kind in zip(widths, kinds):
        if kind == 'mse':
            targets.append(rng.standard_normal((b, t, w)).astype(F32))
        else:
            pred[:, :, col:col + w] *= 2.0
            y = (rng.uniform(size=(b, t, w)) < 0.5).astype(F32)
            pred[0, 0, col], y[0, 0, 0] = 40.0, 1.0
            pred[0, 1, col], y[0, 1, 0] = -40.0, 0.0
            targets.append(y)
        col += w
    seq_len = np.array([t, 0, 5] if form == 'mixed_empty' else [t, 4, t + 3], dtype=np.int64)
    return pred, targets, list(kinds), seq_len


NORMALISE_SHAPES = ((1, 1), (7, 3), (1, 5000), (513, 600))


def normalise_case(rows, d, kind, seed=20261023):
    """(x (rows, D), p0, p1).  mvn: mean N(0, 1), std uniform (0.1, 2).  minmax: mmin N(0, 1), mmax = mmin + uniform (0.5, 3); with D >= 3,
    column 1 has mmax == mmin and column 2 has mmin = 0, mmax = 5e-9 (both take the scale = 1 branch)."""
    rng = np.random.RandomState(seed + 31 * rows + d + kind)
    x = rng.standard_normal((rows, d)).astype(F32)
    p0 = rng.standard_normal(d).astype(F32)
    if kind in (NORM_MVN, DENORM_MVN):
        p1 = rng.uniform(0.1, 2.0, size=d).astype(F32)
    else:
        p1 = (p0 + rng.uniform(0.5, 3.0, size=d).astype(F32)).astype(F32)
        if d >= 3:
            p1[1] = p0[1]
            p0[2], p1[2] = 0.0, 5e-9
    return x, p0, p1


def pad_normalise_case(d, t=6, seed=20261024):
    """(packed (16, D), offsets (5,), p0, p1 for mvn, p0, p1 for minmax): B = 4 utterances of 0, 1, t and t + 3 frames."""
    rng = np.random.RandomState(seed + d)
    lens = np.array([0, 1, t, t + 3], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    packed = rng.standard_normal((int(offsets[-1]), d)).astype(F32)
    _, m0, m1 = normalise_case(1, d, NORM_MVN, seed + 1)
    _, n0, n1 = normalise_case(1, d, NORM_MINMAX, seed + 2)
    return packed, offsets, (m0, m1), (n0, n1)


METRIC_SHAPES = ((1, 1, 1, 0, 1), (3, 50, 5, 1, 3), (3, 90000, 1, 0, 1))     # (B, T, D, col0, width)


def metric_case(shape, seed=20261025, grid=False):
    """(target, pred, voiced, seq_len) for one metric shape: values 0.5 N(0, 1) (multiples of 1/64 with `grid`, for which float32
    differences, squares and short sums are exact), voiced flags 0 / 1, lengths (T + 5, about T / 2, 1)[:B]."""
    b, t, d, _, _ = shape
    rng = np.random.RandomState(seed + b + t + d)
    target = (0.5 * rng.standard_normal((b, t, d))).astype(F32)
    pred = (target + 0.25 * rng.standard_normal((b, t, d))).astype(F32)
    if grid:
        target, pred = (np.round(target * 64) / 64).astype(F32), (np.round(pred * 64) / 64).astype(F32)
    voiced = (rng.uniform(size=(b, t, 1)) < 0.6).astype(F32)
    seq_len = np.array([t + 5, max(t // 2, 1), 1][:b], dtype=np.int64)
    return target, pred, voiced, seq_len


ADAM_SIZES = (1, 255, 1025, 10007)
ADAM_BETAS, ADAM_EPS, ADAM_LR = (0.9, 0.999), 1e-8, 0.01


def adam_case(n, seed=20261026):
    """(param, three gradients): gradients of magnitude 10^uniform(-6, 1) with random sign, and from n // 3 on a stretch of n // 8 + 1
    exact zeros in every step (m = v = 0 there: denom = eps)."""
    rng = np.random.RandomState(seed + n)
    param = rng.standard_normal(n).astype(F32)
    grads = []
    for _ in range(3):
        g = (10.0 ** rng.uniform(-6, 1, size=n) * np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)).astype(F32)
        g[n // 3:n // 3 + n // 8 + 1] = 0.0
        grads.append(g)
    return param, grads
