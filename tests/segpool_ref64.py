"""Restatement of ``utils.pool_segments`` (mg_segment_pool_f32 / mg_segment_pool_bwd_f32 of include/morgana_hip.h) in plain
numpy loops with ``np.longdouble`` sums, and the DERIVED bounds for what may differ from it.  No GPU and no torch.

For x (B, T, F), segment lengths (B, S) and n_b = seq_len[b] clamped to [0, T] (T without seq_len):

    start_s = sum_{j < s} max(len_j, 0)          the frames of segment s:  [start_s, min(start_s + max(len_s, 0), n_b))
    m       = the number of frames in that range (0 when start_s >= n_b)

    'sum'   v = sum_t x[b, t, f]                 'mean'  v = ( sum_t x[b, t, f] ) / m
    'max' / 'min'  v = x[b, t*, f] itself, t* the lowest frame that holds the extremum; with a NaN in the range t* is the lowest
                   NaN frame (torch.amax's rule: NaN wins).  -0 and +0 compare equal, so the lower frame wins.
    m == 0  v = +0 in every mode, index -1, no gradient.

Gradients of sum_{b,s,f} g[b, s, f] v[b, s, f] with respect to x, dense (B, T, F):

    'sum'   g[b, s(t), f]        'mean'  g[b, s(t), f] / m        'max' / 'min'  g[b, s, f] at t = t*, +0 on the other frames
    +0 on every frame outside all ranges (at or past n_b, behind the last segment).

Bounds, from the number formats alone (float32 has 24 significant bits and subnormals down to 2^-149, float64 53 bits):

  * 'sum'.  The kernel adds m float64 terms; each of its m - 1 additions is good to 2^-53 relative to the partial sum it forms, and
    every partial sum is at most A = sum_t |x[b, t, f]|: the float64 total is within (m - 1) 2^-53 A of the exact sum.  The
    restatement's own long-double loop is at least as good, so the two are within m 2^-52 A of each other, with room for the
    second-order term of the step that follows.  The total is then rounded ONCE to float32: half an ulp, at most 2^-24 |v| for a
    normal result and at most 2^-150 < 2^-149 for a subnormal one.

        |got - v| <= 2^-24 |v| + 2^-149 + m 2^-52 A

  * 'mean'.  The float64 total, off by at most (m - 1) 2^-53 A, is divided by m in float64: the quotient is off by at most
    (m - 1) 2^-53 A / m plus one float64 rounding, 2^-53 |v| <= 2^-53 A / m.  Together at most 2^-53 A, charged as
    2^-52 A = (m 2^-52 A) / m, the sum's second term divided by m.  One rounding to float32 follows.

        |got - v| <= 2^-24 |v| + 2^-149 + 2^-52 A

  * 'mean' gradient.  (float)((double) g / m): one float64 rounding of the quotient, 2^-53 relative (charged as 2^-52 against the
    restatement's own division), and one rounding to float32.

        |got - g / m| <= 2^-24 |g / m| + 2^-149 + 2^-52 |g / m|

  * 'max' / 'min' values and indices, the 'sum' / 'max' / 'min' gradients and every +0: no arithmetic is involved, the bits must
    be equal (``same_bits``).
"""
import numpy as np

LD = np.longdouble
MODES = ('sum', 'mean', 'max', 'min')


def valid_frames(seq_len, b, t):
    if seq_len is None:
        return np.full(b, t, dtype=np.int64)
    return np.clip(np.asarray(seq_len, dtype=np.int64).reshape(b), 0, t)


def segment_ranges(segment_lens, seq_len, t):
    """(start, m) int64 (B, S): the first frame and the frame count of every segment, in plain loops."""
    lens = np.asarray(segment_lens, dtype=np.int64)
    lens = lens.reshape(lens.shape[0], -1)
    b, s = lens.shape
    n = valid_frames(seq_len, b, t)
    start, m = np.zeros((b, s), np.int64), np.zeros((b, s), np.int64)
    for i in range(b):
        pos = 0
        for j in range(s):
            length = max(int(lens[i, j]), 0)
            lo, hi = min(pos, int(n[i])), min(pos + length, int(n[i]))
            start[i, j], m[i, j] = lo, hi - lo
            pos += length
    return start, m


def frames_read(segment_lens, seq_len, t):
    """(B, T) bool: the frames that belong to a segment's range - every other frame must never be read."""
    start, m = segment_ranges(segment_lens, seq_len, t)
    read = np.zeros((start.shape[0], t), dtype=bool)
    for i in range(start.shape[0]):
        for j in range(start.shape[1]):
            read[i, start[i, j]:start[i, j] + m[i, j]] = True
    return read


def pool(x, segment_lens, mode, seq_len=None):
    """x (B, T, F) float32.  Returns a dict: ``value`` (B, S, F) - float64 for 'sum' / 'mean' (the long-double result), float32 for
    'max' / 'min' (the element itself); ``index`` int32 (B, S, F), the frame of the extremum, -1 for an empty segment and in the
    other modes; ``bound`` float64 (B, S, F), 0 where bits must be equal; ``start`` and ``m`` int64 (B, S)."""
    assert mode in MODES
    x = np.asarray(x, dtype=np.float32)
    b, t, f = x.shape
    start, m = segment_ranges(segment_lens, seq_len, t)
    s = start.shape[1]
    extremum = mode in ('max', 'min')
    value = np.zeros((b, s, f), dtype=np.float32 if extremum else np.float64)
    index = np.full((b, s, f), -1, dtype=np.int32)
    bound = np.zeros((b, s, f), dtype=np.float64)
    for i in range(b):
        for j in range(s):
            lo, count = int(start[i, j]), int(m[i, j])
            if count == 0:
                continue
            if extremum:
                best, at = x[i, lo].copy(), np.full(f, lo, dtype=np.int32)
                for k in range(lo + 1, lo + count):
                    v = x[i, k]
                    with np.errstate(invalid='ignore'):
                        better = v > best if mode == 'max' else v < best
                    take = ~np.isnan(best) & (np.isnan(v) | better)
                    best = np.where(take, v, best)
                    at = np.where(take, np.int32(k), at)
                value[i, j], index[i, j] = best, at
                continue
            total, scale = np.zeros(f, dtype=LD), np.zeros(f, dtype=LD)
            for k in range(lo, lo + count):
                total = total + x[i, k].astype(LD)
                scale = scale + np.abs(x[i, k]).astype(LD)
            if mode == 'mean':
                total = total / LD(count)
            value[i, j] = total.astype(np.float64)
            accumulation = float(count) * 2.0 ** -52 * scale.astype(np.float64)
            bound[i, j] = 2.0 ** -24 * np.abs(value[i, j]) + 2.0 ** -149 + (accumulation / count if mode == 'mean' else accumulation)
    return {'value': value, 'index': index, 'bound': bound, 'start': start, 'm': m}


def pool_grad(grad_out, segment_lens, mode, t, seq_len=None, index=None):
    """grad_out (B, S, F) float32 -> dict: ``grad`` (B, T, F), float32 for 'sum' / 'max' / 'min' (copies of grad_out's elements and
    +0), float64 for 'mean'; ``bound`` float64 (B, T, F), 0 where bits must be equal.  ``index``: what ``pool`` returned ('max' /
    'min')."""
    assert mode in MODES
    g = np.asarray(grad_out, dtype=np.float32)
    b, s, f = g.shape
    start, m = segment_ranges(segment_lens, seq_len, t)
    grad = np.zeros((b, t, f), dtype=np.float64 if mode == 'mean' else np.float32)
    bound = np.zeros((b, t, f), dtype=np.float64)
    for i in range(b):
        for j in range(s):
            lo, count = int(start[i, j]), int(m[i, j])
            for k in range(lo, lo + count):
                if mode == 'sum':
                    grad[i, k] = g[i, j]
                elif mode == 'mean':
                    quotient = (g[i, j].astype(LD) / LD(count)).astype(np.float64)
                    grad[i, k] = quotient
                    bound[i, k] = 2.0 ** -24 * np.abs(quotient) + 2.0 ** -149 + 2.0 ** -52 * np.abs(quotient)
                else:
                    grad[i, k] = np.where(index[i, j] == k, g[i, j], np.float32(0.0))
    return {'grad': grad, 'bound': bound}


def same_bits(got, want):
    """Bit equality of two float32 (or two integer) arrays: -0 differs from +0, and a NaN equals the same NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == np.float32:
        return bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
    return bool(np.array_equal(got, want))


def bound_share(got, want, bound):
    """The largest |got - want| / bound over the elements with a positive bound (0.0 when there is none); elements whose bound is 0
    must be equal and are asserted to be."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    exact = bound == 0
    assert np.array_equal(got[exact], want[exact]), 'elements that must be exact differ'
    if exact.all():
        return 0.0
    return float((np.abs(got - want)[~exact] / bound[~exact]).max())
