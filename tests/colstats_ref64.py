"""Float64 and exact restatements of per-column corpus statistics (count, mean, variance, min, max over the valid frames of ragged
items, per group), the reference of tests/test_colstats_host.py and tests/test_gpu_colstats.py, and the error bounds the device
kernel (csrc/colstats.hip, K22) is held to.

    two_pass      mean, then sum (x - mean)^2, in float64 (np.sum: pairwise)       - the reference
    exact         the same in rational arithmetic (fractions.Fraction)              - judges the reference on small inputs
    naive         sum x^2 / n - (sum x / n)^2 in float64, sequential or np.sum      - what the kernel must NOT be (shown to fail)
    chunk_chan    NumPy restatement of the kernel's scheme on one column            - shifted chunks + Chan's update

The bounds.  u = 2^-53.  Per column let R = max - min and A = max |x| over EVERYTHING the calls were given (all items of all
batches, those of other groups and of out-of-range groups included: the kernel's anchor is the first frame of the batch, whoever
owns it), N the count of the statistic, nb the number of batches (calls) the state saw.  What the kernel does, and what it costs:

  * chunk: at most L = CHUNK = 32 values, d = x - k with k the chunk's first value (|d| <= R, one rounding), s1 = sum d,
    s2 = sum d^2 (recursive: <= L u each), mean - anchor = (k - anchor) + s1 / n, M2 = s2 - s1^2 / n:
        |err mean| <= (L + 2) u R,      |err M2| <= (3 L + 5) u n R^2        (s2: (L + 2), s1^2 / n: (2 L + 2), the subtraction 1)
  * merge (Chan): mean = mean_a + delta n_b / n, M2 = M2_a + M2_b + delta^2 n_a n_b / n, everything relative to the anchor, so
    every quantity is <= R (means) or <= N R^2 (M2): a merge adds <= 3 u R to a mean and <= 4 u (its M2) to an M2.  A value's
    way to the state passes h <= DEPTH + nb merges: 2 in a thread (<= 96 steps of an item per workgroup: every test shape), 10
    levels of the workgroup's tree (<= 1024 frames per step), 16 records per lane of the second launch (<= 1024 jobs), 6 levels
    over the lanes, 1 per batch into the state.  So every mean - anchor the merges read is off by at most
        e = u R ((L + 2) + 3 h).
  * an error e_a, e_b in the two means of a merge moves its delta^2 n_a n_b / n by <= 2 |delta| (e_a + e_b) min(n_a, n_b)
    <= 4 R e min(n_a, n_b).  The merges fall into g <= STAGES + nb stages (thread chain, 10 tree levels, lane chain, 6 lane
    levels, the state) in each of which the smaller sides are disjoint data, so a stage adds <= 4 R e N to M2.
  * the state holds the full mean: one rounding u A per batch, so from the second batch on its mean is off by <= nb u A + e and
    each of the nb - 1 merges with it adds <= 2 R (nb u A + 2 e) min(n_a, n_b) <= R (nb u A + 2 e) N to M2.
  * var = M2 / N: one more rounding (<= u R^2).  The two-pass reference itself: np.sum is pairwise, <= (log2 N + 2) u of the
    largest partial sum: (log2 N + 2) u A on the mean, (log2 N + 4) u R^2 on the variance (the mean's error enters squared).

        bound_mean = (2 nb + log2 N + 2) u A + e
        bound_var  = u R^2 ((3 L + 5) + 4 h + 4 g ((L + 2) + 3 h) + log2 N + 5) + (nb - 1) R (nb u A + 2 e)

With nb = 1: bound_mean < 300 u A (cap of the tests: 2^-40 A = 8192 u A) and bound_var ~ 1.1e4 u R^2 = 1.2e-12 R^2 (cap: 1e-9 var,
met while R^2 <= 800 var: a column spread over less than 28 standard deviations; the 2^20 + k / 8 column has R^2 = 9.3 var).
Nothing above is fitted to what the kernel returns."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
CHUNK = 32
DEPTH = 2 + 10 + 16 + 6          # merges on a value's way to the state, without the state merges (one per batch)
STAGES = 1 + 10 + 1 + 6          # stages of merges with disjoint smaller sides, without the state merges
CAP_MEAN = 2.0 ** -40            # x max |x|
CAP_VAR = 1e-9                   # x var_ref


def _rows_of_group(items, item_row, group, groups):
    if item_row is None:
        picked = list(items) if group == 0 else []
    else:
        picked = [x for x, row in zip(items, item_row) if int(row) == group and 0 <= int(row) < groups]
    picked = [np.asarray(x, dtype=np.float32) for x in picked if len(x)]
    return np.concatenate(picked, axis=0) if picked else None


def two_pass(items, item_row=None, groups=1):
    """{'count', 'mean', 'm2', 'var', 'mmin', 'mmax'}: float64 (groups, D) over ragged ``items`` (list of (len, D) float32); item i
    belongs to group item_row[i] (all to group 0 without it), an item_row outside [0, groups) to none.  Population variance.
    A group without frames: count 0, NaN elsewhere.  min / max are those of the float32 values (exact)."""
    width = np.asarray(items[0]).shape[1]
    out = {k: np.full((groups, width), np.nan) for k in ('mean', 'm2', 'var', 'mmin', 'mmax')}
    out['count'] = np.zeros((groups, width))
    for g in range(groups):
        rows = _rows_of_group(items, item_row, g, groups)
        if rows is None:
            continue
        x = rows.astype(np.float64)
        n = x.shape[0]
        with np.errstate(invalid='ignore', over='ignore'):
            mean = np.sum(x, axis=0) / n
            m2 = np.sum((x - mean) ** 2, axis=0)
        out['count'][g] = n
        out['mean'][g], out['m2'][g], out['var'][g] = mean, m2, m2 / n
        with np.errstate(invalid='ignore'):
            out['mmin'][g], out['mmax'][g] = np.fmin.reduce(rows, axis=0), np.fmax.reduce(rows, axis=0)
    return out


def exact(column):
    """(mean, population variance) of a 1-D array as Fractions."""
    values = [Fraction(float(v)) for v in np.asarray(column).reshape(-1)]
    n = len(values)
    mean = sum(values) / n
    return mean, sum((v - mean) ** 2 for v in values) / n


def naive(column, sequential):
    """Population variance as sum x^2 / n - (sum x / n)^2 in float64: a python loop, or np.sum (pairwise)."""
    x = np.asarray(column, dtype=np.float64).reshape(-1)
    if sequential:
        s1 = s2 = 0.0
        for v in x:
            s1 += float(v)
            s2 += float(v) * float(v)
    else:
        s1, s2 = float(np.sum(x)), float(np.sum(x * x))
    return s2 / x.size - (s1 / x.size) ** 2


def chan(a, b):
    """Chan's update of (n, mean, M2) partials; an empty side is skipped, never divided by."""
    (na, ma, m2a), (nb, mb, m2b) = a, b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = na + nb
    delta = mb - ma
    return n, ma + delta * (nb / n), m2a + m2b + delta * delta * (na * nb / n)


def chunk_chan(column, chunk=CHUNK):
    """The kernel's scheme on one float32 column, in NumPy float64: chunks of ``chunk`` values summed as d = x - k and d^2 with k the
    chunk's first value, turned into (n, mean - anchor, M2) with anchor = the column's first value, merged pairwise in a fixed tree
    by ``chan``; the anchor comes back at the end.  Returns (n, mean, M2)."""
    x = np.asarray(column, dtype=np.float32).reshape(-1).astype(np.float64)
    anchor = float(x[0])
    parts = []
    for lo in range(0, x.size, chunk):
        block = x[lo:lo + chunk]
        k = float(block[0])
        s1 = s2 = 0.0
        for v in block:
            d = float(v) - k
            s1 += d
            s2 += d * d
        n = float(block.size)
        m2 = s2 - s1 * s1 / n
        parts.append((n, (k - anchor) + s1 / n, m2 if not m2 < 0.0 else 0.0))
    while len(parts) > 1:
        half = (len(parts) + 1) // 2
        parts = [chan(parts[i], parts[i + half]) if i + half < len(parts) else parts[i] for i in range(half)]
    n, mean, m2 = parts[0]
    return n, anchor + mean, m2


def bounds(all_items, count, n_batches=1):
    """(bound_mean, bound_var), each (D,) or broadcastable to ``count`` (groups, D): see the module docstring.  ``all_items``: every
    item any of the calls was given; ``count``: the statistic's count."""
    rows = np.concatenate([np.asarray(x, dtype=np.float64) for x in all_items if len(x)], axis=0)
    finite = np.where(np.isfinite(rows), rows, np.nan)
    with np.errstate(all='ignore'):
        spread = np.nanmax(finite, axis=0) - np.nanmin(finite, axis=0)
        largest = np.nanmax(np.abs(finite), axis=0)
    log_n = np.log2(np.maximum(np.asarray(count, dtype=np.float64), 2.0))
    nb = float(n_batches)
    h, g = DEPTH + nb, STAGES + nb
    e = U * spread * ((CHUNK + 2) + 3 * h)
    bound_mean = (2 * nb + log_n + 2) * U * largest + e
    bound_var = (U * spread ** 2 * ((3 * CHUNK + 5) + 4 * h + 4 * g * ((CHUNK + 2) + 3 * h) + log_n + 5)
                 + (nb - 1) * spread * (nb * U * largest + 2 * e))
    return bound_mean, bound_var


def adversarial_column(n=2113, seed=0):
    """float32(2^20) + k / 8, k uniform in 0..7: values near 2^20 that differ by multiples of 1 / 8 (all exact in float32)."""
    k = np.random.RandomState(seed).randint(0, 8, size=n)
    return (np.float32(2.0 ** 20) + k.astype(np.float32) / np.float32(8.0)).astype(np.float32)
