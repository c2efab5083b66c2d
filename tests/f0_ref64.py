"""Extended-precision restatement of the continuous log-F0 operator (csrc/f0.hip, K29; data.continuous_lf0), the reference of
tests/test_f0_host.py and tests/test_gpu_f0.py, the per-element bound both forms are held to, and the voicing patterns they share.

The operator, per item of n frames and per column: voiced[t] = x[t] > voiced_above (float32 comparison; a NaN is unvoiced);
l[t] = log(x[t]) (x[t] itself with log_input); on a voiced frame the value is l[t]; on an unvoiced frame between the nearest voiced
frames a < t < b it is l[a] + (l[b] - l[a]) * ((t - a) / (b - a)); before the first voiced frame l[first], behind the last l[last];
`fill` when the item has no voiced frame.  ``reference`` evaluates this in np.longdouble (x87 80-bit: 64 significant bits), the
logarithm in long double as well, the neighbours found by a plain Python loop over the frames.

The bound, per element, derived from the number formats alone (nothing is fitted to what a kernel returns).  u = 2^-53.
Let M = max(|l[a]|, |l[b]|) of the two neighbours an element uses (|l[t]| on a voiced frame, 0 for `fill`).

  * the logarithm.  A float64 `log` is documented as good to 1 ulp (ROCm's device library, glibc's libm); nobody has measured the
    device's on this chip, so 2 ulp are allowed: every l the form under test uses is off by at most 2 ulp(l) <= 4 u |l| <= 4 u M.
    The interpolated value is a convex combination of l[a] and l[b] (0 < w < 1), so these input errors move it by at most 4 u M.
    With log_input there is no logarithm: this term is 0.
  * the interpolation, four roundings in float64: w = (t - a) / (b - a) (both operands exact integers; |l[b] - l[a]| <= 2 M, so the
    error of w moves the value by <= 2 u M), the difference l[b] - l[a] (<= 2 u M), the product (<= 2 u M), the sum (|value| <= M:
    <= u M): 7 u M to first order, 8 u M with the second-order terms and the reference's own 2^-64 relative error.
    A voiced frame, an edge frame and a filled frame have no interpolation: this term is 0.
  * one rounding of the float64 value v' to float32: <= 2^-24 |v'| <= 2^-24 (|ref| + E), E the sum of the two float64 terms.

        bound = 2^-24 |ref| + (1 + 2^-24) E,     E = (4 [log] + 8 [interpolated]) u M

`vuv`, the zeros of pad frames and `fill` are exact (bound 0: `fill` is a float32, M = 0).  There is no undecided set: every element
has a bound and is inside it or not."""
import numpy as np

U = 2.0 ** -53
LOG_ULPS = 2                     # allowed error of a float64 log, in ulp (documented: 1)
EPS32 = 2.0 ** -24


def threshold(voiced_above=None, log_input=False):
    """The float32 voicing threshold: the operator's defaults, 0 for a raw track and -1e9 for a log track."""
    if voiced_above is None:
        voiced_above = -1e9 if log_input else 0.0
    return np.float32(voiced_above)


def reference(x, log_input=False, voiced_above=None, fill=0.0):
    """(ref, vuv, scale, interpolated) of one (n, D) float32 item: the operator's value in np.longdouble, the voicing flag as float32,
    M = max(|l[a]|, |l[b]|) of the neighbours each element uses as float64, and whether the element is an interpolated one."""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 2
    n, d = x.shape
    above = threshold(voiced_above, log_input)
    ref = np.zeros((n, d), dtype=np.longdouble)
    vuv = np.zeros((n, d), dtype=np.float32)
    scale = np.zeros((n, d), dtype=np.float64)
    interpolated = np.zeros((n, d), dtype=bool)
    for c in range(d):
        column = x[:, c]
        voiced = [bool(column[t] > above) for t in range(n)]
        with np.errstate(all='ignore'):
            wide = column.astype(np.longdouble)
            logs = wide if log_input else np.log(np.where(voiced, wide, np.longdouble(1)))
        if not any(voiced):
            ref[:, c] = np.longdouble(np.float32(fill))
            continue
        before, last = [], -1                               # the nearest voiced frame before t ...
        for t in range(n):
            before.append(last)
            if voiced[t]:
                last = t
        after, nxt = [-1] * n, -1                           # ... and after it
        for t in range(n - 1, -1, -1):
            after[t] = nxt
            if voiced[t]:
                nxt = t
        for t in range(n):
            if voiced[t]:
                vuv[t, c] = 1.0
                ref[t, c], scale[t, c] = logs[t], abs(float(logs[t]))
                continue
            a, b = before[t], after[t]
            if a < 0:
                ref[t, c], scale[t, c] = logs[b], abs(float(logs[b]))
            elif b < 0:
                ref[t, c], scale[t, c] = logs[a], abs(float(logs[a]))
            else:
                w = np.longdouble(t - a) / np.longdouble(b - a)
                ref[t, c] = logs[a] + (logs[b] - logs[a]) * w
                scale[t, c] = max(abs(float(logs[a])), abs(float(logs[b])))
                interpolated[t, c] = True
    return ref, vuv, scale, interpolated


def bound(ref, scale, interpolated, log_input=False):
    """The per-element bound of the module docstring, float64."""
    ulps = (0.0 if log_input else 2.0 * LOG_ULPS) + 8.0 * np.asarray(interpolated, dtype=np.float64)
    err64 = ulps * U * scale
    return EPS32 * np.abs(ref).astype(np.float64) + (1.0 + EPS32) * err64


def misses(got, ref, limit):
    """[(index, got, ref, bound)] of the elements of ``got`` (float32) outside |got - ref| <= bound; a NaN is a miss."""
    got = np.asarray(got, dtype=np.float32)
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    bad = ~(err <= limit)
    return [(tuple(int(i) for i in at), float(got[tuple(at)]), float(ref[tuple(at)]), float(limit[tuple(at)])) for at in np.argwhere(bad)]


def worst_ratio(got, ref, limit):
    """max |got - ref| / bound over the elements with a positive bound (0 if there is none)."""
    err = np.abs(np.asarray(got, dtype=np.float32).astype(np.longdouble) - ref).astype(np.float64)
    with np.errstate(all='ignore'):
        ratio = np.where(limit > 0, err / np.where(limit > 0, limit, 1.0), 0.0)
    return float(ratio.max()) if ratio.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- the shared cases
def _pattern_flags(chunk):
    """{length: [(pattern name, voiced flags)]}: every voicing pattern the tests name, for the lengths 0, 1, 2, 63, 64, 65 and
    2 * chunk + 1 (one frame longer than two trips of a workgroup)."""
    long = 2 * chunk + 1
    v, u = True, False

    def flags(length, voiced_at=(), default=u):
        out = np.full(length, default, dtype=bool)
        for at in voiced_at:
            out[at] = not default
        return out

    gaps = np.ones(long, dtype=bool)                        # gaps of exactly 64, 65 and chunk + 1 frames between voiced stretches
    at = 7
    for width in (64, 65, chunk + 1):
        gaps[at:at + width] = u
        at += width + 5
    assert at <= long
    edge_gap = np.ones(long, dtype=bool)                    # a gap that starts on the last frame of a chunk
    edge_gap[chunk - 1:chunk + 40] = u
    lead_trail_long = np.zeros(long, dtype=bool)            # the first voiced frame more than a chunk in: a walk over several segments
    lead_trail_long[chunk + 70:chunk + 90] = v
    return {
        0: [('empty', flags(0))],
        1: [('one voiced', flags(1, default=v)), ('one unvoiced', flags(1))],
        2: [('voiced, unvoiced', np.array([v, u])), ('unvoiced, voiced', np.array([u, v])), ('two unvoiced', flags(2)),
            ('two voiced', flags(2, default=v))],
        63: [('all voiced', flags(63, default=v)), ('alternating', np.arange(63) % 2 == 0),
             ('leading and trailing unvoiced', flags(63, range(20, 41)))],
        64: [('all unvoiced', flags(64)), ('voiced at the first frame only', flags(64, [0])),
             ('voiced at the last frame only', flags(64, [63]))],
        65: [('voiced at a middle frame only', flags(65, [31])), ('alternating from unvoiced', np.arange(65) % 2 == 1),
             ('ends unvoiced behind a full wave', flags(65, [64], default=v))],
        long: [('gaps of 64, 65 and chunk + 1', gaps), ('a gap from the last frame of a chunk', edge_gap),
               ('voiced at frames 0 and n - 1 only', flags(long, [0, long - 1])), ('all unvoiced, long', flags(long)),
               ('voiced at a middle frame only, long', flags(long, [chunk + 3])), ('leading and trailing runs over chunks', lead_trail_long)],
    }


def case(width, chunk, seed=0):
    """(items, names): float32 (len, width) raw F0 tracks and, per item, the pattern names of its columns.  Item j of a length takes
    pattern (j + c) of that length in column c, so the columns of an item differ in their voicing and at width 1 every pattern
    appears.  Voiced frames are 60 .. 420 Hz; unvoiced ones are 0, or - every fifth of them - NaN or a negative value, so NaN and
    negative entries also sit inside voiced stretches (the alternating patterns).  The order puts an item that ends unvoiced directly
    in front of one that starts voiced, and the reverse pair (``adjacent_pairs``)."""
    rng = np.random.RandomState(9000 + 17 * width + seed)
    patterns = _pattern_flags(chunk)
    items, names = [], []
    for length in (63, 0, 64, 1, 65, 2, 2 * chunk + 1):
        pats = patterns[length]
        for j in range(len(pats)):
            x = np.zeros((length, width), dtype=np.float32)
            picked = []
            for c in range(width):
                name, flags = pats[(j + c) % len(pats)]
                picked.append(name)
                column = (60.0 + 360.0 * rng.rand(length)).astype(np.float32)
                odd = rng.randint(0, 5, size=length) == 0
                junk = np.where(rng.rand(length) < 0.5, np.float32(np.nan), np.float32(-3.5))
                x[:, c] = np.where(flags, column, np.where(odd, junk, np.float32(0.0)))
            x.setflags(write=False)
            items.append(x)
            names.append(tuple(picked))
    return tuple(items), tuple(names)


def log_case(items):
    """The same tracks as log-F0 tracks in the HTS / Merlin convention: float32(log x) where voiced, -1e10 where unvoiced (the NaN
    entries stay NaN)."""
    out = []
    for x in items:
        with np.errstate(all='ignore'):
            y = np.where(x > 0, np.log(np.where(x > 0, x, 1.0).astype(np.float64)).astype(np.float32),
                         np.where(np.isnan(x), np.float32(np.nan), np.float32(-1e10))).astype(np.float32)
        y.setflags(write=False)
        out.append(y)
    return tuple(out)


def adjacent_pairs(items, column=0):
    """(an item ending unvoiced directly followed by one starting voiced, the reverse pair): do both occur in ``column``?"""
    ends_u_starts_v = ends_v_starts_u = False
    rows = [x for x in items if len(x)]                     # (an empty item between two others has no rows: they still touch)
    for left, right in zip(rows[:-1], rows[1:]):
        end, start = bool(left[-1, column] > 0), bool(right[0, column] > 0)
        ends_u_starts_v |= (not end) and start
        ends_v_starts_u |= end and (not start)
    return ends_u_starts_v, ends_v_starts_u
