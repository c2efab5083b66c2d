"""An independent reference of the frame-level positional features (data.frame_counters, csrc/counters.hip): plain Python integers
and ``fractions.Fraction`` per frame, every value rounded to float32 from the EXACT rational (round to nearest, ties to even, done on
the integers here), not through float64 and not with the arithmetic of morgana_amd/data.py.

Definition (the issue's): d[p][s] integer durations, segments in (p, s) order, start = the sum of the durations before a segment,
n_s = d[p][s], n_p = sum_s d[p][s]; frame t of segment (p, s): i = t - start[p][s], j = t - start[p][0].
'full':  (i+1)/n_s, (n_s-i)/n_s, n_s, s+1, S-s, n_p, n_s/n_p, (n_p-j)/n_p, (j+1)/n_p.      'phone': (j+1)/n_p, (n_p-j)/n_p, n_p."""
import math
from fractions import Fraction

import numpy as np

COLUMNS = {'full': 9, 'phone': 3}


def to_f32(q):
    """The float32 nearest to the positive rational ``q`` (ties to even), exactly; q is far inside the normal range here."""
    q = Fraction(q)
    assert q > 0
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1) and -100 < e < 100
    scaled = q / Fraction(2) ** (e - 23)                  # in [2^23, 2^24)
    m = scaled.numerator // scaled.denominator
    rest = scaled - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and m % 2 == 1):
        m += 1
    value = np.float32(math.ldexp(m, e - 23))             # m <= 2^24: exact in float32
    assert Fraction(float(value)) == Fraction(m) * Fraction(2) ** (e - 23)
    return value


def _grid(dur, n_phones=None):
    """Durations as a list of P lists of S python ints, a negative one and every phone from ``n_phones`` on counting as 0."""
    d = np.asarray(dur)
    if d.ndim == 1:
        d = d.reshape(-1, 1)
    grid = [[max(int(v), 0) for v in row] for row in d]
    if n_phones is not None:
        for p in range(max(int(n_phones), 0), len(grid)):
            grid[p] = [0] * len(grid[p])
    return grid


def total(dur, n_phones=None):
    return sum(sum(row) for row in _grid(dur, n_phones))


def rows(dur, kind, frames=None, n_phones=None):
    """(len(frames), C) float32: the counters of the given frames (default: every frame) of one item."""
    grid = _grid(dur, n_phones)
    n_states = len(grid[0]) if grid else 1
    segments, at = [], 0                                  # (start, n_s, p, s, start of the phone, n_p) of every segment that owns a frame
    for p, row in enumerate(grid):
        phone_start, n_p = at, sum(row)
        for s, n_s in enumerate(row):
            if n_s > 0:
                segments.append((at, n_s, p, s, phone_start, n_p))
            at += n_s
    frames = range(at) if frames is None else list(frames)
    out = np.zeros((len(frames), COLUMNS[kind]), dtype=np.float32)
    k = 0
    for r, t in enumerate(frames):
        assert 0 <= t < at
        if k >= len(segments) or t < segments[k][0]:
            k = 0
        while not segments[k][0] <= t < segments[k][0] + segments[k][1]:
            k += 1
        start, n_s, p, s, phone_start, n_p = segments[k]
        i, j = t - start, t - phone_start
        if kind == 'full':
            out[r] = (to_f32(Fraction(i + 1, n_s)), to_f32(Fraction(n_s - i, n_s)), to_f32(n_s), to_f32(s + 1), to_f32(n_states - s),
                      to_f32(n_p), to_f32(Fraction(n_s, n_p)), to_f32(Fraction(n_p - j, n_p)), to_f32(Fraction(j + 1, n_p)))
        else:
            out[r] = (to_f32(Fraction(j + 1, n_p)), to_f32(Fraction(n_p - j, n_p)), to_f32(n_p))
    return out


def padded(durs, kind, t, seq_len=None, n_phones=None):
    """(B, t, C) float32 of a batch (``durs``: (B, P, S) or (B, P) integers): frames below min(t, total_b, seq_len[b]) hold the counters,
    all others zeros."""
    out = np.zeros((len(durs), t, COLUMNS[kind]), dtype=np.float32)
    for b, dur in enumerate(durs):
        used = None if n_phones is None else n_phones[b]
        valid = min(t, total(dur, used))
        if seq_len is not None:
            valid = min(valid, max(int(seq_len[b]), 0))
        out[b, :valid] = rows(dur, kind, frames=range(valid), n_phones=used)
    return out


def random_durations(rng, n_phones, n_states, high=40):
    """(P, S) int64 in 0..high, about one in seven zero; with P >= 4 a zero-length phone and, with S > 1, phones whose first, middle and last
    state is empty."""
    d = rng.randint(1, high + 1, size=(n_phones, n_states)).astype(np.int64)
    d[rng.rand(n_phones, n_states) < 0.15] = 0
    if n_phones >= 4:
        d[3, :] = 0                                       # a zero-length phone
        if n_states > 1:
            d[0, 0] = 0                                   # a zero-length state at the start of a phone
            d[1, n_states - 1] = 0                        # ... at the end
            d[2, n_states // 2] = 0                       # ... in the middle
            d[0, 1], d[1, 0], d[2, 0] = 3, 1, 2           # (those phones are not empty)
    return d
