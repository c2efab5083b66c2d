"""An independent reference for the delta features (mg_deltas_f32, data.compute_deltas): an explicit loop over frames, windows, columns
and taps in exact rational arithmetic - ``fractions.Fraction`` of the float32 inputs and of the double coefficients - and the bounds a
result is held to.  Nothing here looks at what the code under test returns, and nothing is shared with it.

Per output element the reference gives the exact value, its correctly rounded float32 and S = sum_k |c_k x_k|.

Bounds.  The code under test accumulates in float64 (unit roundoff 2^-53) and rounds the sum once to float32 (2^-24):
  general windows   |got - exact| <= 2^-24 |exact| + 2^-50 S.  At most 5 products and 4 additions, each within 2^-53 relative of its
                    exact result: the float64 sum is within (1 + 2^-53)^5 - 1 < 2^-50 of S away from exact (S bounds every partial
                    sum); the float32 rounding adds half an ulp, at most 2^-24 of the value it rounds.
  default windows   coefficients 1, +-0.5, -2 are powers of two: every product is exact, and while the exponents of the data span
                    fewer than 29 bits (``exponent_span``) every partial sum - a multiple of 2^(emin - 24) below 2^(emax + 3) - has at
                    most 53 significant bits and is exact too.  ``got`` must then BE the correctly rounded float32.  The same holds
                    for any window of one coefficient 1 (the static window).
Results that are subnormal in float32 are outside both statements; the test data (N(5, 2)) has none.
"""
import math
from fractions import Fraction

import numpy as np

DEFAULT_WINDOWS = ((0, 0, (1.0,)), (1, 1, (-0.5, 0.0, 0.5)), (1, 1, (1.0, -2.0, 1.0)))
STATIC_WINDOW = ((0, 0, (1.0,)),)
WINDOWS_5PT = ((0, 0, (1.0,)), (2, 2, (-0.2, -0.1, 0.0, 0.1, 0.2)), (1, 1, (1.0, -2.0, 1.0)))      # test_gpu_parity.MLPG_WINDOWS_5PT
U32, U64 = Fraction(1, 2 ** 24), Fraction(1, 2 ** 50)


def round_f32(value):
    """The float32 nearest to the rational ``value``, ties to even.  Going through the nearest float64 rounds twice, which differs only
    where that float64 sits exactly half way between two float32: those values are decided in rational arithmetic."""
    if value == 0:
        return np.float32(0.0)
    near = float(value)
    guess = np.float32(near)
    if float(guess) == near:
        return guess
    other = np.nextafter(guess, np.float32(np.inf if near > float(guess) else -np.inf))
    if abs(near - float(guess)) != abs(float(other) - near):
        return guess
    best, best_miss = None, None
    for cand in (guess, other):
        miss = abs(Fraction(float(cand)) - value)
        even = (np.float32(cand).view(np.uint32) & 1) == 0
        if best is None or miss < best_miss or (miss == best_miss and even):
            best, best_miss = np.float32(cand), miss
    return best


def reference(x, windows, edge):
    """x (len, D) float32 -> (exact, rounded, S): (len, W*D) arrays of Fraction, float32 and Fraction.  Column w*D + d at frame t is
    sum_k c[w][k] x[t - l_w + k, d]; a tap outside [0, len) reads frame 0 / len - 1 (edge 'replicate') or is left out ('zero')."""
    assert x.dtype == np.float32 and x.ndim == 2 and edge in ('replicate', 'zero')
    n, d = x.shape
    width = len(windows) * d
    exact = np.empty((n, width), dtype=object)
    total = np.empty((n, width), dtype=object)
    rounded = np.zeros((n, width), dtype=np.float32)
    rational = [[Fraction(float(v)) for v in row] for row in x]
    size = [[abs(v) for v in row] for row in rational]
    coefficients = [[Fraction(float(c)) for c in coeff] for _, _, coeff in windows]
    for t in range(n):
        for w, (l, u, coeff) in enumerate(windows):
            assert len(coeff) == l + u + 1
            taps = []
            for k, c in enumerate(coefficients[w]):
                tap = t - l + k
                if tap < 0 or tap >= n:
                    if edge == 'zero':
                        continue
                    tap = 0 if tap < 0 else n - 1
                if c != 0:                                # a zero coefficient adds an exact zero to both sums
                    taps.append((c, abs(c), tap))
            for col in range(d):
                value = sum((c * rational[tap][col] for c, _, tap in taps), Fraction(0))
                exact[t, w * d + col] = value
                total[t, w * d + col] = sum((a * size[tap][col] for _, a, tap in taps), Fraction(0))
                rounded[t, w * d + col] = round_f32(value)
    return exact, rounded, total


def exponent_span(x):
    """emax - emin + 1 over the non-zero entries of x (0 for none): the number of binary exponents the data touches."""
    values = np.abs(np.asarray(x, dtype=np.float64).reshape(-1))
    values = values[values > 0]
    if values.size == 0:
        return 0
    exponents = np.frexp(values)[1]
    return int(exponents.max() - exponents.min() + 1)


def exact_windows(windows):
    """True if every coefficient is 0 or a signed power of two: the products are then exact in float64."""
    return all(c == 0 or math.frexp(abs(c))[0] == 0.5 for _, _, coeff in windows for c in coeff)


def misses(got, ref, must_be_rounded):
    """The (frame, column) positions at which ``got`` (len, W*D) float32 breaks its bound: not the correctly rounded float32
    (``must_be_rounded``), or further from exact than 2^-24 |exact| + 2^-50 S.  An element that IS the correctly rounded value is
    inside the general bound by construction (half an ulp of a normal float32 is at most 2^-24 of the value), so only the others are
    checked in rational arithmetic."""
    exact, rounded, total = ref
    assert got.shape == rounded.shape and got.dtype == np.float32
    differ = np.argwhere(~((got == rounded) | (np.isnan(got) & np.isnan(rounded))))
    if must_be_rounded:
        return [tuple(p) for p in differ]
    bad = []
    for t, col in differ:
        value = got[t, col]
        if not np.isfinite(value) or abs(Fraction(float(value)) - exact[t, col]) > U32 * abs(exact[t, col]) + U64 * total[t, col]:
            bad.append((t, col))
    return bad


def residual(ref):
    """rounded - exact as float64 (len, W*D): the float32 rounding residual of the observations."""
    exact, rounded, _ = ref
    out = np.zeros(rounded.shape)
    for t in range(rounded.shape[0]):
        for col in range(rounded.shape[1]):
            out[t, col] = float(Fraction(float(rounded[t, col])) - exact[t, col])
    return out


def window_matrices(windows, n):
    """W_w (n, n) of morgana/viz/synthesis.py:8-36 as dense float64 arrays: row t holds coeff[k] at column t - l + k where that is a
    frame."""
    mats = []
    for l, u, coeff in windows:
        mat = np.zeros((n, n))
        for t in range(n):
            for k, c in enumerate(coeff):
                if 0 <= t - l + k < n:
                    mat[t, t - l + k] = c
        mats.append(mat)
    return mats
