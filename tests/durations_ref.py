"""An independent reference of the duration quantiser (data.quantise_durations, csrc/durations.hip): python floats and ``math`` up to
the 16-bit fixed-point value, python integers from there on, one item at a time, and the SEQUENTIAL emit rule

    emit d_i = max(lo, R_i - the frames emitted so far),    R_i = (q_0 + .. + q_i + 32768) >> 16

not the closed form with a running maximum that the kernel and the NumPy host form use.

Definition (the issue's): segments i = 0 .. n-1 in (p, s) order over the valid phones.  x_i = pred * p1[s] + p0[s] in float64 (the
product of two float32 is exact there: one rounding), exp(x_i) if log_input, times scale; NaN, infinite or negative -> 0 (flag bit 0);
min(x_i, hi); q_i = floor(x_i * 65536 + 0.5).  With total: Q = sum q_i; Q > 0 and total > 0: q_i = min(floor(float(q_i) *
(float(total << 16) / float(Q)) + 0.5), hi << 16), else flag bit 1.  'nearest': d_i = max(lo, (q_i + 32768) >> 16).  'carry': the rule
above; flag bit 2 when the frames emitted differ from (sum q_i + 32768) >> 16.  An item that names no parameter row: zeros, flag bit 3.

The only step that is not correctly rounded arithmetic is ``exp``: two libraries may differ in its last places.  A segment is DECIDED
when x_i * 65536 lies further than 8 * 2^-52 * x_i * 65536 + 2^-40 from every half-integer (and x_i as far from ``hi``), so that any exp
within 8 units in the last place gives the same q_i; ``Result.undecided`` counts the others.  Without log_input every segment is
decided by construction."""
import math

import numpy as np

INVALID, NO_FIT, PUSHED, NO_ROW = 1, 2, 4, 8
MAX_FRAMES = 2 ** 20


class Result(object):
    def __init__(self, dur, phone_dur, n_frames, flags, undecided, fixed):
        self.dur, self.phone_dur, self.n_frames, self.flags, self.undecided, self.fixed = dur, phone_dur, n_frames, flags, undecided, fixed


def _value(v, p0, p1, log_input, scale):
    """x_i before the clamps, as a python float (inf where exp overflows)."""
    x = float(v)
    if p0 is not None:
        x = float(v) * float(p1) + float(p0)
    if log_input:
        try:
            x = math.exp(x)
        except OverflowError:
            x = math.inf
    return x * scale


def _undecided(x, hi):
    """x (finite, >= 0, before min(x, hi)) could round to another q_i - or be clamped or not - under an exp 8 ulp away."""
    slack = 8 * 2.0 ** -52 * x
    if abs(x - hi) <= slack:
        return True
    y = min(x, float(hi)) * 65536.0
    return abs((y - math.floor(y)) - 0.5) <= slack * 65536.0 + 2.0 ** -40


def sequential(q, lo):
    """The emit rule on fixed-point values -> (durations, frames emitted)."""
    out, emitted, run = [], 0, 0
    for v in q:
        run += v
        d = max(lo, ((run + 32768) >> 16) - emitted)
        out.append(d)
        emitted += d
    return out, emitted


def closed_form(q, lo):
    """E_i = (i+1) lo + max(0, max_{j<=i}(R_j - (j+1) lo)), d_i = E_i - E_{i-1}: what the kernel computes, in python integers."""
    out, run, best, before = [], 0, 0, 0
    for i, v in enumerate(q):
        run += v
        best = max(best, ((run + 32768) >> 16) - (i + 1) * lo)
        end = (i + 1) * lo + best
        out.append(end - before)
        before = end
    return out, before


def item(pred, n_phones=None, p0=None, p1=None, log_input=False, scale=1.0, lo=1, hi=MAX_FRAMES, rounding='carry', total=None):
    """One item: ``pred`` (P,) or (P, S) float32, p0 / p1 (S,) or None -> Result with dur (P, S) and phone_dur (P,) int64 arrays."""
    pred = np.asarray(pred, dtype=np.float32)
    pred = pred.reshape(pred.shape[0], -1)
    n_all, n_states = pred.shape
    used = n_all if n_phones is None else min(max(int(n_phones), 0), n_all)
    flags, undecided, q = 0, 0, []
    for p in range(used):
        for s in range(n_states):
            x = _value(pred[p, s], None if p0 is None else p0[s], None if p0 is None else p1[s], log_input, float(scale))
            if math.isnan(x) or math.isinf(x) or x < 0.0:
                x = 0.0
                flags |= INVALID
            elif log_input and _undecided(x, hi):
                undecided += 1
            x = min(x, float(hi))
            q.append(int(math.floor(x * 65536.0 + 0.5)))
    if total is not None:
        whole = sum(q)
        if whole > 0 and int(total) > 0:
            ratio = float(int(total) << 16) / float(whole)
            q = [min(int(math.floor(float(v) * ratio + 0.5)), hi << 16) for v in q]
        else:
            flags |= NO_FIT
    if rounding == 'carry':
        d, emitted = sequential(q, lo)
        if emitted != (sum(q) + 32768) >> 16:
            flags |= PUSHED
    else:
        assert rounding == 'nearest'
        d = [max(lo, (v + 32768) >> 16) for v in q]
    dur = np.zeros((n_all, n_states), dtype=np.int64)
    dur.reshape(-1)[:len(d)] = d
    return Result(dur, dur.sum(axis=1), int(dur.sum()), flags, undecided, q)


def batch(pred, n_phones=None, p0=None, p1=None, item_row=None, total=None, **kwargs):
    """A batch (B, P) or (B, P, S) -> (dur shaped like pred, phone_dur (B, P), n_frames (B,) int64, flags (B,) int32, undecided).  With
    ``item_row`` p0 / p1 are (rows, S) tables; an item whose index names no row gives zeros and NO_ROW."""
    pred = np.asarray(pred, dtype=np.float32)
    shape = pred.shape
    pred = pred.reshape(shape[0], shape[1], -1)
    dur = np.zeros(pred.shape, dtype=np.int64)
    phone_dur = np.zeros(pred.shape[:2], dtype=np.int64)
    n_frames, flags, undecided = np.zeros(shape[0], dtype=np.int64), np.zeros(shape[0], dtype=np.int32), 0
    for b in range(shape[0]):
        q0, q1 = p0, p1
        if item_row is not None:
            row = int(item_row[b])
            if not 0 <= row < len(p0):
                flags[b] = NO_ROW
                continue
            q0, q1 = p0[row], p1[row]
        res = item(pred[b], None if n_phones is None else n_phones[b], q0, q1, total=None if total is None else int(total[b]), **kwargs)
        dur[b], phone_dur[b], n_frames[b], flags[b] = res.dur, res.phone_dur, res.n_frames, res.flags
        undecided += res.undecided
    return dur.reshape(shape), phone_dur, n_frames, flags, undecided
