#!/usr/bin/env python
"""What generation under a global-variance prior costs, on a resident 64 x 1000 batch with padding 100 (the shipped models' call); the
method of scripts/bench_mlpg_grad.py.

ops.mlpg and ops.mlpg_gv (csrc/mlpg_gv.hip) under global variances for D = 1, 5, 60 (lf0, bap, mcep) by device events: --repeats
rounds, each timing the two in turn over a window of --calls calls; the median and the spread of the rounds.  The prior is
mu_v = --factor x v(x0) of every system itself (per item), sigma_v = 0.1 mu_v, as the tests draw it.  The yardsticks are ops.mlpg of the
same run and (evaluations x ops.mlpg): every evaluation of the root search is one banded solve with two right-hand sides, and a wave
runs for as long as its slowest system searches, so the evaluations are reported as mean and maximum over the systems.
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from morgana_amd import losses, ops  # noqa: E402
from morgana_amd.viz import synthesis  # noqa: E402

DEV = 'cuda:0'
B, T, PADDING = 64, 1000, 100
STREAMS = (('lf0', 1), ('bap', 5), ('mcep', 60))


def window(fn, calls):
    """Milliseconds per call of ``fn`` over one event-timed window of ``calls`` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=10, help='calls per timed window')
    ap.add_argument('--repeats', type=int, default=5, help='rounds per measurement')
    ap.add_argument('--factor', type=float, nargs='+', default=[2.0, 0.5], help='mu_v as a multiple of v(x0)')
    ap.add_argument('--max-iter', type=int, default=48)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mlpg_gv.py needs an MI355X: there is no CPU path to time')
    for name, d in STREAMS:
        g = torch.Generator(device=DEV).manual_seed(d)
        means = torch.randn(B, T, 3 * d, device=DEV, generator=g)
        var = (torch.rand(3 * d, device=DEV, generator=g) * 0.4 + 0.2) ** 2
        seq = torch.full((B,), T, dtype=torch.int64, device=DEV)
        plain = lambda: ops.mlpg(means, var, synthesis.DEFAULT_WINDOWS, padding_size=PADDING, seq_len=seq)      # noqa: E731
        v0 = losses.global_variance(plain(), seq)
        for factor in args.factor:
            gv_mean = factor * v0
            gv_variance = (0.1 * gv_mean) ** 2
            with_gv = lambda **kw: ops.mlpg_gv(means, var, gv_mean, gv_variance, synthesis.DEFAULT_WINDOWS, padding_size=PADDING,      # noqa: E731
                                               seq_len=seq, max_iter=args.max_iter, **kw)
            info = with_gv(want_info=True)[1].cpu().numpy()
            for fn in (plain, with_gv):
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            rounds = {'mlpg': [], 'mlpg_gv': []}
            for _ in range(args.repeats):                   # the two in turn inside every round: drift hits them alike
                rounds['mlpg'].append(window(plain, args.calls))
                rounds['mlpg_gv'].append(window(with_gv, args.calls))
            med = {what: float(np.median(v)) for what, v in rounds.items()}
            evals = info[:, :, 2]
            print(json.dumps({'stream': name, 'D': d, 'systems': B * d, 'unknowns': T + 2 * PADDING, 'factor': factor,
                              'mlpg_ms': round(med['mlpg'], 4), 'mlpg_gv_ms': round(med['mlpg_gv'], 4),
                              'mlpg_gv_min': round(min(rounds['mlpg_gv']), 4), 'mlpg_gv_max': round(max(rounds['mlpg_gv']), 4),
                              'evaluations_mean': round(float(evals.mean()), 2), 'evaluations_max': int(evals.max()),
                              'fallbacks': int(info[:, :, 3].sum()), 'over_mlpg': round(med['mlpg_gv'] / med['mlpg'], 2),
                              'over_max_evaluations_x_mlpg': round(med['mlpg_gv'] / (evals.max() * med['mlpg']), 3),
                              'calls': args.calls, 'repeats': args.repeats}))


if __name__ == '__main__':
    main()
