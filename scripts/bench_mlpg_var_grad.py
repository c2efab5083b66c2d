#!/usr/bin/env python
"""What the variance gradient of MLPG costs, on a resident 64 x 1000 batch with padding 100 (the shipped models' call); the method of
scripts/bench_mlpg_grad.py.

    bench_mlpg_var_grad.py kernels  ops.mlpg, ops.mlpg_backward and ops.mlpg_backward_mv under per-frame variances for D = 1, 5, 60
                                    (lf0, bap, mcep) by device events: --repeats rounds, each timing the three in turn over a window of
                                    --calls calls; the median and the spread of the rounds.  The yardstick of the new backward is the
                                    means-only backward of the same run.
    bench_mlpg_var_grad.py steps    the f0gru training step (forward, backward, Adam; eager launches, bf16 as bench.py runs it) at
                                    trajectory_weight=1 with predict_variance False and True
    bench_mlpg_var_grad.py trace    the calls of `kernels`, a few of each and nothing else: run it under
                                    `rocprofv3 --kernel-trace --stats -- python scripts/bench_mlpg_var_grad.py trace`, a run of its
                                    own, for the per-kernel times (mlpg_band_pair_kernel, mlpg_solve_pair_kernel, mlpg_fold_mv_kernel,
                                    mlpg_fold_mv_edge_kernel next to the means-only ones)
Prints one JSON line per measurement."""
import argparse
import gc
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from morgana_amd import data, models, ops, optim, synthetic  # noqa: E402
from morgana_amd import functional as F_hip  # noqa: E402
from morgana_amd.viz import synthesis  # noqa: E402

DEV = 'cuda:0'
B, T, PADDING = 64, 1000, 100
STREAMS = (('lf0', 1), ('bap', 5), ('mcep', 60))
OPS = ('mlpg', 'mlpg_backward', 'mlpg_backward_mv')


def window(fn, calls):
    """Milliseconds per call of ``fn`` over one event-timed window of ``calls`` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def kernel_inputs(d):
    g = torch.Generator(device=DEV).manual_seed(d)
    means = torch.randn(B, T, 3 * d, device=DEV, generator=g)
    grad_out = torch.randn(B, T, d, device=DEV, generator=g)
    var = (torch.rand(B, T, 3 * d, device=DEV, generator=g) * 0.4 + 0.2) ** 2
    seq = torch.full((B,), T, dtype=torch.int64, device=DEV)
    forward = lambda: ops.mlpg(means, var, synthesis.DEFAULT_WINDOWS, padding_size=PADDING, seq_len=seq)                          # noqa: E731
    backward = lambda: ops.mlpg_backward(grad_out, var, synthesis.DEFAULT_WINDOWS, padding_size=PADDING, seq_len=seq)             # noqa: E731
    both = lambda: ops.mlpg_backward_mv(grad_out, means, var, synthesis.DEFAULT_WINDOWS, padding_size=PADDING, seq_len=seq)       # noqa: E731
    return forward, backward, both


def kernels(args):
    for name, d in STREAMS:
        fns = kernel_inputs(d)
        for fn in fns:
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        rounds = {what: [] for what in OPS}
        for _ in range(args.repeats):                       # the three in turn inside every round: drift hits them alike
            for what, fn in zip(OPS, fns):
                rounds[what].append(window(fn, args.calls))
        medians = {what: float(np.median(v)) for what, v in rounds.items()}
        for what in OPS:
            print(json.dumps({'op': what, 'stream': name, 'D': d, 'systems': B * d, 'unknowns': T + 2 * PADDING,
                              'ms_per_call': round(medians[what], 4), 'min': round(min(rounds[what]), 4), 'max': round(max(rounds[what]), 4),
                              'over_mlpg_backward': round(medians[what] / medians['mlpg_backward'], 3), 'calls': args.calls,
                              'repeats': args.repeats}))


def trace(args):
    for name, d in STREAMS:
        for fn in kernel_inputs(d):
            for _ in range(5):
                fn()
    torch.cuda.synchronize()


def steps(args):
    built = []
    for predict_variance in (False, True):
        torch.manual_seed(synthetic.REFERENCE_SEED)
        feats = synthetic.make_acoustic_batch(B, T, streams=(('lf0', 3, 'mse'),), with_raw=True)
        model = models.GRUF0Model(precision=args.precision, trajectory_weight=1., predict_variance=predict_variance).to(DEV)
        own = model.state_dict()
        for key, value in synthetic.gru_f0_state(output_dim=model.streams[0].width).items():
            own[key].copy_(torch.from_numpy(value))
        synthetic.acoustic_normalisers(model, device=DEV)
        model.mode = 'train'
        model.metrics.reset_state('train')
        features = data.to_device(feats, DEV, bf16_tables=model.bf16_table_features())
        optimizer = optim.Adam(model.parameters(), lr=0.01, fused_loop=True)

        def step(model=model, optimizer=optimizer, features=features):
            optimizer.zero_grad()
            loss, _ = model(features)
            F_hip.backward(loss)
            optimizer.step()

        for _ in range(args.warmup):
            step()
        built.append((predict_variance, step))
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    rounds = {flag: [] for flag, _ in built}
    for _ in range(args.repeats):                           # alternating, as the kernels
        for flag, step in built:
            rounds[flag].append(window(step, args.step_calls))
    gc.enable()
    for flag, _ in built:
        print(json.dumps({'config': 'f0gru', 'precision': args.precision, 'trajectory_weight': 1.0, 'predict_variance': flag,
                          'ms_per_step': round(float(np.median(rounds[flag])), 3), 'min': round(min(rounds[flag]), 3),
                          'max': round(max(rounds[flag]), 3), 'steps': args.step_calls, 'repeats': args.repeats}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('part', choices=['kernels', 'steps', 'trace'])
    ap.add_argument('--calls', type=int, default=50, help='kernels: calls per timed window')
    ap.add_argument('--step-calls', type=int, default=10, help='steps: training steps per timed window')
    ap.add_argument('--repeats', type=int, default=7, help='rounds per measurement')
    ap.add_argument('--warmup', type=int, default=5, help='steps: untimed steps in front')
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'fp32'])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mlpg_var_grad.py needs an MI355X: there is no CPU path to time')
    {'kernels': kernels, 'steps': steps, 'trace': trace}[args.part](args)


if __name__ == '__main__':
    main()
