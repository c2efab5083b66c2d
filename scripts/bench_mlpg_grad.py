#!/usr/bin/env python
"""What differentiable MLPG costs, on a resident 64 x 1000 batch with padding 100 (the shipped models' call).

    bench_mlpg_grad.py kernels     ops.mlpg and ops.mlpg_backward for D = 1, 5, 60 (lf0, bap, mcep) by device events: the median and the
                                   spread of --repeats windows of --calls calls each
    bench_mlpg_grad.py steps       the f0gru and lstm training steps (forward, backward, Adam; eager launches, bf16 as bench.py runs
                                   them) with trajectory_weight 0 and 1; the lstm model also with fused_loss=False and weight 0, which
                                   is what a positive weight has to be compared with (it needs fused_loss=False)
    bench_mlpg_grad.py trace       the calls of `kernels`, a few of each and nothing else: run it under
                                   `rocprofv3 --kernel-trace --stats -- python scripts/bench_mlpg_grad.py trace`, a run of its own, for
                                   the per-kernel times (mlpg_band_kernel, mlpg_solve_kernel, mlpg_scatter_kernel)
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


def timed(fn, calls, repeats):
    """Milliseconds per call of ``fn``: (median, min, max) over ``repeats`` event-timed windows of ``calls`` calls."""
    per_call = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) / calls)
    return float(np.median(per_call)), min(per_call), max(per_call)


def kernel_inputs(d):
    g = torch.Generator(device=DEV).manual_seed(d)
    means = torch.randn(B, T, 3 * d, device=DEV, generator=g)
    grad_out = torch.randn(B, T, d, device=DEV, generator=g)
    var = (torch.rand(3 * d, device=DEV, generator=g) * 0.4 + 0.2) ** 2
    seq = torch.full((B,), T, dtype=torch.int64, device=DEV)
    forward = lambda: ops.mlpg(means, var, synthesis.DEFAULT_WINDOWS, padding_size=PADDING, seq_len=seq)                   # noqa: E731
    backward = lambda: ops.mlpg_backward(grad_out, var, synthesis.DEFAULT_WINDOWS, padding_size=PADDING, seq_len=seq)      # noqa: E731
    return forward, backward


def kernels(args):
    for name, d in STREAMS:
        for what, fn in zip(('mlpg', 'mlpg_backward'), kernel_inputs(d)):
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            median, low, high = timed(fn, args.calls, args.repeats)
            print(json.dumps({'op': what, 'stream': name, 'D': d, 'systems': B * d, 'unknowns': T + 2 * PADDING, 'ms_per_call': round(median, 4),
                              'min': round(low, 4), 'max': round(high, 4), 'calls': args.calls, 'repeats': args.repeats}))


def trace(args):
    for name, d in STREAMS:
        for fn in kernel_inputs(d):
            for _ in range(5):
                fn()
    torch.cuda.synchronize()


def steps(args):
    configs = [('f0gru', {'trajectory_weight': 0.}), ('f0gru', {'trajectory_weight': 1.}),
               ('lstm', {'trajectory_weight': 0.}), ('lstm', {'trajectory_weight': 0., 'fused_loss': False}),
               ('lstm', {'trajectory_weight': 1., 'fused_loss': False})]
    for config, kwargs in configs:
        torch.manual_seed(synthetic.REFERENCE_SEED)
        if config == 'f0gru':
            feats = synthetic.make_acoustic_batch(B, T, streams=(('lf0', 3, 'mse'),), with_raw=True)
            model, state = models.GRUF0Model(precision=args.precision, **kwargs).to(DEV), synthetic.gru_f0_state()
        else:
            feats = synthetic.make_acoustic_batch(B, T, with_raw=True)
            model, state = models.LSTMAcousticModel(precision=args.precision, **kwargs).to(DEV), synthetic.lstm_acoustic_state()
        own = model.state_dict()
        for key, value in state.items():
            own[key].copy_(torch.from_numpy(value))
        synthetic.acoustic_normalisers(model, device=DEV)
        model.mode = 'train'
        model.metrics.reset_state('train')
        features = data.to_device(feats, DEV, bf16_tables=model.bf16_table_features())
        optimizer = optim.Adam(model.parameters(), lr=0.01, fused_loop=True)

        def step():
            optimizer.zero_grad()
            loss, _ = model(features)
            F_hip.backward(loss)
            optimizer.step()

        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        gc.collect()
        gc.disable()
        median, low, high = timed(step, args.step_calls, args.repeats)
        gc.enable()
        print(json.dumps(dict({'config': config, 'precision': args.precision, 'ms_per_step': round(median, 3), 'min': round(low, 3),
                               'max': round(high, 3), 'steps': args.step_calls, 'repeats': args.repeats}, **kwargs)))
        del model, optimizer, features


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('part', choices=['kernels', 'steps', 'trace'])
    ap.add_argument('--calls', type=int, default=50, help='kernels: calls per timed window')
    ap.add_argument('--step-calls', type=int, default=10, help='steps: training steps per timed window')
    ap.add_argument('--repeats', type=int, default=7, help='timed windows per measurement')
    ap.add_argument('--warmup', type=int, default=5, help='steps: untimed steps in front')
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'fp32'])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mlpg_grad.py needs an MI355X: there is no CPU path to time')
    {'kernels': kernels, 'steps': steps, 'trace': trace}[args.part](args)


if __name__ == '__main__':
    main()
