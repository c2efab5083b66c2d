#!/usr/bin/env python
"""Cost of the global-variance loss (csrc/gv.hip): forward plus backward on a RESIDENT ragged batch, and of the training steps that
carry it.

A 64 x 1000 batch with ragged lengths drawn from 300..2000 and clipped to T, at D = 1, 5, 60 and 180 (lf0, bap, mcep statics, and a
delta-wide stream).  Four legs are timed with device events, in turn inside every round (they see the same moments of a shared
machine):

    kernels  ``ops.gv`` + ``ops.gv_backward`` replayed from a HIP graph: the three launches alone (device time)
    direct   the same two calls from Python: what the launches cost with their host work
    wrapper  ``losses.gv`` and ``torch.autograd.grad``: what a model pays, autograd's host work included
    eager    the same loss composed of torch ops on the same device (mask, means, centred squares, logs, their autograd mirrors)

The MEDIAN round of each leg is reported with the algorithmic bytes of the three launches - the forward reads the valid frames of
two operands, the backward reads those of one and writes the dense gradient - and the rate they give against the 6.29 TB/s copy
rate.  Then the f0gru and lstm (``fused_loss=False``, ``trajectory_weight=1``) training steps with ``gv_weight`` 0 and 1.  Prints one
JSON line per shape and one per model.  Not part of bench.py.

    python scripts/bench_gv.py [--steps 50] [--rounds 7] [--warmup 20] [--precision bf16] [--skip-steps] [--trace]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morgana_amd import data, losses, models, ops, optim, synthetic  # noqa: E402
from morgana_amd import functional as F_hip  # noqa: E402

COPY_RATE = 6.29e12
DIMS = (1, 5, 60, 180)
BATCH, FRAMES = 64, 1000
REPLAY_CALLS = 10


def eager_gv(pred, tgt, seq_len, eps=1e-6):
    """``losses.gv`` (log=True) in torch ops."""
    mask = (torch.arange(pred.shape[1], device=pred.device)[None, :] < seq_len[:, None]).to(pred.dtype).unsqueeze(-1)
    n = torch.sum(mask, dim=1)

    def variance(x):
        mean = torch.sum(x * mask, dim=1, keepdim=True) / n.unsqueeze(1)
        return torch.sum(((x - mean) * mask) ** 2, dim=1) / n

    return torch.mean((torch.log(variance(pred) + eps) - torch.log(variance(tgt) + eps)) ** 2)


def _graph_of(call):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(REPLAY_CALLS):
            call()
    return graph


def _time_legs(legs, args):
    """{name: [ms per call, one per round]}: the legs in turn inside every round; legs = [(name, call, calls per call())]."""
    for _, call, _ in legs:
        for _ in range(args.warmup):
            call()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, call, per in legs:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.steps):
                call()
            end.record()
            end.synchronize()
            times[name].append(start.elapsed_time(end) / (args.steps * per))
    return times


def measure_loss(d, args, dev):
    b, t = BATCH, FRAMES
    rng = np.random.RandomState(20261019 + d)
    lens = np.minimum(rng.randint(300, 2001, size=b), t).astype(np.int64)
    seq_len = torch.from_numpy(lens).to(dev)
    valid = int(lens.sum())
    y_np = rng.standard_normal((b, t, d)).astype(np.float32)
    y = torch.from_numpy(y_np).to(dev)
    x = torch.from_numpy((0.6 * y_np + 0.2 * rng.standard_normal((b, t, d))).astype(np.float32)).to(dev).requires_grad_(True)
    xd = x.detach()
    one = torch.ones((), device=dev)

    def wrapper():
        return torch.autograd.grad(losses.gv(x, y, seq_len), x)[0]

    def direct():
        _, state, _, _ = ops.gv(xd, y, seq_len)
        return ops.gv_backward(one, state, xd, seq_len)

    def eager():
        return torch.autograd.grad(eager_gv(x, y, seq_len), x)[0]

    want = eager()
    for name, call in (('wrapper', wrapper), ('direct', direct)):
        err = ((call() - want).abs().max() / want.abs().max()).item()
        assert err <= 1e-4, (name, err)
    kernels = _graph_of(direct)
    legs = [('kernels', kernels.replay, REPLAY_CALLS), ('direct', direct, 1), ('wrapper', wrapper, 1), ('eager', eager, 1)]
    times = _time_legs(legs, args)
    n_bytes = 4 * d * (2 * valid + valid + b * t)
    record = {'D': d, 'batch': b, 'frames': t, 'valid_frames': valid, 'steps': args.steps, 'rounds': args.rounds, 'bytes': n_bytes}
    for name, _, _ in legs:
        ms = statistics.median(times[name])
        record['ms_' + name] = round(ms, 5)
        record['ms_%s_min_max' % name] = [round(min(times[name]), 5), round(max(times[name]), 5)]
        if name != 'eager':
            record['TBps_' + name] = round(n_bytes / (ms * 1e-3) / 1e12, 4)
            record['share_of_copy_rate_' + name] = round(n_bytes / (ms * 1e-3) / COPY_RATE, 4)
    record['eager_over_wrapper'] = round(record['ms_eager'] / record['ms_wrapper'], 2)
    record['eager_over_kernels'] = round(record['ms_eager'] / record['ms_kernels'], 2)
    return record


def trace(dev, calls=20):
    """``calls`` direct calls at every D, one D after the other: the kernel trace then holds runs of ``calls`` launches per kernel."""
    one = torch.ones((), device=dev)
    for d in DIMS:
        rng = np.random.RandomState(20261019 + d)
        seq_len = torch.from_numpy(np.minimum(rng.randint(300, 2001, size=BATCH), FRAMES).astype(np.int64)).to(dev)
        y = torch.from_numpy(rng.standard_normal((BATCH, FRAMES, d)).astype(np.float32)).to(dev)
        x = 0.6 * y + 0.2 * torch.randn_like(y)
        for _ in range(calls):
            _, state, _, _ = ops.gv(x, y, seq_len)
            ops.gv_backward(one, state, x, seq_len)
        torch.cuda.synchronize()


def measure_steps(config, args, dev):
    """The training step (forward, backward, Adam; eager launches) of a shipped model with gv_weight 0 and 1, in turn per round."""
    legs = []
    for gv_weight in (0., 1.):
        torch.manual_seed(synthetic.REFERENCE_SEED)
        if config == 'f0gru':
            feats = synthetic.make_acoustic_batch(BATCH, FRAMES, streams=(('lf0', 3, 'mse'),), with_raw=True)
            model, state = models.GRUF0Model(precision=args.precision, gv_weight=gv_weight).to(dev), synthetic.gru_f0_state()
        else:
            feats = synthetic.make_acoustic_batch(BATCH, FRAMES, with_raw=True)
            model = models.LSTMAcousticModel(precision=args.precision, fused_loss=False, trajectory_weight=1., gv_weight=gv_weight).to(dev)
            state = synthetic.lstm_acoustic_state()
        own = model.state_dict()
        for key, value in state.items():
            own[key].copy_(torch.from_numpy(value))
        synthetic.acoustic_normalisers(model, device=dev)
        model.mode = 'train'
        model.metrics.reset_state('train')
        features = data.to_device(feats, dev, bf16_tables=model.bf16_table_features())
        optimizer = optim.Adam(model.parameters(), lr=0.01, fused_loop=True)

        def step(model=model, optimizer=optimizer, features=features):
            optimizer.zero_grad()
            loss, _ = model(features)
            F_hip.backward(loss)
            optimizer.step()
            return loss

        assert np.isfinite(step().item())
        legs.append(('gv_weight_%d' % gv_weight, step, 1))
    times = _time_legs(legs, args)
    what = {'f0gru': 'GRUF0Model', 'lstm': 'LSTMAcousticModel, fused_loss=False, trajectory_weight=1'}[config]
    record = {'step': '%s: %d x %d frames, %s, eager launches' % (what, BATCH, FRAMES, args.precision), 'steps': args.steps,
              'rounds': args.rounds}
    for name, _, _ in legs:
        record['ms_' + name] = round(statistics.median(times[name]), 4)
        record['ms_%s_min_max' % name] = [round(min(times[name]), 4), round(max(times[name]), 4)]
    record['gv_over_none'] = round(record['ms_gv_weight_1'] / record['ms_gv_weight_0'], 4)
    return record


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--steps', type=int, default=50)
    parser.add_argument('--rounds', type=int, default=7)
    parser.add_argument('--warmup', type=int, default=20)
    parser.add_argument('--precision', default='bf16', choices=['bf16', 'fp32', 'bf16x3'])
    parser.add_argument('--skip-steps', action='store_true', help='the loss legs only')
    parser.add_argument('--trace', action='store_true', help='a few direct calls per D and nothing else: run it under '
                        '`rocprofv3 --kernel-trace --stats -- python scripts/bench_gv.py --trace`, a run of its own, for the time of '
                        'each of the three kernels (gv_partial_kernel, gv_finish_kernel, gv_bwd_kernel)')
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_gv.py measures on an MI355X: no device found')
    dev = torch.device('cuda:0')
    if args.trace:
        trace(dev)
        return
    for d in DIMS:
        print(json.dumps(measure_loss(d, args, dev)), flush=True)
    if not args.skip_steps:
        for config in ('f0gru', 'lstm'):
            print(json.dumps(measure_steps(config, args, dev)), flush=True)


if __name__ == '__main__':
    main()
