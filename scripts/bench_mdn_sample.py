#!/usr/bin/env python
"""Cost of ``losses.mdn_sample`` (csrc/mdn.hip, mg_mdn_sample_f32): one draw per frame from a mixture-density stream on a RESIDENT
64 x 1000 batch at (K, D) = (8, 3) and (16, 3) (an lf0 stream) and (4, 180) (a mel-cepstrum stream), with ragged lengths drawn from
300..2000 and clipped to T.

Legs per shape, timed with device events in turn inside every round (they see the same moments of a shared machine):

    sample0  the launch of mg_mdn_sample_f32 at noise_scale = 0 (``ops.mdn_sample`` with an explicit seed and counter) replayed from
             a HIP graph: device time, no host in it
    sample1  the same at noise_scale = 1 (a Philox block, a logarithm, a square root and a sine / cosine per output element)
    select   ``ops.mdn_select`` replayed from a graph likewise: the launch sampling replaces, on the same library
    wrapper  ``losses.mdn_sample`` at noise_scale = 1 called from Python: the launch, the step counter's launch and their host cost
    eager    the same draw composed of torch ops on the same device: softmax, torch.distributions.Categorical.sample, two gathers,
             exp, randn_like, addcmul (torch's own generator: not restatable, not the counter scheme)

The MEDIAN round of each leg is reported with the algorithmic bytes of the kernel (valid frames: 4 (K + 2 D) read; every frame:
8 + 8 D written) and the rate they give against the 6.29 TB/s copy rate.  One JSON line per shape.  Not part of bench.py.

    python scripts/bench_mdn_sample.py [--steps 50] [--rounds 7] [--warmup 20]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morgana_amd import losses, ops  # noqa: E402

COPY_RATE = 6.29e12
SHAPES = ((8, 3), (16, 3), (4, 180))
BATCH, FRAMES = 64, 1000
REPLAY_CALLS = 10
SEED = 0x0123456789ABCDEF


def eager_sample(x, k, d, noise_scale=1.0):
    b, t, _ = x.shape
    a, mu, s = x[:, :, :k], x[:, :, k:k + k * d].reshape(b, t, k, d), x[:, :, k + k * d:].reshape(b, t, k, d)
    component = torch.distributions.Categorical(probs=torch.softmax(a, dim=-1)).sample()
    pick = component[:, :, None, None].expand(-1, -1, 1, d)
    mean, log_std = torch.gather(mu, 2, pick)[:, :, 0], torch.gather(s, 2, pick)[:, :, 0]
    std = torch.exp(log_std)
    return component, torch.addcmul(mean, std, torch.randn_like(mean), value=noise_scale), std * std


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


def measure(k, d, args, dev):
    b, t, w = BATCH, FRAMES, k * (1 + 2 * d)
    rng = np.random.RandomState(20261021 + 1000 * k + d)
    lens = np.minimum(rng.randint(300, 2001, size=b), t).astype(np.int64)
    seq_len = torch.from_numpy(lens).to(dev)
    valid = int(lens.sum())
    pred = np.concatenate((2.0 * rng.standard_normal((b, t, k)), rng.standard_normal((b, t, k * d)),
                           -0.5 + 0.5 * rng.standard_normal((b, t, k * d))), axis=2).astype(np.float32)
    x = torch.from_numpy(pred).to(dev)
    used = torch.tensor([7], dtype=torch.int64, device=dev)
    ops.dropout_state(dev)

    # the launch draws what its definition says: the share of every component over the valid frames against the mean softmax
    component = ops.mdn_sample(x, seq_len, k, d, SEED, used)[0]
    mask = torch.arange(t, device=dev)[None, :] < seq_len[:, None]
    share = torch.bincount(component[mask], minlength=k).double() / valid
    want = torch.softmax(x[:, :, :k].double(), dim=-1)[mask].mean(0)
    assert (share - want).abs().max().item() <= 5.0 * 0.5 / np.sqrt(valid), (share, want)

    sample0 = _graph_of(lambda: ops.mdn_sample(x, seq_len, k, d, SEED, used))
    sample1 = _graph_of(lambda: ops.mdn_sample(x, seq_len, k, d, SEED, used, noise_scale=1.0))
    select = _graph_of(lambda: ops.mdn_select(x, seq_len, k, d))
    legs = [('sample0', sample0.replay, REPLAY_CALLS), ('sample1', sample1.replay, REPLAY_CALLS), ('select', select.replay, REPLAY_CALLS),
            ('wrapper', lambda: losses.mdn_sample(x, k, d, seq_len=seq_len, noise_scale=1.0), 1),
            ('eager', lambda: eager_sample(x, k, d), 1)]
    times = _time_legs(legs, args)
    n_bytes = valid * 4 * (k + 2 * d) + b * t * (8 + 8 * d)
    record = {'K': k, 'D': d, 'W': w, 'batch': b, 'frames': t, 'valid_frames': valid, 'steps': args.steps, 'rounds': args.rounds,
              'bytes': n_bytes}
    for name, _, _ in legs:
        ms = statistics.median(times[name])
        record['us_' + name] = round(1e3 * ms, 2)
        record['us_%s_min_max' % name] = [round(1e3 * min(times[name]), 2), round(1e3 * max(times[name]), 2)]
    for name in ('sample0', 'sample1', 'select'):
        record['share_of_copy_rate_' + name] = round(n_bytes / (record['us_' + name] * 1e-6) / COPY_RATE, 4)
    record['sample0_over_select'] = round(record['us_sample0'] / record['us_select'], 3)
    record['sample1_over_select'] = round(record['us_sample1'] / record['us_select'], 3)
    record['eager_over_wrapper'] = round(record['us_eager'] / record['us_wrapper'], 2)
    record['eager_over_sample1'] = round(record['us_eager'] / record['us_sample1'], 2)
    return record


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--steps', type=int, default=50)
    parser.add_argument('--rounds', type=int, default=7)
    parser.add_argument('--warmup', type=int, default=20)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mdn_sample.py measures on an MI355X: no device found')
    dev = torch.device('cuda:0')
    for k, d in SHAPES:
        print(json.dumps(measure(k, d, args, dev)), flush=True)


if __name__ == '__main__':
    main()
