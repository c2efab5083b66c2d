#!/usr/bin/env python
"""Cost of the reduction behind ``losses.sequence_loss`` (csrc/seqmean.hip): forward plus backward on a RESIDENT feature loss.

Two shapes, (64, 1000, 180) - a mel-cepstrum stream of the acoustic model's batch - and (64, 1000, 1), with ragged lengths drawn
from 300..2000 and clipped to T.  Three legs are timed with device events, in turn inside every round (they see the same moments of a
shared machine):

    wrapper  an identity-wrapped ``losses.sequence_loss`` and ``torch.autograd.grad``: what a model pays, autograd's host work included
    kernels  ``ops.masked_seq_mean`` + ``ops.masked_seq_mean_bwd`` called directly: the three launches alone
    eager    the reference's formulation of the same wrapper in torch ops on the same device (mask, mul, two sums, div, mean and
             their autograd mirrors)

The MEDIAN round of each leg is reported with the algorithmic bytes of the kernel pair (4 B T D read forward, 4 B T D written
backward) and the rate they give against the 6.29 TB/s copy rate.  Prints one JSON line per shape.  Not part of bench.py.

    python scripts/bench_seqloss.py [--steps 200] [--rounds 7] [--warmup 50]
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
SHAPES = ((64, 1000, 180), (64, 1000, 1))


def eager_sequence_loss(feature_loss, seq_len):
    """morgana/losses.py:29-46 restated in torch ops (the mask as utils.sequence_mask builds it)."""
    mask = (torch.arange(feature_loss.shape[1], device=seq_len.device)[None, :] < seq_len[:, None]).to(feature_loss.dtype).unsqueeze(-1)
    num_valid_frames = torch.sum(mask, dim=1)
    return torch.mean(torch.sum(feature_loss * mask, dim=1) / num_valid_frames)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--steps', type=int, default=200)
    parser.add_argument('--rounds', type=int, default=7)
    parser.add_argument('--warmup', type=int, default=50)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_seqloss.py measures on an MI355X: no device found')
    dev = torch.device('cuda:0')
    identity = losses.sequence_loss(lambda predictions, targets: predictions)
    one = torch.ones((), device=dev)
    for shape in SHAPES:
        b, t, d = shape
        rng = np.random.RandomState(20261019)
        seq_len = torch.from_numpy(np.minimum(rng.randint(300, 2001, size=b), t).astype(np.int64)).to(dev)
        x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev).requires_grad_(True)

        def wrapper():
            return torch.autograd.grad(identity(x, None, seq_len), x)[0]

        def kernels():
            ops.masked_seq_mean(x.detach(), seq_len)
            return ops.masked_seq_mean_bwd(one, seq_len, shape)

        def eager():
            return torch.autograd.grad(eager_sequence_loss(x, seq_len), x)[0]

        legs = (('wrapper', wrapper), ('kernels', kernels), ('eager', eager))
        want = eager()
        for name, call in legs:
            got = call()
            err = ((got - want).abs().max() / want.abs().max()).item()
            assert err <= 1e-6, (name, err)
            for _ in range(args.warmup):
                call()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, call in legs:
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(args.steps):
                    call()
                end.record()
                end.synchronize()
                times[name].append(start.elapsed_time(end) / args.steps)
        n_bytes = 8 * b * t * d
        record = {'shape': list(shape), 'valid_frames': int(seq_len.sum().item()), 'steps': args.steps, 'rounds': args.rounds,
                  'kernel_pair_bytes': n_bytes, 'feature_loss_MB': round(4 * b * t * d / 1e6, 2)}
        for name, _ in legs:
            ms = statistics.median(times[name])
            record['ms_' + name] = round(ms, 5)
            record['ms_%s_min_max' % name] = [round(min(times[name]), 5), round(max(times[name]), 5)]
            if name != 'eager':
                record['TBps_' + name] = round(n_bytes / (ms * 1e-3) / 1e12, 4)
                record['share_of_copy_rate_' + name] = round(n_bytes / (ms * 1e-3) / COPY_RATE, 4)
        record['eager_over_wrapper'] = round(record['ms_eager'] / record['ms_wrapper'], 3)
        record['eager_over_kernels'] = round(record['ms_eager'] / record['ms_kernels'], 3)
        print(json.dumps(record), flush=True)


if __name__ == '__main__':
    main()
