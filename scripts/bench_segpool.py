#!/usr/bin/env python
"""Cost of ``utils.pool_segments`` (csrc/segpool.hip): mean pooling, forward plus backward, on RESIDENT 64 x 1000 ragged batches.

Three shapes: F = 512 with 80 phone segments per utterance (hidden activations at phone rate), F = 3 with the same segments (lf0 and
its deltas) and F = 64 with one segment per utterance (the VAE encoder's case).  Lengths are drawn from 300..2000 and clipped to T;
the phone segments partition each utterance's valid frames.  Three legs are timed with device events around ``--steps`` calls, in turn
inside every round (they see the same moments of a shared machine):

    kernels  ``ops.segment_pool`` + ``ops.segment_pool_backward`` called directly: the two launches alone (``forward`` and ``backward``
             time each of the two on its own)
    wrapper  ``utils.pool_segments`` and ``torch.autograd.grad``: what a model pays, autograd's host work included
    former   this library's former route: ``utils.split_to_segments`` + ``torch.sum(dim=2)`` / lengths and its autograd mirror, with
             the host read of ``segment_lens.max()`` that sizes the padded block

The MEDIAN round of each leg is reported with the algorithmic bytes of the kernel pair (valid frames read and (B, S, F) written
forward; (B, S, F) read and (B, T, F) written backward) and the rate they give against the 6.29 TB/s copy rate.  Prints one JSON line
per shape.  Not part of bench.py.

    python scripts/bench_segpool.py [--steps 50] [--rounds 7] [--warmup 20]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morgana_amd import ops, utils  # noqa: E402

COPY_RATE = 6.29e12
SHAPES = (('wide rows, phone segments', 512, 80), ('narrow rows, phone segments', 3, 80), ('one segment per utterance', 64, 1))
B, T = 64, 1000


def phone_segments(rng, n_frames, s):
    """(B, s) int64: every utterance's valid frames cut into s segments of at least one frame, the longest around 60 at 1000 frames."""
    lens = np.zeros((len(n_frames), s), dtype=np.int64)
    for i, n in enumerate(n_frames):
        weights = rng.gamma(2.0, size=s)
        extra = rng.multinomial(int(n) - s, weights / weights.sum())
        lens[i] = 1 + extra
    return lens


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--steps', type=int, default=50)
    parser.add_argument('--rounds', type=int, default=7)
    parser.add_argument('--warmup', type=int, default=20)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_segpool.py measures on an MI355X: no device found')
    dev = torch.device('cuda:0')
    for label, f, s in SHAPES:
        rng = np.random.RandomState(20261021)
        n_frames = np.minimum(rng.randint(300, 2001, size=B), T).astype(np.int64)
        lens_np = phone_segments(rng, n_frames, s) if s > 1 else n_frames.reshape(B, 1)
        seq_len, lens = torch.from_numpy(n_frames).to(dev), torch.from_numpy(lens_np).to(dev)
        x = torch.from_numpy(rng.standard_normal((B, T, f)).astype(np.float32)).to(dev).requires_grad_(True)
        g = torch.from_numpy(rng.standard_normal((B, s, f)).astype(np.float32)).to(dev)
        counts = lens.clamp(min=1).to(torch.float32).unsqueeze(-1)

        def kernels():
            ops.segment_pool(x.detach(), lens, seq_len, 'mean')
            return ops.segment_pool_backward(g, lens, seq_len, None, 'mean', T)

        def forward():
            return ops.segment_pool(x.detach(), lens, seq_len, 'mean')[0]

        def backward():
            return ops.segment_pool_backward(g, lens, seq_len, None, 'mean', T)

        def wrapper():
            return torch.autograd.grad(utils.pool_segments(x, lens, 'mean', seq_len=seq_len), x, g)[0]

        def former():
            return torch.autograd.grad(torch.sum(utils.split_to_segments(x, lens), dim=2) / counts, x, g)[0]

        legs = (('kernels', kernels), ('wrapper', wrapper), ('former', former))
        want = former()
        for name, call in legs:
            got = call()
            err = ((got - want).abs().max() / want.abs().max()).item()
            assert err <= 1e-5, (name, err)
        legs = legs + (('forward', forward), ('backward', backward))
        for name, call in legs:
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
        valid = int(n_frames.sum())
        n_bytes = 4 * f * (valid + B * s) + 4 * f * (B * s + B * T)
        record = {'shape': label, 'B': B, 'T': T, 'F': f, 'S': s, 'valid_frames': valid, 'longest_segment': int(lens_np.max()),
                  'steps': args.steps, 'rounds': args.rounds, 'kernel_pair_bytes': n_bytes, 'input_MB': round(4 * B * T * f / 1e6, 2),
                  'padded_block_MB': round(4 * B * s * int(lens_np.max()) * f / 1e6, 2)}
        for name, _ in legs:
            ms = statistics.median(times[name])
            record['ms_' + name] = round(ms, 5)
            record['ms_%s_min_max' % name] = [round(min(times[name]), 5), round(max(times[name]), 5)]
            if name in ('kernels', 'wrapper'):
                record['TBps_' + name] = round(n_bytes / (ms * 1e-3) / 1e12, 4)
                record['share_of_copy_rate_' + name] = round(n_bytes / (ms * 1e-3) / COPY_RATE, 4)
        record['former_over_wrapper'] = round(record['ms_former'] / record['ms_wrapper'], 3)
        record['former_over_kernels'] = round(record['ms_former'] / record['ms_kernels'], 3)
        record['wrapper_over_kernels'] = round(record['ms_wrapper'] / record['ms_kernels'], 3)
        print(json.dumps(record), flush=True)


if __name__ == '__main__':
    main()
