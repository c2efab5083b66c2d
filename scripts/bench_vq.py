#!/usr/bin/env python
"""Cost of the vector quantiser (csrc/vq.hip): assignment plus both gradients on a RESIDENT batch.

Two sizes, the ends of what the kernel is meant for: an utterance-level quantiser (N = 64 rows, K = 64 codes, D = 16) and a frame-
or segment-level one (N = 64 000, K = 512, D = 64).  Three legs are timed with device events, in turn inside every round (they see
the same moments of a shared machine):

    kernels  ``ops.vq_assign`` + ``ops.vq_backward`` replayed from a HIP graph: the five launches alone (device time)
    wrapper  ``functional.VQFn`` and ``torch.autograd.grad``: what a model pays, autograd's host work included
    eager    the same thing composed of torch ops on the same device: ``cdist``, ``argmin``, an index select, the straight-through
             sum and two ``mse_loss`` with detaches, and their autograd mirrors (float32 distances in the expanded form: what a
             user would write, not what the kernel computes)

The MEDIAN round of each leg is reported, with the float64 distance terms (N K D) per second the kernels' time gives.  Prints one
JSON line per size.  Not part of bench.py.

    python scripts/bench_vq.py [--steps 50] [--rounds 7] [--warmup 20]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morgana_amd import ops  # noqa: E402
from morgana_amd import functional as F_hip  # noqa: E402

SIZES = ((64, 64, 16), (64000, 512, 64))
REPLAY_CALLS = 10
CODEBOOK_WEIGHT, COMMITMENT_WEIGHT = 1.0, 0.25


def eager_vq(z, codebook):
    """The textbook quantiser in torch ops -> (latent, loss)."""
    index = torch.argmin(torch.cdist(z.detach(), codebook.detach()), dim=1)
    z_q = codebook.index_select(0, index)
    latent = z + (z_q - z).detach()
    return latent, CODEBOOK_WEIGHT * F.mse_loss(z.detach(), z_q) + COMMITMENT_WEIGHT * F.mse_loss(z, z_q.detach())


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


def measure_quantiser(n, k, d, args, dev):
    rng = np.random.RandomState(20261020 + n)
    codebook_np = rng.standard_normal((k, d)).astype(np.float32)
    z_np = (codebook_np[rng.randint(0, k, size=n)] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    z = torch.from_numpy(z_np).to(dev).requires_grad_(True)
    codebook = torch.from_numpy(codebook_np).to(dev).requires_grad_(True)
    up = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
    zd, cd, one = z.detach(), codebook.detach(), torch.ones((), device=dev)

    def wrapper():
        latent, _, loss, _, _ = F_hip.VQFn.apply(z, codebook, None, CODEBOOK_WEIGHT, COMMITMENT_WEIGHT)
        return torch.autograd.grad((latent * up).sum() + loss, (z, codebook))

    def direct():
        index, quantised, _, _, _, n_valid = ops.vq_assign(zd, cd)
        return ops.vq_backward(up, one, zd, quantised, index, n_valid, k, CODEBOOK_WEIGHT, COMMITMENT_WEIGHT)

    def eager():
        latent, loss = eager_vq(z, codebook)
        return torch.autograd.grad((latent * up).sum() + loss, (z, codebook))

    want = eager()
    for name, call in (('wrapper', wrapper), ('direct', direct)):
        for got, ref in zip(call(), want):
            err = ((got - ref).abs().max() / ref.abs().max()).item()
            assert err <= 1e-4, (name, err)
    kernels = _graph_of(direct)
    legs = [('kernels', kernels.replay, REPLAY_CALLS), ('wrapper', wrapper, 1), ('eager', eager, 1)]
    times = _time_legs(legs, args)
    record = {'N': n, 'K': k, 'D': d, 'steps': args.steps, 'rounds': args.rounds, 'distance_terms': n * k * d}
    for name, _, _ in legs:
        ms = statistics.median(times[name])
        record['ms_' + name] = round(ms, 5)
        record['ms_%s_min_max' % name] = [round(min(times[name]), 5), round(max(times[name]), 5)]
    record['G_terms_per_s_kernels'] = round(n * k * d / (record['ms_kernels'] * 1e-3) / 1e9, 2)
    record['eager_over_wrapper'] = round(record['ms_eager'] / record['ms_wrapper'], 2)
    record['eager_over_kernels'] = round(record['ms_eager'] / record['ms_kernels'], 2)
    return record


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--steps', type=int, default=50)
    parser.add_argument('--rounds', type=int, default=7)
    parser.add_argument('--warmup', type=int, default=20)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_vq.py measures on an MI355X: no device found')
    dev = torch.device('cuda:0')
    for n, k, d in SIZES:
        print(json.dumps(measure_quantiser(n, k, d, args, dev)), flush=True)


if __name__ == '__main__':
    main()
