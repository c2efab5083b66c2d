#!/usr/bin/env python
"""Cost of getting generated features off the device: ``utils.detach_batched_seqs`` (ragged pack on the device, one D2H copy of
the valid frames) against the reference's formulation in the same process (per feature ``.cpu().detach().numpy()`` of the whole
padded tensor, then the per-item slices; morgana/utils.py:66-102).

Workload: BASELINE config C5's lengths (64 utterances of 300-2000 frames) and the four outputs of ``LSTMAcousticModel``
(lf0 1, vuv 1, mcep 60, bap 5 columns, float32).  Warm-up, then ``--repeats`` timed calls of each, taking turns; the MEDIAN is reported.  The
pack launch's time is a device-event interval around 50 launches enqueued back to back, divided by 50 (median as well): an upper
bound of the kernel's time that still holds whatever the host spends per call beyond it; its GB/s counts bytes read plus bytes written.  Prints one JSON line.  Not part of bench.py.

    python scripts/bench_detach.py [--repeats 30] [--warmup 5] [--batch 64] [--seed 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morgana_amd import ops, utils  # noqa: E402

WIDTHS = (('lf0', 1), ('vuv', 1), ('mcep', 60), ('bap', 5))
LAUNCHES = 50


def reference_detach(features, seq_len):
    seq_len = seq_len.cpu().detach().numpy()
    out = []
    for feature in features:
        whole = feature.cpu().detach().numpy()
        out.append([item[:n].squeeze() for item, n in zip(whole, seq_len)])
    return out


def timed(fns, warmup, repeats):
    """Median host time of each function, the functions taking turns (both see the same moments of a shared host)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    return [statistics.median(t) for t in times]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--repeats', type=int, default=30)
    parser.add_argument('--warmup', type=int, default=5)
    parser.add_argument('--batch', type=int, default=64)
    parser.add_argument('--seed', type=int, default=5)
    args = parser.parse_args()
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(args.seed)
    lens = rng.randint(300, 2001, size=args.batch).astype(np.int64)
    t = int(lens.max())
    mask = torch.from_numpy((np.arange(t)[None, :] < lens[:, None])[..., None]).to(dev)
    features = [torch.randn(args.batch, t, w, device=dev) * mask for _, w in WIDTHS]
    seq_len = torch.from_numpy(lens).to(dev)

    got, want = utils.detach_batched_seqs(*features, seq_len=seq_len), reference_detach(features, seq_len)
    assert all(np.array_equal(g, w) for gs, ws in zip(got, want) for g, w in zip(gs, ws)), 'the two formulations disagree'

    packed_s, padded_s = timed([lambda: utils.detach_batched_seqs(*features, seq_len=seq_len), lambda: reference_detach(features, seq_len)],
                               args.warmup, args.repeats)
    packed_ms, padded_ms = packed_s * 1e3, padded_s * 1e3

    # the pack launch alone: LAUNCHES launches enqueued back to back between two device events, so that the device works through a
    # queue and the host's share of one call (allocation, descriptors, the ctypes call) is not inside the interval; interval / LAUNCHES
    kernel_times = []
    for i in range(args.warmup + args.repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ops.unpad_rows(features, seq_len, lens)              # the device is busy while the host enqueues the timed ones
        start.record()
        for _ in range(LAUNCHES):
            ops.unpad_rows(features, seq_len, lens)
        end.record()
        end.synchronize()
        if i >= args.warmup:
            kernel_times.append(start.elapsed_time(end) / LAUNCHES)
    kernel_ms = statistics.median(kernel_times)

    columns = sum(w for _, w in WIDTHS)
    packed_bytes = int(lens.sum()) * columns * 4
    padded_bytes = args.batch * t * columns * 4
    print(json.dumps({
        'workload': 'c5 lengths, %d utterances, T=%d, %d float32 columns in 4 features' % (args.batch, t, columns),
        'valid_frames': int(lens.sum()), 'padded_frames': args.batch * t, 'padding_share': round(1.0 - lens.sum() / (args.batch * t), 4),
        'detach_packed_ms': round(packed_ms, 3), 'detach_padded_reference_ms': round(padded_ms, 3),
        'pcie_bytes_packed': packed_bytes + args.batch * 8, 'pcie_bytes_padded_reference': padded_bytes + args.batch * 8,
        'unpad_launch_ms': round(kernel_ms, 4), 'unpad_launch_GBps': round(2 * packed_bytes / (kernel_ms * 1e-3) / 1e9, 1),
        'repeats': args.repeats, 'warmup': args.warmup}))


if __name__ == '__main__':
    main()
