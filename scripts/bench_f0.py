#!/usr/bin/env python
"""Cost of the continuous log-F0 pass (``ops.continuous_lf0``, csrc/f0.hip) and of a loader that computes ``lf0`` / ``vuv`` /
``lf0_deltas`` from the raw F0 track.  Prints ONE JSON line.  Not part of bench.py.  Runs on the GPU only: there is no CPU path.

(a) Kernel figures on resident batches of B x 1000 x 1 frames, B = 64 and 256 (lengths uniform in [500, 1000], about 40 % of the
frames unvoiced, in runs of 5-80 frames), in turns:
    launch         the bare launch: packed f0 -> padded lf0 and vuv;
    loader         the launches a loader makes for an ``lf0`` + deltas feature from ``f0``: one mg_continuous_lf0_f32 (lf0, normalised
                   twin, vuv, the packed track) and one mg_deltas_f32 on that track (deltas and their normalised twin);
    pad_normalise  the yardstick: ``ops.pad_normalise`` of the PRECOMPUTED packed lf0 (with its normaliser), vuv and lf0_deltas -
                   what a loader fed the three files launches.  It writes the same tensors short of the deltas' twin.
Warmed, then ``--rounds`` rounds, each leg timed by device events around enough repetitions to fill ``--fill`` seconds; the median
round and the spread between rounds are reported.

(b) Loader figure (named ``loader``, NOT a kernel figure): ``DeviceBatches`` over in-memory raw utterances, ``lf0`` + ``vuv`` +
``lf0_deltas`` arrays as files would give them against the ``f0`` array alone with everything computed on the device: batches / s,
and the bytes a batch moves over PCIe counted from the shapes.

Every step is a child process of its own under its own time limit (``--limit`` seconds); after a step that fails or runs out of
time nothing more is started.

    python scripts/bench_f0.py [--batches 64,256] [--rounds 5] [--fill 0.3] [--no-loader]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FRAMES = 1000


def timed(call, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / reps


def make_track(rng, frames):
    """A raw F0 track (frames, 1): 80-400 Hz, about 40 % of the frames 0 in runs of 5-80 frames."""
    import numpy as np
    f0 = (80.0 + 320.0 * rng.rand(frames, 1)).astype(np.float32)
    at = 0
    while at < frames:
        run = int(rng.randint(5, 81))
        if rng.rand() < 0.4:
            f0[at:at + run] = 0.0
        at += run
    return f0


def kernel_worker(batch, rounds, fill):
    import numpy as np
    import torch
    from morgana_amd import data, ops
    from morgana_amd.viz import synthesis
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    windows = synthesis.DEFAULT_WINDOWS
    tracks = [make_track(rng, int(rng.randint(FRAMES // 2, FRAMES + 1))) for _ in range(batch)]
    lens = np.array([len(x) for x in tracks])
    total = int(lens.sum())
    offsets = torch.from_numpy(np.concatenate(([0], np.cumsum(lens))).astype(np.int64)).to(dev)
    f0 = torch.from_numpy(np.concatenate(tracks)).to(dev)
    p0, p1 = torch.randn(1, device=dev) + 5, torch.rand(1, device=dev) + 0.5
    d0, d1 = torch.randn(3, device=dev), torch.rand(3, device=dev) + 0.5
    # the precomputed features of the yardstick: what the three files would hold
    host = [data.continuous_lf0(x) for x in tracks]
    lf0 = torch.from_numpy(np.concatenate([h[0] for h in host])).to(dev)
    vuv = torch.from_numpy(np.concatenate([h[1] for h in host])).to(dev)
    wide = torch.from_numpy(np.concatenate([data.compute_deltas(h[0]) for h in host])).to(dev)

    def launch():
        return ops.continuous_lf0(f0, offsets=offsets, t=FRAMES)

    def loader():
        raw, norm, flag, track = ops.continuous_lf0(f0, offsets=offsets, t=FRAMES, want_packed=True, p0=p0, p1=p1, kind=ops.NORM_MVN)
        return raw, norm, flag, ops.deltas(track, windows, offsets=offsets, t=FRAMES, p0=d0, p1=d1, kind=ops.NORM_MVN)

    def yardstick():
        return (ops.pad_normalise(lf0, offsets, FRAMES, p0, p1, ops.NORM_MVN), ops.pad_normalise(vuv, offsets, FRAMES),
                ops.pad_normalise(wide, offsets, FRAMES))

    got, want = loader(), yardstick()
    assert torch.equal(got[2], want[1][0]), 'vuv differs from the host form'
    off = (got[0] - want[0][0]).abs().max().item()
    legs = {'launch': launch, 'loader': loader, 'pad_normalise': yardstick}
    reps = {}
    for name, call in legs.items():
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        reps[name] = max(3, min(5000, int(fill / max(timed(call, 3), 1e-7))))
    times = {name: [] for name in legs}
    for _ in range(rounds):
        for name, call in legs.items():
            times[name].append(timed(call, reps[name]))
    unvoiced = 1.0 - float(np.concatenate([h[1] for h in host]).mean())
    record = {'batch': batch, 'valid_frames': total, 'unvoiced': round(unvoiced, 3), 'lf0_max_abs_off_host_form': off, 'reps': reps,
              'launches': {'launch': 1, 'loader': 2, 'pad_normalise': 3}}
    for name in legs:
        record[name] = {'us': round(statistics.median(times[name]) * 1e6, 2),
                        'us_min_max': [round(min(times[name]) * 1e6, 2), round(max(times[name]) * 1e6, 2)]}
    record['loader_over_pad_normalise'] = round(statistics.median(times['loader']) / statistics.median(times['pad_normalise']), 3)
    return record


def loader_worker(utterances, batch_size, passes):
    import numpy as np
    import torch
    from morgana_amd import data
    rng = np.random.RandomState(1)
    normaliser = data.MeanVarianceNormaliser('lf0', use_deltas=True).set_params(
        {'mean': [5.0], 'std_dev': [0.4]}, {'mean': [5.0, 0.0, 0.0], 'std_dev': [0.4, 0.05, 0.03]})
    raw = [{'name': 'utt%04d' % i, 'f0': make_track(rng, int(rng.randint(FRAMES // 2, FRAMES + 1)))} for i in range(utterances)]
    with_files = []
    for item in raw:
        lf0, vuv = data.continuous_lf0(item['f0'])
        with_files.append({'name': item['name'], 'lf0': lf0, 'vuv': vuv, 'lf0_deltas': data.compute_deltas(lf0)})
    loaders = {'file_style': data.DeviceBatches(with_files, batch_size, {'lf0': normaliser}, 'cuda:0'),
               'computed': data.DeviceBatches(raw, batch_size, {'lf0': normaliser}, 'cuda:0', delta_specs={'lf0': data.DeltaSpec()},
                                              f0_specs={'lf0': data.F0Spec()})}

    def pcie_bytes(items):
        return sum(v.nbytes for item in items for v in item.values() if isinstance(v, np.ndarray)) // max(len(items) // batch_size, 1)

    def one_pass(loader):
        t0 = time.perf_counter()
        n = sum(1 for _ in loader)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    for loader in loaders.values():
        one_pass(loader)
    rates = {name: [] for name in loaders}
    for _ in range(passes):
        for name, loader in loaders.items():
            rates[name].append(one_pass(loader))
    a, b = (next(iter(loaders[name])) for name in ('file_style', 'computed'))
    median = {name: statistics.median(v) for name, v in rates.items()}
    return {'what': 'DeviceBatches over in-memory utterances, lf0 + vuv + lf0_deltas (host pack / PCIe bound, not a kernel figure)',
            'utterances': utterances, 'batch_size': batch_size, 'vuv_equal': bool(torch.equal(a['vuv'], b['vuv'])),
            'lf0_max_abs_difference': (a['lf0'] - b['lf0']).abs().max().item(),
            'batches_per_s': {name: round(v, 1) for name, v in median.items()},
            'batches_per_s_min_max': {name: [round(min(v), 1), round(max(v), 1)] for name, v in rates.items()},
            'pcie_bytes_per_batch': {'file_style': pcie_bytes(with_files), 'computed': pcie_bytes(raw)},
            'computed_over_file_style': round(median['computed'] / median['file_style'], 3)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--batches', default='64,256')
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--fill', type=float, default=0.3)
    parser.add_argument('--limit', type=float, default=120.0)
    parser.add_argument('--no-loader', action='store_true')
    parser.add_argument('--worker', default=None, help=argparse.SUPPRESS)
    args = parser.parse_args()
    if args.worker == 'loader':
        print(json.dumps(loader_worker(512, 64, 5)))
        return
    if args.worker is not None:
        print(json.dumps(kernel_worker(int(args.worker), args.rounds, args.fill)))
        return
    steps = args.batches.split(',') + ([] if args.no_loader else ['loader'])
    record = {'frames': FRAMES, 'kernel': [], 'loader': None, 'stopped_at': None}
    for step in steps:                                    # the parent never opens the device: every step is a fresh process
        command = [sys.executable, os.path.abspath(__file__), '--worker', step, '--rounds', str(args.rounds), '--fill', str(args.fill)]
        try:
            done = subprocess.run(command, stdout=subprocess.PIPE, universal_newlines=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            record['stopped_at'] = '%s: over %.0f s' % (step, args.limit)
            break
        if done.returncode != 0:
            record['stopped_at'] = '%s: exit status %d' % (step, done.returncode)
            break
        result = json.loads(done.stdout.strip().splitlines()[-1])
        if step == 'loader':
            record['loader'] = result
        else:
            record['kernel'].append(result)
    print(json.dumps(record), flush=True)
    if record['stopped_at'] is not None:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
