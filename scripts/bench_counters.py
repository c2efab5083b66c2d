#!/usr/bin/env python
"""Cost of the frame-level positional features (``ops.frame_counters``, csrc/counters.hip) and of a loader that computes ``counters``
from the durations.  Prints ONE JSON line.  Not part of bench.py.  Runs on the GPU only: there is no CPU path.

(a) Kernel figures on a resident batch of 64 x 1000 frames, P = 80 phones of S = 1 and S = 5 states (every utterance exactly 1000
frames: random cuts of the 1000 frames into P * S segments, about one in ten empty), raw + normalised outputs, in turns:
    blocks_N       the one launch with N workgroups per item (``blocks_per_item``): 1 - one workgroup per item - 2, 4, 8, 12, 16, 24, 36 (one element per thread);
    default        the launch as the loaders make it (the library's choice of N);
    pad_normalise  the yardstick, the parent's route on the same device: ``ops.pad_normalise`` over the nine PRECOMPUTED, uploaded
                   columns (with their normaliser).  It writes the same two tensors.
Warmed, then ``--rounds`` rounds, the legs alternating inside each round, each timed by device events around enough repetitions to
fill ``--fill`` seconds; the median round and the spread between rounds are reported.

(b) Loader figure (named ``loader``, NOT a kernel figure): ``DeviceBatches`` over in-memory raw utterances with the feature set of
``LSTMAcousticModel`` (lab 600, counters 9, dur, lf0 / mcep / bap with their deltas, vuv): the ``counters`` array in the utterances, as
files would give it, against no such array with the counters computed on the device.  batches / s, and the bytes a batch moves
over PCIe counted from the shapes.

Every step is a child process of its own under its own time limit (``--limit`` seconds); after a step that fails or runs out of
time nothing more is started.

    python scripts/bench_counters.py [--states 1,5] [--rounds 5] [--fill 0.3] [--no-loader]
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

BATCH, FRAMES, PHONES = 64, 1000, 80
BLOCKS = (1, 2, 4, 8, 12, 16, 24, 36)
DELTA_FEATURES = (('lf0', 1), ('mcep', 60), ('bap', 5))


def timed(call, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / reps


def cut_frames(rng, frames, segments):
    """``segments`` non-negative integers that add up to ``frames``: a random cut, about one segment in ten empty."""
    import numpy as np
    cuts = np.sort(rng.randint(0, frames + 1, size=segments - 1))
    lens = np.diff(np.concatenate(([0], cuts, [frames])))
    empty = np.flatnonzero(rng.rand(segments) < 0.1)
    for k in empty:                                       # an emptied segment's frames go to its neighbour
        lens[(k + 1) % segments] += lens[k]
        lens[k] = 0
    assert lens.sum() == frames and (lens >= 0).all()
    return lens.astype(np.int64)


def kernel_worker(states, rounds, fill):
    import numpy as np
    import torch
    from morgana_amd import data, ops
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    durs = np.stack([cut_frames(rng, FRAMES, PHONES * states).reshape(PHONES, states) for _ in range(BATCH)])
    dur = torch.from_numpy(durs).to(dev)
    seq_len = torch.full((BATCH,), FRAMES, dtype=torch.int64, device=dev)
    p0, p1 = torch.zeros(9, device=dev), torch.full((9,), 50.0, device=dev)
    host = [data.frame_counters(d) for d in durs]         # the precomputed feature of the yardstick: what the files would hold
    packed = torch.from_numpy(np.concatenate(host)).to(dev)
    offsets = torch.from_numpy(np.arange(BATCH + 1, dtype=np.int64) * FRAMES).to(dev)

    def launch(blocks):
        return lambda: ops.frame_counters(dur, t=FRAMES, seq_len=seq_len, p0=p0, p1=p1, norm_kind=ops.NORM_MINMAX, blocks_per_item=blocks)

    def yardstick():
        return ops.pad_normalise(packed, offsets, FRAMES, p0, p1, ops.NORM_MINMAX)

    legs = {'blocks_%d' % n: launch(n) for n in BLOCKS}
    legs['default'] = launch(None)
    legs['pad_normalise'] = yardstick
    want = yardstick()
    same = all(torch.equal(a, b) for name, call in legs.items() for a, b in zip(call(), want))
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
    record = {'states': states, 'batch_x_frames_x_phones': [BATCH, FRAMES, PHONES], 'output_bytes': 2 * BATCH * FRAMES * 9 * 4,
              'every_leg_equals_pad_normalise_of_the_host_form': bool(same), 'reps': reps}
    for name in legs:
        record[name] = {'us': round(statistics.median(times[name]) * 1e6, 2),
                        'us_min_max': [round(min(times[name]) * 1e6, 2), round(max(times[name]) * 1e6, 2)]}
    record['default_over_pad_normalise'] = round(statistics.median(times['default']) / statistics.median(times['pad_normalise']), 3)
    return record


def loader_worker(utterances, batch_size, passes):
    import numpy as np
    import torch
    from morgana_amd import data
    rng = np.random.RandomState(1)
    normalisers, raw = {}, []
    for name, width in DELTA_FEATURES:
        normalisers[name] = data.MeanVarianceNormaliser(name, use_deltas=True).set_params(
            {'mean': rng.randn(width), 'std_dev': rng.rand(width) + 0.5}, {'mean': rng.randn(3 * width), 'std_dev': rng.rand(3 * width) + 0.5})
    normalisers['lab'] = data.MinMaxNormaliser('lab').set_params({'mmin': np.zeros(600), 'mmax': np.ones(600)})
    normalisers['counters'] = data.MinMaxNormaliser('counters').set_params({'mmin': np.zeros(9), 'mmax': np.full(9, 50.0)})
    for i in range(utterances):
        frames = int(rng.randint(FRAMES // 2, FRAMES + 1))
        phones = max(frames // 12, 1)
        item = {'name': 'utt%04d' % i, 'n_frames': frames, 'n_phones': phones, 'lab': rng.rand(phones, 600).astype(np.float32),
                'dur': cut_frames(rng, frames, phones).reshape(phones, 1), 'vuv': (rng.rand(frames, 1) > 0.3).astype(np.float32)}
        for name, width in DELTA_FEATURES:
            item[name] = (rng.randn(frames, width) * 2.0 + 5.0).astype(np.float32)
            item[name + '_deltas'] = data.compute_deltas(item[name])
        raw.append(item)
    with_files = [dict(item, counters=data.frame_counters(item['dur'])) for item in raw]
    loaders = {'file_style': data.DeviceBatches(with_files, batch_size, normalisers, 'cuda:0'),
               'computed': data.DeviceBatches(raw, batch_size, normalisers, 'cuda:0', counter_specs={'counters': data.CountersSpec()})}

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
    same = sorted(a) == sorted(b) and all(torch.equal(a[key], b[key]) for key in a if isinstance(a[key], torch.Tensor))
    median = {name: statistics.median(v) for name, v in rates.items()}
    return {'what': 'DeviceBatches over in-memory utterances, LSTMAcousticModel features (host pack / PCIe bound, not a kernel figure)',
            'utterances': utterances, 'batch_size': batch_size, 'file_style_batches_equal_computed': bool(same),
            'batches_per_s': {name: round(v, 1) for name, v in median.items()},
            'batches_per_s_min_max': {name: [round(min(v), 1), round(max(v), 1)] for name, v in rates.items()},
            'pcie_bytes_per_batch': {'file_style': pcie_bytes(with_files), 'computed': pcie_bytes(raw)},
            'computed_over_file_style': round(median['computed'] / median['file_style'], 3)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--states', default='1,5')
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--fill', type=float, default=0.3)
    parser.add_argument('--limit', type=float, default=120.0)
    parser.add_argument('--no-loader', action='store_true')
    parser.add_argument('--worker', default=None, help=argparse.SUPPRESS)
    args = parser.parse_args()
    if args.worker == 'loader':
        print(json.dumps(loader_worker(256, 64, 5)))
        return
    if args.worker is not None:
        print(json.dumps(kernel_worker(int(args.worker), args.rounds, args.fill)))
        return
    steps = args.states.split(',') + ([] if args.no_loader else ['loader'])
    record = {'kernel': [], 'loader': None, 'stopped_at': None}
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
