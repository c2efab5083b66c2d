#!/usr/bin/env python
"""Cost of the delta features (``ops.deltas``, csrc/deltas.hip) and of a loader that computes them.  Prints ONE JSON line.  Not part of
bench.py.  Runs on the GPU only: there is no CPU path.

(a) Kernel figure, B x T = 64 x 1000 frames (lengths uniform in [T/2, T]) for D = 1, 5, 60 and for the three of them as one batch's
three launches: ``ops.deltas`` on the packed statics (N, D) -> padded raw and normalised (B, T, 3 D), in turns with the yardstick,
``ops.pad_normalise`` on the PRECOMPUTED 3 D wide packed feature - an existing kernel that writes the same bytes and reads three times
as many.  Warmed, then ``--rounds`` rounds, each leg timed by device events around enough repetitions to fill ``--fill`` seconds; the
median round and the spread between rounds are reported.  bytes = statics read + both outputs written, from the shapes; bytes / s is
set against the 6.29 TB/s float4 copy rate measured on an MI355X.

(b) Loader figure (named ``loader``, NOT a kernel figure): ``DeviceBatches`` over in-memory raw utterances with the feature set of
``LSTMAcousticModel`` (lab 600, counters 9, dur, lf0 1, vuv 1, mcep 60, bap 5): the ``_deltas`` arrays in the utterances, as files would
give them, against statics only with the deltas computed on the device.  batches / s, and the bytes a batch moves over PCIe
counted from the shapes.

Every step is a child process of its own under its own time limit (``--limit`` seconds); after a step that fails or runs out of
time nothing more is started.

    python scripts/bench_deltas.py [--widths 1,5,60] [--rounds 5] [--fill 0.3] [--no-loader]
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

COPY_RATE = 6.29e12
BATCH, FRAMES = 64, 1000
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


def kernel_worker(widths, rounds, fill):
    import numpy as np
    import torch
    from morgana_amd import ops
    from morgana_amd.viz import synthesis
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    windows = synthesis.DEFAULT_WINDOWS
    lens = np.random.RandomState(0).randint(FRAMES // 2, FRAMES + 1, size=BATCH)
    offsets = torch.from_numpy(np.concatenate(([0], np.cumsum(lens))).astype(np.int64)).to(dev)
    total = int(lens.sum())
    jobs = []
    for d in widths:
        statics = torch.randn((total, d), device=dev) * 2.0 + 5.0
        p0, p1 = torch.randn(3 * d, device=dev), torch.rand(3 * d, device=dev) + 0.5
        wide, _ = ops.deltas(statics, windows, offsets=offsets, packed_rows=total)
        jobs.append((statics, wide, p0, p1))

    def deltas():
        return [ops.deltas(statics, windows, offsets=offsets, t=FRAMES, p0=p0, p1=p1, kind=ops.NORM_MVN) for statics, _, p0, p1 in jobs]

    def yardstick():
        return [ops.pad_normalise(wide, offsets, FRAMES, p0, p1, ops.NORM_MVN) for _, wide, p0, p1 in jobs]

    legs = {'deltas': deltas, 'pad_normalise': yardstick}
    for got, want in zip(deltas(), yardstick()):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), 'the two legs do not write the same values'
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
    seconds = {name: statistics.median(v) for name, v in times.items()}
    columns = sum(widths)
    written = 2 * BATCH * FRAMES * 3 * columns * 4
    n_bytes = {'deltas': total * columns * 4 + written, 'pad_normalise': total * 3 * columns * 4 + written}
    record = {'widths': list(widths), 'launches_per_leg': len(widths), 'valid_frames': total, 'reps': reps}
    for name in legs:
        record[name] = {'us': round(seconds[name] * 1e6, 2), 'us_min_max': [round(min(times[name]) * 1e6, 2), round(max(times[name]) * 1e6, 2)],
                        'bytes': n_bytes[name], 'TB_per_s': round(n_bytes[name] / seconds[name] / 1e12, 3),
                        'of_copy_rate': round(n_bytes[name] / seconds[name] / COPY_RATE, 4)}
    record['deltas_over_pad_normalise'] = round(seconds['deltas'] / seconds['pad_normalise'], 3)
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
    normalisers['counters'] = data.MinMaxNormaliser('counters').set_params({'mmin': np.zeros(9), 'mmax': np.ones(9)})
    for i in range(utterances):
        frames = int(rng.randint(FRAMES // 2, FRAMES + 1))
        phones = max(frames // 12, 1)
        item = {'name': 'utt%04d' % i, 'n_frames': frames, 'n_phones': phones,
                'lab': rng.rand(phones, 600).astype(np.float32), 'counters': rng.rand(frames, 9).astype(np.float32),
                'dur': rng.randint(1, 20, size=(phones, 1)).astype(np.int64), 'vuv': (rng.rand(frames, 1) > 0.3).astype(np.float32)}
        for name, width in DELTA_FEATURES:
            item[name] = (rng.randn(frames, width) * 2.0 + 5.0).astype(np.float32)
        raw.append(item)
    with_files = [dict(item, **{name + '_deltas': data.compute_deltas(item[name]) for name, _ in DELTA_FEATURES}) for item in raw]
    specs = {name: data.DeltaSpec() for name, _ in DELTA_FEATURES}
    loaders = {'file_style': data.DeviceBatches(with_files, batch_size, normalisers, 'cuda:0'),
               'computed': data.DeviceBatches(raw, batch_size, normalisers, 'cuda:0', delta_specs=specs)}

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
    same = all(torch.equal(a[key], b[key]) for key in a if isinstance(a[key], torch.Tensor))
    median = {name: statistics.median(v) for name, v in rates.items()}
    return {'what': 'DeviceBatches over in-memory utterances, LSTMAcousticModel features (host pack / PCIe bound, not a kernel figure)',
            'utterances': utterances, 'batch_size': batch_size, 'file_style_batches_equal_computed': bool(same),
            'batches_per_s': {name: round(v, 1) for name, v in median.items()},
            'batches_per_s_min_max': {name: [round(min(v), 1), round(max(v), 1)] for name, v in rates.items()},
            'pcie_bytes_per_batch': {'file_style': pcie_bytes(with_files), 'computed': pcie_bytes(raw)},
            'computed_over_file_style': round(median['computed'] / median['file_style'], 3)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--widths', default='1,5,60')
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
        print(json.dumps(kernel_worker([int(v) for v in args.worker.split('+')], args.rounds, args.fill)))
        return
    widths = args.widths.split(',')
    steps = widths + (['+'.join(widths)] if len(widths) > 1 else []) + ([] if args.no_loader else ['loader'])
    record = {'copy_rate_GB_per_s': COPY_RATE / 1e9, 'batch_x_frames': [BATCH, FRAMES], 'kernel': [], 'loader': None, 'stopped_at': None}
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
