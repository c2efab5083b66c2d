#!/usr/bin/env python
"""Cost of the corpus statistics (``data.ColumnStats.update_padded``, csrc/colstats.hip) on resident padded batches, and of the
file-backed ``data.fit_normalisers`` path.  Prints ONE JSON line.  Not part of bench.py.

Kernel figure, per shape B x T x D (default: 64x1000x3, 64x1000x187, 64x80x609, 256x1000x187; lengths uniform in [T/2, T]):
warmed, then ``--rounds`` rounds in which the kernel and the eager torch formulation of the same statistics (masked ``.double()``
mean, two-pass variance, ``amin`` / ``amax``) take turns on the same device, each timed by device events around enough repetitions
to fill ``--fill`` seconds; the median round is reported.  bytes = sum(len_b) * D * 4, from the shapes; bytes / s is set against
the 6.29 TB/s float4 copy rate measured on an MI355X.

File figure (named ``files``, NOT a kernel figure): ``fit_normalisers`` end to end over a generated corpus of ``.npy`` files in a
temporary directory - bounded by the file reads, the host pack and the copy to the device, not by the kernel.

Every step is a child process of its own under its own time limit (``--limit`` seconds); after a step that fails or runs out of
time nothing more is started.

    python scripts/bench_fit.py [--shapes 64x1000x3,64x1000x187,64x80x609,256x1000x187] [--rounds 5] [--fill 0.3] [--no-files]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

COPY_RATE = 6.29e12
DEFAULT_SHAPES = '64x1000x3,64x1000x187,64x80x609,256x1000x187'


def eager_stats(x, seq_len):
    import torch
    mask = (torch.arange(x.shape[1], device=x.device)[None, :] < seq_len[:, None])[:, :, None]
    n = seq_len.sum().double()
    wide = x.double()
    mean = (wide * mask).sum(dim=(0, 1)) / n
    var = (((wide - mean) * mask) ** 2).sum(dim=(0, 1)) / n
    inf = torch.tensor(float('inf'), device=x.device)
    return n, mean, var, torch.where(mask, x, inf).amin(dim=(0, 1)), torch.where(mask, x, -inf).amax(dim=(0, 1))


def timed(call, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / reps


def kernel_worker(shape, rounds, fill):
    import numpy as np
    import torch
    from morgana_amd import data
    b, t, d = (int(v) for v in shape.split('x'))
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    x = torch.randn((b, t, d), device=dev) * 1.5 + 3.0
    lens = np.random.RandomState(0).randint(t // 2, t + 1, size=b)
    seq_len = torch.from_numpy(lens.astype(np.int64)).to(dev)
    stats = data.ColumnStats(d, device=dev)
    legs = {'kernel': lambda: stats.update_padded(x, seq_len), 'eager': lambda: eager_stats(x, seq_len)}
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
    n_bytes = int(lens.sum()) * d * 4
    seconds = {name: statistics.median(v) for name, v in times.items()}
    got, want = stats.result(), eager_stats(x, seq_len)
    return {'shape': shape, 'bytes': n_bytes, 'padded_bytes': b * t * d * 4, 'reps': reps,
            'update_padded_us': round(seconds['kernel'] * 1e6, 2),
            'update_padded_us_min_max': [round(min(times['kernel']) * 1e6, 2), round(max(times['kernel']) * 1e6, 2)],
            'eager_torch_us': round(seconds['eager'] * 1e6, 2),
            'GB_per_s': round(n_bytes / seconds['kernel'] / 1e9, 1), 'of_copy_rate': round(n_bytes / seconds['kernel'] / COPY_RATE, 4),
            'eager_over_kernel': round(seconds['eager'] / seconds['kernel'], 2),
            'max_rel_var_diff_to_eager': float(np.max(np.abs(got['var'][0] - want[2].cpu().numpy()) / want[2].cpu().numpy()))}


def files_worker(utterances, frames, width):
    import numpy as np
    import torch
    from morgana_amd import data
    rng = np.random.RandomState(1)
    with tempfile.TemporaryDirectory() as root:
        names = ['utt%04d' % i for i in range(utterances)]
        n_bytes = 0
        for key, d in (('mcep', width), ('mcep_deltas', 3 * width)):
            os.makedirs(os.path.join(root, 'train', key))
        for name in names:
            n = int(rng.randint(frames // 2, frames + 1))
            for key, d in (('mcep', width), ('mcep_deltas', 3 * width)):
                np.save(os.path.join(root, 'train', key, name + '.npy'), (rng.randn(n, d) + 1.0).astype(np.float32))
                n_bytes += n * d * 4
        with open(os.path.join(root, 'ids.scp'), 'w') as f:
            f.write('\n'.join(names) + '\n')

        def fit(id_list):
            normalisers = {'mcep': data.MeanVarianceNormaliser('mcep', use_deltas=True)}
            dataset = data.FilesDataset({'mcep': data.NumpyBinarySource('mcep', use_deltas=True)}, 'train', id_list, normalisers,
                                        data_root=root)
            t0 = time.perf_counter()
            data.fit_normalisers(dataset, normalisers, device='cuda:0', out_dir='norm', data_root=root)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        with open(os.path.join(root, 'warm.scp'), 'w') as f:
            f.write('\n'.join(names[:8]) + '\n')
        fit('warm.scp')
        seconds = [fit('ids.scp') for _ in range(3)]       # the files are in the page cache from the second pass on
    best = min(seconds)
    return {'what': 'fit_normalisers end to end over .npy files (disk / host pack / PCIe bound, not a kernel figure)',
            'utterances': utterances, 'bytes': n_bytes, 'seconds': [round(s, 4) for s in seconds], 'GB_per_s_best': round(n_bytes / best / 1e9, 3)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--shapes', default=DEFAULT_SHAPES)
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--fill', type=float, default=0.3)
    parser.add_argument('--limit', type=float, default=120.0)
    parser.add_argument('--no-files', action='store_true')
    parser.add_argument('--worker', default=None, help=argparse.SUPPRESS)
    args = parser.parse_args()
    if args.worker == 'files':
        print(json.dumps(files_worker(128, 500, 60)))
        return
    if args.worker is not None:
        print(json.dumps(kernel_worker(args.worker, args.rounds, args.fill)))
        return
    steps = args.shapes.split(',') + ([] if args.no_files else ['files'])
    record = {'copy_rate_GB_per_s': COPY_RATE / 1e9, 'kernel': [], 'files': None, 'stopped_at': None}
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
        if step == 'files':
            record['files'] = result
        else:
            record['kernel'].append(result)
    print(json.dumps(record), flush=True)
    if record['stopped_at'] is not None:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
