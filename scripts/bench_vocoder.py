#!/usr/bin/env python
"""Cost of the vocoder-feature kernels (csrc/vocoder.hip) at the shipped acoustic model's rate: a validation batch of 32 utterances
of 300-2000 frames, 60 mel-cepstra, FFT 2048 (1025 bins), 5 aperiodicity bands at 48 kHz.  Prints ONE JSON line.  Not part of
bench.py.  Runs on the GPU only: there is no CPU path.

Legs, on the same packed rows, in turns:
    spectrum_f32 / spectrum_f64        ops.mcep_spectrum into a float32 / float64 output (one launch);
    torch_f32                          the torch form of the same arithmetic, torch.exp(2 * (mcep @ basis)): a GEMM that writes the
                                       product and two elementwise passes that re-read it (float64: the same, then .double());
    aperiodicity_f32 / _f64            ops.bap_aperiodicity;
    f0_f64                             ops.smooth_f0 (window 7).
Warmed, then ``--rounds`` rounds, each leg timed by device events around enough repetitions to fill ``--fill`` seconds; the median
round and the spread between rounds are reported, with the output bytes per second (the output is the traffic) and, for the
spectrum, the fused multiply-adds per second counted from the shapes.

    python scripts/bench_vocoder.py [--batch 32] [--rounds 5] [--fill 0.3]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ORDER, FFT_SIZE, BANDS, SAMPLE_RATE, ALPHA = 60, 2048, 5, 48000, 0.77


def timed(call, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / reps


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--batch', type=int, default=32)
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--fill', type=float, default=0.3)
    args = parser.parse_args()
    import numpy as np
    import torch
    from morgana_amd import ops
    assert torch.cuda.is_available(), 'bench_vocoder.py needs an MI355X'
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    lens = rng.randint(300, 2001, size=args.batch)
    rows, bins = int(lens.sum()), FFT_SIZE // 2 + 1
    offsets = torch.from_numpy(np.concatenate(([0], np.cumsum(lens))).astype(np.int64)).to(dev)
    c = rng.randn(rows, ORDER) / np.maximum(np.arange(ORDER), 1)[None, :]
    c[:, 0] = rng.uniform(-4, 4, size=rows)
    mcep = torch.from_numpy(c.astype(np.float32)).to(dev)
    bap = torch.from_numpy(rng.uniform(-40, 0, size=(rows, BANDS)).astype(np.float32)).to(dev)
    lf0 = torch.from_numpy(rng.uniform(4.5, 5.5, size=(rows, 1)).astype(np.float32)).to(dev)
    vuv = torch.from_numpy((rng.rand(rows, 1) > 0.3).astype(np.float32)).to(dev)
    basis = ops.mcep_basis(ORDER, ALPHA, FFT_SIZE, dev)
    out32 = torch.empty((rows, bins), dtype=torch.float32, device=dev)
    out64 = torch.empty((rows, bins), dtype=torch.float64, device=dev)
    f0_out = torch.empty((rows, 1), dtype=torch.float64, device=dev)

    legs = {
        'spectrum_f32': lambda: ops.mcep_spectrum(mcep, ALPHA, FFT_SIZE, offsets=offsets, out=out32),
        'torch_f32': lambda: torch.exp(2 * (mcep @ basis)),
        'spectrum_f64': lambda: ops.mcep_spectrum(mcep, ALPHA, FFT_SIZE, offsets=offsets, out=out64, out_dtype=torch.float64),
        'torch_f64': lambda: torch.exp(2 * (mcep @ basis)).double(),
        'aperiodicity_f32': lambda: ops.bap_aperiodicity(bap, SAMPLE_RATE, FFT_SIZE, offsets=offsets, out=out32),
        'aperiodicity_f64': lambda: ops.bap_aperiodicity(bap, SAMPLE_RATE, FFT_SIZE, offsets=offsets, out=out64, out_dtype=torch.float64),
        'f0_f64': lambda: ops.smooth_f0(lf0, vuv, offsets=offsets, out=f0_out, out_dtype=torch.float64),
    }
    out_bytes = {'spectrum_f32': rows * bins * 4, 'torch_f32': rows * bins * 4, 'spectrum_f64': rows * bins * 8, 'torch_f64': rows * bins * 8,
                 'aperiodicity_f32': rows * bins * 4, 'aperiodicity_f64': rows * bins * 8, 'f0_f64': rows * 8}
    ours, theirs = legs['spectrum_f32']().clone(), legs['torch_f32']()
    worst = ((ours - theirs).abs() / theirs).max().item()
    reps = {}
    for name, call in legs.items():
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        reps[name] = max(3, min(5000, int(args.fill / max(timed(call, 3), 1e-7))))
    times = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, call in legs.items():
            times[name].append(timed(call, reps[name]))
    record = {'batch': args.batch, 'rows': rows, 'order': ORDER, 'fft_size': FFT_SIZE, 'bins': bins, 'bands': BANDS,
              'spectrum_fma': rows * bins * ORDER, 'spectrum_max_rel_difference_from_torch': worst, 'reps': reps}
    for name in legs:
        median = statistics.median(times[name])
        record[name] = {'us': round(median * 1e6, 2), 'us_min_max': [round(min(times[name]) * 1e6, 2), round(max(times[name]) * 1e6, 2)],
                        'output_GB_per_s': round(out_bytes[name] / median * 1e-9, 1)}
        if name.startswith(('spectrum', 'torch')):
            record[name]['Gfma_per_s'] = round(rows * bins * ORDER / median * 1e-9, 1)
    record['spectrum_f32_over_torch_f32'] = round(statistics.median(times['spectrum_f32']) / statistics.median(times['torch_f32']), 3)
    record['spectrum_f64_over_torch_f64'] = round(statistics.median(times['spectrum_f64']) / statistics.median(times['torch_f64']), 3)
    print(json.dumps(record), flush=True)


if __name__ == '__main__':
    main()
