#!/usr/bin/env python
"""Cost of the vocoder-analysis kernels (csrc/analysis.hip) on the batch of scripts/bench_vocoder.py: 32 utterances of 300-2000 frames
(35 856 packed rows), FFT 2048 (1025 bins), 60 mel-cepstra at alpha 0.77, 5 aperiodicity bands at 48 kHz.  Prints ONE JSON line.  Not
part of bench.py.  Runs on the GPU only: there is no CPU path.

Legs, on the same packed rows, in turns:
    mcep_in64 / mcep_in32          ops.spectrum_mcep of a float64 / float32 power spectrum into a float32 output (one launch);
    torch_in64 / torch_in32        what a user would write today: ((0.5 * torch.log(sp.double())) @ table.T).float() - a pass that writes
                                   the logarithms, a float64 GEMM that re-reads them, a rounding pass;
    bap_in64 / bap_in32            ops.aperiodicity_bap;
    torch_bap_in64                 index_select of the two bins of every band, log10, clamp, lerp, .float().
Warmed, then ``--rounds`` rounds, each leg timed by device events around enough repetitions to fill ``--fill`` seconds; the median
round and the spread between rounds are reported, next to two floors counted from the launch: the bytes read over the project's
6.29 TB/s copy rate, and the float64 multiply-adds over the chip's float64 matrix peak of 78.6 TFLOP/s (the vendor's figure: cited,
not measured here).  ``--extract`` adds ``data.extract_world_features`` end to end over ``.npy`` files in a temporary directory
(float64 sp and ap: 294 MB per feature across the bus), wall clock, files in the page cache.

    python scripts/bench_analysis.py [--batch 32] [--rounds 5] [--fill 0.3] [--extract]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ORDER, FFT_SIZE, BANDS, SAMPLE_RATE, ALPHA = 60, 2048, 5, 48000, 0.77
COPY_BYTES_PER_S, F64_FLOP_PER_S = 6.29e12, 78.6e12


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
    parser.add_argument('--extract', action='store_true')
    args = parser.parse_args()
    import numpy as np
    import torch
    from morgana_amd import data, ops
    assert torch.cuda.is_available(), 'bench_analysis.py needs an MI355X'
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    lens = rng.randint(300, 2001, size=args.batch)
    rows, bins = int(lens.sum()), FFT_SIZE // 2 + 1
    ends = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    offsets = torch.from_numpy(ends).to(dev)
    c = rng.randn(rows, ORDER) / np.maximum(np.arange(ORDER), 1)[None, :]
    c[:, 0] = rng.uniform(-4, 4, size=rows)
    mcep = torch.from_numpy(c.astype(np.float32)).to(dev)
    sp64 = ops.mcep_spectrum(mcep, ALPHA, FFT_SIZE, offsets=offsets, out_dtype=torch.float64)      # a realistic envelope
    sp32 = sp64.float()
    ap64 = torch.from_numpy(10.0 ** (rng.uniform(-65.0, 0.0, size=(rows, bins)) / 20.0)).to(dev)
    ap32 = ap64.float()
    table = ops.mcep_analysis_matrix(ORDER, ALPHA, FFT_SIZE, dev)
    table_t = table.t().contiguous()
    out_mcep = torch.empty((rows, ORDER), dtype=torch.float32, device=dev)
    out_bap = torch.empty((rows, BANDS), dtype=torch.float32, device=dev)
    anchors = [divmod(3000 * (b + 1) * FFT_SIZE, SAMPLE_RATE) for b in range(BANDS)]
    k0 = torch.tensor([a[0] for a in anchors], dtype=torch.int64, device=dev)
    w = torch.tensor([a[1] / SAMPLE_RATE for a in anchors], dtype=torch.float64, device=dev)

    def torch_bap(ap):
        lo = (20.0 * torch.log10(ap.index_select(1, k0).double())).clamp(-60.0, 0.0)
        hi = (20.0 * torch.log10(ap.index_select(1, k0 + 1).double())).clamp(-60.0, 0.0)
        return torch.lerp(lo, hi, w).float()

    legs = {
        'mcep_in64': lambda: ops.spectrum_mcep(sp64, ORDER, ALPHA, offsets=offsets, out=out_mcep),
        'torch_in64': lambda: ((0.5 * torch.log(sp64)) @ table_t).float(),
        'mcep_in32': lambda: ops.spectrum_mcep(sp32, ORDER, ALPHA, offsets=offsets, out=out_mcep),
        'torch_in32': lambda: ((0.5 * torch.log(sp32.double())) @ table_t).float(),
        'bap_in64': lambda: ops.aperiodicity_bap(ap64, SAMPLE_RATE, BANDS, offsets=offsets, out=out_bap),
        'bap_in32': lambda: ops.aperiodicity_bap(ap32, SAMPLE_RATE, BANDS, offsets=offsets, out=out_bap),
        'torch_bap_in64': lambda: torch_bap(ap64),
    }
    in_bytes = {'mcep_in64': rows * bins * 8, 'torch_in64': rows * bins * 8, 'mcep_in32': rows * bins * 4, 'torch_in32': rows * bins * 4}
    ours, theirs = legs['mcep_in64']().clone(), legs['torch_in64']()
    worst = (ours - theirs).abs().max().item()
    back = (ours - mcep).abs().max().item()
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
    fma = rows * bins * ORDER
    record = {'batch': args.batch, 'rows': rows, 'order': ORDER, 'fft_size': FFT_SIZE, 'bins': bins, 'bands': BANDS, 'mcep_fma': fma,
              'logarithms': rows * bins, 'mcep_max_difference_from_torch': worst, 'mcep_max_difference_from_the_generating_cepstra': back,
              'floor_us': {'read_in64': round(rows * bins * 8 / COPY_BYTES_PER_S * 1e6, 1),
                           'read_in32': round(rows * bins * 4 / COPY_BYTES_PER_S * 1e6, 1),
                           'f64_fma_at_78.6_TFLOPs': round(2 * fma / F64_FLOP_PER_S * 1e6, 1)}, 'reps': reps}
    for name in legs:
        median = statistics.median(times[name])
        record[name] = {'us': round(median * 1e6, 2), 'us_min_max': [round(min(times[name]) * 1e6, 2), round(max(times[name]) * 1e6, 2)]}
        if name in in_bytes:
            record[name]['input_GB_per_s'] = round(in_bytes[name] / median * 1e-9, 1)
            record[name]['Gfma_per_s'] = round(fma / median * 1e-9, 1)
    for ours, theirs in (('mcep_in64', 'torch_in64'), ('mcep_in32', 'torch_in32'), ('bap_in64', 'torch_bap_in64')):
        record['%s_over_%s' % (ours, theirs)] = round(statistics.median(times[ours]) / statistics.median(times[theirs]), 3)
    if args.extract:
        sp_host, ap_host = sp64.cpu().numpy(), ap64.cpu().numpy()
        with tempfile.TemporaryDirectory() as root:
            for name in ('sp', 'ap'):
                os.makedirs(os.path.join(root, 'in', name))
            ids = ['utt%03d' % i for i in range(args.batch)]
            for i, utt in enumerate(ids):
                np.save(os.path.join(root, 'in', 'sp', utt + '.npy'), sp_host[ends[i]:ends[i + 1]])
                np.save(os.path.join(root, 'in', 'ap', utt + '.npy'), ap_host[ends[i]:ends[i + 1]])
            walls = []
            for _ in range(1 + min(args.rounds, 3)):
                started = time.perf_counter()
                data.extract_world_features(ids, os.path.join(root, 'in'), os.path.join(root, 'out'), SAMPLE_RATE, n_mcep=ORDER, alpha=ALPHA,
                                            n_bands=BANDS, device=dev, overwrite=True)
                walls.append(time.perf_counter() - started)
            walls = walls[1:]                                 # the first call builds the staging buffers
            record['extract'] = {'ms': round(statistics.median(walls) * 1e3, 1), 'ms_min_max': [round(min(walls) * 1e3, 1), round(max(walls) * 1e3, 1)],
                                 'input_MB': round(2 * rows * bins * 8 * 1e-6, 1),
                                 'input_GB_per_s': round(2 * rows * bins * 8 / statistics.median(walls) * 1e-9, 2)}
    print(json.dumps(record), flush=True)


if __name__ == '__main__':
    main()
