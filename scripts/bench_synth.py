#!/usr/bin/env python
"""Cost of the waveform synthesis (csrc/synth.hip) on the batch of scripts/bench_vocoder.py: 32 utterances of 300-2000 frames
(35 856 frames, 5 ms each) at 16 kHz / FFT 1024 and at 48 kHz / FFT 2048.  Prints ONE JSON line.  Not part of bench.py.  Runs on the
GPU only: there is no CPU path.

Legs, per setting, in turns inside every round:
    synth            ops.world_synthesise from resident float64 f0 / sp / ap and a resident noise track into a float32 waveform: the
                     pulse kernel, the read of the (B,) pulse counts, then responses and overlap-add per pulse range;
    kernels          the same call's launches by name, from device events around each (``timings=``);
    torch_fft        the same definition for the same pulses (taken from the pulse kernel, outside the timing) composed of batched
                     float64 torch.fft calls, ``--chunk`` pulses at a time, overlap-add by index_add_;
    batch            viz.synthesis.synthesise_batch from the models' lf0 / vuv / mcep / bap to per-utterance host waveforms, wall clock;
    host_route       what the hook did before: viz.synthesis.world_features(as_numpy=True) - sp and ap as float64 to the host, the point
                     at which a host synthesiser would only start - wall clock.
Warmed, then ``--rounds`` rounds; the median round and the spread between rounds are reported.

    python scripts/bench_synth.py [--batch 32] [--rounds 7] [--chunk 4096]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SETTINGS = ((16000, 1024, 0.58, 1), (48000, 2048, 0.77, 5))      # rate, FFT, alpha, bands
ORDER, PERIOD = 60, 5.


def device_ms(call):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def wall_ms(call):
    import torch
    torch.cuda.synchronize()
    started = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return (time.perf_counter() - started) * 1e3, out


def torch_synth(f0, sp, ap, noise, plan, fs, fft_size, chunk):
    """Steps 4-8 of the definition for the pulses of ``plan`` in batched torch.fft calls."""
    import torch
    item, i_m, delta, period, voiced, frame_start, n_frames, sample_off, s_per, table = plan
    half, total = fft_size // 2, noise.shape[0]
    k = torch.arange(half + 1, dtype=torch.float64, device=sp.device)
    t = torch.arange(fft_size, device=sp.device)
    order = (t - half + 1) % fft_size
    fold = torch.zeros(fft_size, dtype=torch.float64, device=sp.device)
    fold[0], fold[1:half], fold[half] = 1., 2., 1.
    d = table[fft_size:]
    y = torch.zeros(total, dtype=torch.float64, device=sp.device)

    def minphase(p):
        c = torch.fft.irfft(.5 * torch.log(p), n=fft_size)
        return torch.exp(torch.fft.rfft(c * fold))

    for lo in range(0, item.shape[0], chunk):
        sl = slice(lo, lo + chunk)
        b, im, dl, tm, vo = item[sl], i_m[sl], delta[sl], period[sl], voiced[sl]
        last = (n_frames[b] - 1).double()
        u = torch.minimum(((im.double() - dl) / s_per).clamp_min(0.), last)
        j = torch.minimum(u.floor().long(), n_frames[b] - 1)
        j1 = torch.minimum(j + 1, n_frames[b] - 1)
        w = (u - j.double())[:, None]
        r0, r1 = frame_start[b] + j, frame_start[b] + j1
        s = (sp[r0] + (sp[r1] - sp[r0]) * w).clamp_min(0.)
        a = ap[r0] + (ap[r1] - ap[r0]) * w
        r = (a * a).clamp(0., 1.)
        vcol = vo[:, None]
        h_spec = minphase(s * (1. - r) + 1e-12) * torch.exp(1j * (2. * math.pi / fft_size) * dl[:, None] * k[None, :])
        g_spec = minphase(torch.where(vcol, s * r, s) + 1e-12)
        h = torch.fft.irfft(h_spec, n=fft_size)[:, order]
        h = (h - d[None, :] * h.sum(dim=1, keepdim=True)) * tm.double().sqrt()[:, None]
        start = sample_off[b] + im
        pos = (start[:, None] + t[None, :]).clamp_max(total - 1)
        e = torch.where(t[None, :] < tm[:, None], noise[pos], torch.zeros((), dtype=torch.float64, device=sp.device))
        shaped = torch.fft.irfft(torch.fft.rfft(e) * g_spec, n=fft_size)[:, order]
        x = torch.where(vcol, h, torch.zeros((), dtype=torch.float64, device=sp.device)) + shaped
        at = start[:, None] - half + 1 + t[None, :]
        ok = (at >= sample_off[b][:, None]) & (at < sample_off[b + 1][:, None])
        y.index_add_(0, at[ok], x[ok])
    return y.float()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--batch', type=int, default=32)
    parser.add_argument('--rounds', type=int, default=7)
    parser.add_argument('--chunk', type=int, default=4096)
    args = parser.parse_args()
    import numpy as np
    import torch
    from morgana_amd import ops, viz
    assert torch.cuda.is_available(), 'bench_synth.py needs an MI355X'
    dev = torch.device('cuda:0')
    record = {'batch': args.batch, 'rounds': args.rounds, 'chunk': args.chunk}
    for fs, fft_size, alpha, bands in SETTINGS:
        rng = np.random.RandomState(0)
        lens = rng.randint(300, 2001, size=args.batch)
        rows, t_max = int(lens.sum()), int(lens.max())
        c = rng.randn(args.batch, t_max, ORDER) / np.maximum(np.arange(ORDER), 1)[None, None, :]
        c[:, :, 0] = rng.uniform(-6, -2, size=(args.batch, t_max))
        mcep = torch.from_numpy(c.astype(np.float32)).to(dev)
        bap = torch.from_numpy(rng.uniform(-30., -1., size=(args.batch, t_max, bands)).astype(np.float32)).to(dev)
        contour = 5. + .3 * np.sin(np.arange(t_max)[None, :, None] / 40. + rng.rand(args.batch, 1, 1) * 6.)
        lf0 = torch.from_numpy(contour.astype(np.float32)).to(dev)
        vuv = torch.from_numpy((np.sin(np.arange(t_max)[None, :, None] / 23. + rng.rand(args.batch, 1, 1) * 6.) > -.5).astype(np.float32)).to(dev)
        per = viz.synthesis.world_features(lf0, vuv, mcep, bap, fs, lens, alpha=alpha, fft_size=fft_size, as_numpy=False)
        f0 = torch.cat([p[0] for p in per]).contiguous()
        sp = torch.cat([p[1] for p in per]).contiguous()
        ap = torch.cat([p[2] for p in per]).contiguous()
        offsets = np.concatenate(([0], np.cumsum(lens))).astype(np.int64).tolist()
        s_per = ops.synth_samples_per_frame(fs, PERIOD)
        total = sum(ops.synth_sample_counts(lens, s_per))
        noise = ops.synth_noise(total, 7, ops.dropout_draw(dev))

        def synth(timings=None, want_info=False):
            return ops.world_synthesise(f0, sp, ap, fs, PERIOD, offsets=offsets, noise=noise, timings=timings, want_info=want_info)

        wav, sample_off, info = synth(want_info=True)
        counts, region = info['counts'], info['region_offsets']
        keep = np.concatenate([np.arange(region[b], region[b] + counts[b]) for b in range(args.batch)])
        keep_d = torch.from_numpy(keep).to(dev)
        plan = (torch.from_numpy(np.repeat(np.arange(args.batch), counts)).to(dev), info['index'][keep_d].long(), info['delta'][keep_d],
                info['period'][keep_d].long(), info['voiced'][keep_d] != 0, torch.tensor(offsets[:-1], device=dev),
                torch.from_numpy(lens.astype(np.int64)).to(dev), sample_off, s_per, ops.synth_table_on(fft_size, dev))
        legs = {
            'synth': lambda: device_ms(synth)[0],
            'torch_fft': lambda: device_ms(lambda: torch_synth(f0, sp, ap, noise, plan, fs, fft_size, args.chunk))[0],
            'batch': lambda: wall_ms(lambda: viz.synthesis.synthesise_batch(lf0, vuv, mcep, bap, fs, lens, alpha=alpha, fft_size=fft_size))[0],
            'host_route': lambda: wall_ms(lambda: viz.synthesis.world_features(lf0, vuv, mcep, bap, fs, lens, alpha=alpha,
                                                                               fft_size=fft_size))[0],
        }
        theirs = torch_synth(f0, sp, ap, noise, plan, fs, fft_size, args.chunk)
        for call in legs.values():
            call()
        times = {name: [] for name in legs}
        kernels = {}
        for _ in range(args.rounds):
            for name, call in legs.items():
                times[name].append(call())
            marks = {}
            synth(timings=marks)
            torch.cuda.synchronize()
            for name, pairs in marks.items():
                kernels.setdefault(name, []).append(sum(a.elapsed_time(b) for a, b in pairs))
        entry = {'frames': rows, 'samples': total, 'seconds_of_audio': round(total / float(fs), 2), 'pulses': int(counts.sum()),
                 'ranges': len(info['ranges']), 'lds_bytes': 32 * fft_size,
                 'max_difference_from_torch_fft': float((wav - theirs).abs().max()), 'peak': float(wav.abs().max()),
                 'host_route_MB': round(2 * rows * (fft_size // 2 + 1) * 8e-6, 1), 'batch_MB_out': round(total * 4e-6, 1)}
        for name, values in list(times.items()) + list(kernels.items()):
            entry[name] = {'ms': round(statistics.median(values), 3), 'ms_min_max': [round(min(values), 3), round(max(values), 3)]}
        entry['real_time_factor'] = round(statistics.median(times['synth']) * 1e-3 / (total / float(fs)), 5)
        entry['synth_over_torch_fft'] = round(statistics.median(times['synth']) / statistics.median(times['torch_fft']), 3)
        record['%d_%d' % (fs, fft_size)] = entry
    print(json.dumps(record), flush=True)


if __name__ == '__main__':
    main()
