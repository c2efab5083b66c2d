#!/usr/bin/env python
"""Cost of global gradient-norm clipping (``optim.Adam(max_grad_norm=)``, csrc/clip.hip) inside the training step.

For each of the bench's ``lstm``, ``f0gru`` and ``c2`` configurations (same models, batches and loop body as bench.py: 64 x 1000
frames for the recurrent models, 256 x 1000 for the F0Model) three optimisers are timed in turn on one rank, every step as ordinary
launches - a clipped step is not captured into a HIP graph, so ``c2``, which bench.py replays as a graph, is timed here in its eager
form on all three legs (its ``none`` leg is therefore NOT the bench's headline number):

    none    max_grad_norm=None   - the step as it is without the feature: the yardstick
    loose   max_grad_norm=1e30   - never bites: +2 launches per step, one read of the gradient; on c2 the slab deferral is off
    biting  max_grad_norm=1e-3   - always bites: + one read and one write of the gradient

``--rounds`` rounds, every round times ``--steps`` steps of each leg one after the other (the legs see the same moments of a shared
machine); the MEDIAN round of each leg is reported, with the gradient's size and the algorithmic bytes the clip moves.  Prints one
JSON line per configuration.  Not part of bench.py.

    python scripts/bench_clip.py [--configs lstm,f0gru,c2] [--steps 20] [--rounds 5] [--warmup 5] [--precision bf16]
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morgana_amd import data, models, ops, optim, synthetic  # noqa: E402
from morgana_amd import functional as F_hip  # noqa: E402

LEGS = (('none', None), ('loose', 1e30), ('biting', 1e-3))
WARM_STEPS_C2 = 200                       # an F0Model step is well under a millisecond: load the chip before the clock starts


def build(config, precision, dev, frames):
    """(model, features) of one bench configuration, as bench.py builds them."""
    torch.manual_seed(synthetic.REFERENCE_SEED)
    if config == 'c2':
        feats_np = synthetic.make_batch(256, frames)
        model, state = models.F0Model(precision=precision).to(dev), synthetic.f0_model_state()
    elif config == 'f0gru':
        feats_np = synthetic.make_acoustic_batch(64, frames, streams=(('lf0', 3, 'mse'),), with_raw=True)
        model, state = models.GRUF0Model(precision=precision).to(dev), synthetic.gru_f0_state()
    elif config == 'lstm':
        feats_np = synthetic.make_acoustic_batch(64, frames, with_raw=True)
        model, state = models.LSTMAcousticModel(precision=precision).to(dev), synthetic.lstm_acoustic_state()
    else:
        raise SystemExit('unknown configuration %r' % config)
    own = model.state_dict()
    for key, value in state.items():
        own[key].copy_(torch.from_numpy(value))
    if config in ('lstm', 'f0gru'):
        synthetic.acoustic_normalisers(model, device=dev)
        model.mode = 'train'
        model.metrics.reset_state('train')
    return model, data.to_device(feats_np, dev, bf16_tables=model.bf16_table_features()), int(feats_np['n_frames'].sum())


def make_leg(config, precision, dev, frames, max_grad_norm, steps):
    """(callable that performs ``per_call`` steps, per_call, optimiser, how it runs)."""
    model, features, n_frames = build(config, precision, dev, frames)
    optimizer = optim.Adam(model.parameters(), lr=0.01, fused_loop=True, max_grad_norm=max_grad_norm)

    def step():
        optimizer.zero_grad()
        loss, _ = model(features)
        F_hip.backward(loss)
        optimizer.step()
        return loss

    return step, 1, optimizer, 'eager launches', n_frames


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--configs', default='lstm,f0gru,c2')
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--warmup', type=int, default=5)
    parser.add_argument('--frames', type=int, default=1000)
    parser.add_argument('--precision', default='bf16', choices=['bf16', 'fp32', 'bf16x3'])
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_clip.py measures on an MI355X: no device found')
    dev = torch.device('cuda:0')
    for config in args.configs.split(','):
        legs = [make_leg(config, args.precision, dev, args.frames, c, args.steps) for _, c in LEGS]
        gc.collect()
        gc.disable()
        for call, per_call, _, how, _ in legs:
            warm = max(args.warmup, WARM_STEPS_C2 if config == 'c2' else 0)
            for _ in range(-(-warm // per_call)):
                call()
        torch.cuda.synchronize()
        times = [[] for _ in legs]
        for _ in range(args.rounds):
            for i, (call, per_call, _, _, _) in enumerate(legs):
                t0 = time.perf_counter()
                for _ in range(args.steps // per_call):
                    call()
                torch.cuda.synchronize()
                times[i].append((time.perf_counter() - t0) / (args.steps // per_call * per_call))
        gc.enable()
        ops.check_persistent_status()
        ms = [statistics.median(t) * 1e3 for t in times]
        n_grad = sum(f['grad'].numel() for f in legs[0][2]._flat if f is not None)
        norms = {name: [round(float(v), 6) for v in leg[2].grad_norms()[0].cpu()] for (name, c), leg in zip(LEGS, legs) if c is not None}
        record = {'config': config, 'precision': args.precision, 'how': legs[0][3], 'frames_per_step': legs[0][4],
                  'gradient_floats': n_grad, 'gradient_MB': round(n_grad * 4 / 1e6, 2),
                  'clip_bytes_loose': n_grad * 4, 'clip_bytes_biting': n_grad * 12,
                  'steps': args.steps, 'rounds': args.rounds}
        for (name, _), t, spread in zip(LEGS, ms, times):
            record['step_ms_' + name] = round(t, 4)
            record['step_ms_%s_min_max' % name] = [round(min(spread) * 1e3, 4), round(max(spread) * 1e3, 4)]
        record['loose_over_none'] = round(ms[1] / ms[0], 4)
        record['biting_over_none'] = round(ms[2] / ms[0], 4)
        record['last_norm_coef'] = norms
        print(json.dumps(record), flush=True)
        del legs
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
