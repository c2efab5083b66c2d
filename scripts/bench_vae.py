"""What a latent costs: ms per training step of the shipped GRU F0 model, of its VAE form (models.VAEF0Model) and of the VAE's encoder
alone (forward + backward), at the f0gru shape of bench.py (64 x 1000 frames, bf16, with the per-step MLPG + LF0 metric), eager and
replayed as HIP graphs.  Prints one JSON line; ``overhead_ms`` = VAE step - GRU-F0 step - encoder, the part the latent conditioning,
the sampler and the KLD add (design bar: at most 5 % of the GRU-F0 step).

    python scripts/bench_vae.py [--steps 50] [--warmup 20] [--batch 64] [--frames 1000] [--precision bf16] [--only-vae]
"""
import argparse
import gc
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morgana_amd import data, graphs, models, optim, synthetic          # noqa: E402
from morgana_amd import functional as F_hip                             # noqa: E402


def _time(call, steps, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _model(cls, feats_np, precision, dev):
    model = cls(precision=precision).to(dev)
    if cls is models.GRUF0Model:
        own = model.state_dict()
        for key, value in synthetic.gru_f0_state().items():
            own[key].copy_(torch.from_numpy(value))
    synthetic.acoustic_normalisers(model, device=dev)
    model.mode = 'train'
    model.metrics.reset_state('train')
    return model, data.to_device(feats_np, dev, bf16_tables=model.bf16_table_features())


def _train_step(model, features):
    optimizer = optim.Adam(model.parameters(), lr=0.01, fused_loop=True)

    def step():
        optimizer.zero_grad()
        loss, _ = model(features)
        F_hip.backward(loss)
        optimizer.step()
        return loss
    return step, optimizer


def _measure_model(cls, feats_np, args, dev):
    model, features = _model(cls, feats_np, args.precision, dev)
    step, optimizer = _train_step(model, features)
    eager = _time(step, args.steps, args.warmup)
    graphed = graphs.GraphedTrainStep(model, optimizer, features)
    replay = _time(graphed, args.steps, args.warmup)
    return {'eager_ms': round(eager, 4), 'graph_ms': round(replay, 4)}


def _measure_encoder(feats_np, args, dev):
    model, features = _model(models.VAEF0Model, feats_np, args.precision, dev)
    grads = None

    def fwd_bwd():
        nonlocal grads
        mean, log_variance = model.encode(features)
        if grads is None:
            grads = (torch.ones_like(mean), torch.ones_like(log_variance))
        torch.autograd.backward((mean, log_variance), grads)
    eager = _time(fwd_bwd, args.steps, args.warmup)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fwd_bwd()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fwd_bwd()
    replay = _time(graph.replay, args.steps, args.warmup)
    return {'eager_ms': round(eager, 4), 'graph_ms': round(replay, 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--precision', default='bf16', choices=['fp32', 'bf16x3', 'bf16'])
    ap.add_argument('--only-vae', action='store_true', help='time the VAE step alone (for a kernel trace of it)')
    args = ap.parse_args()
    dev = 'cuda:0'
    torch.manual_seed(0)
    feats_np = synthetic.make_acoustic_batch(args.batch, args.frames, streams=(('lf0', 3, 'mse'),), with_raw=True)
    gc.collect()
    if args.only_vae:
        print(json.dumps({'shape': '%dx%d' % (args.batch, args.frames), 'precision': args.precision,
                          'vae_f0': _measure_model(models.VAEF0Model, feats_np, args, dev)}))
        return
    result = {'shape': '%dx%d' % (args.batch, args.frames), 'precision': args.precision, 'steps': args.steps, 'warmup': args.warmup,
              'gru_f0': _measure_model(models.GRUF0Model, feats_np, args, dev),
              'encoder_fwd_bwd': _measure_encoder(feats_np, args, dev),
              'vae_f0': _measure_model(models.VAEF0Model, feats_np, args, dev)}
    for kind in ('eager_ms', 'graph_ms'):
        over = result['vae_f0'][kind] - result['gru_f0'][kind] - result['encoder_fwd_bwd'][kind]
        result.setdefault('overhead_ms', {})[kind] = round(over, 4)
        result.setdefault('overhead_frac_of_gru_f0', {})[kind] = round(over / result['gru_f0'][kind], 4)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
