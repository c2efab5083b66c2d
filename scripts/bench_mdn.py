#!/usr/bin/env python
"""Cost of ``losses.mdn`` (csrc/mdn.hip): forward plus backward of the masked mixture-density negative log likelihood on a RESIDENT
64 x 1000 batch at (K, D) = (8, 3) and (16, 3) (an lf0 stream) and (4, 180) (a mel-cepstrum stream, the bandwidth-bound shape), with
ragged lengths drawn from 300..2000 and clipped to T.

Four legs per shape, timed with device events in turn inside every round (they see the same moments of a shared machine):

    kernels  the two launches of mg_masked_mdn_f32 (``ops.masked_mdn``) replayed from a HIP graph: device time, no host in it
    direct   ``ops.masked_mdn`` called from Python: the same launches with their host cost
    wrapper  ``losses.mdn`` and ``torch.autograd.grad``: what a model pays, autograd's host work included
    eager    the same NLL composed of torch ops on the same device (log_softmax, exp, square, sum, logsumexp, the mask, the sums)
             and their autograd mirrors

The MEDIAN round of each leg is reported with the algorithmic bytes of the kernel (valid frames: 4 W read + 4 D target; every frame:
4 W gradient written; W = K (1 + 2 D)) and the rate they give against the 6.29 TB/s copy rate.  ``select``: ``ops.mdn_select`` replayed
from a graph likewise.  Last line: the shipped GRU F0 model's training step (64 x 1000 frames, MLPG and the LF0 metric inside, eager
launches) with its lf0 stream as masked MSE (``n_components=0``) and as an 8-component mixture.  One JSON line each.  Not part of bench.py.

    python scripts/bench_mdn.py [--steps 50] [--rounds 7] [--warmup 20] [--precision bf16]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morgana_amd import data, losses, models, ops, optim, synthetic  # noqa: E402
from morgana_amd import functional as F_hip  # noqa: E402

COPY_RATE = 6.29e12
SHAPES = ((8, 3), (16, 3), (4, 180))
BATCH, FRAMES = 64, 1000
REPLAY_CALLS = 10
HALF_LOG_2PI = 0.9189385332046727


def eager_mdn(x, y, seq_len, k):
    b, t, d = y.shape
    a, mu, s = x[:, :, :k], x[:, :, k:k + k * d].reshape(b, t, k, d), x[:, :, k + k * d:].reshape(b, t, k, d)
    z = (y[:, :, None, :] - mu) * torch.exp(-s)
    q = torch.log_softmax(a, dim=-1) - (0.5 * z * z + s).sum(dim=-1) - d * HALF_LOG_2PI
    frame = (-torch.logsumexp(q, dim=-1) / d).unsqueeze(-1)
    mask = (torch.arange(t, device=x.device)[None, :] < seq_len[:, None]).to(frame.dtype).unsqueeze(-1)
    return torch.mean(torch.sum(frame * mask, dim=1) / torch.sum(mask, dim=1))


def _graph_of(call):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(REPLAY_CALLS):
            call()
    return graph


def _time_legs(legs, args):
    """{name: [ms per call, one per round]}: the legs in turn inside every round; legs = [(name, call, calls per call())]."""
    for _, call, _ in legs:
        for _ in range(args.warmup):
            call()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, call, per in legs:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.steps):
                call()
            end.record()
            end.synchronize()
            times[name].append(start.elapsed_time(end) / (args.steps * per))
    return times


def measure_loss(k, d, args, dev):
    b, t, w = BATCH, FRAMES, k * (1 + 2 * d)
    rng = np.random.RandomState(20261019 + 1000 * k + d)
    lens = np.minimum(rng.randint(300, 2001, size=b), t).astype(np.int64)
    seq_len = torch.from_numpy(lens).to(dev)
    valid = int(lens.sum())
    y = torch.from_numpy(rng.standard_normal((b, t, d)).astype(np.float32)).to(dev)
    scale = min(1.0, 2.0 / np.sqrt(d))
    pred = np.concatenate((rng.standard_normal((b, t, k)), np.tile(y.cpu().numpy(), (1, 1, k)) + scale * rng.standard_normal((b, t, k * d)),
                           -0.5 + 0.5 * scale * rng.standard_normal((b, t, k * d))), axis=2).astype(np.float32)
    x = torch.from_numpy(pred).to(dev).requires_grad_(True)
    xd = x.detach()

    def wrapper():
        return torch.autograd.grad(losses.mdn(x, y, seq_len, n_components=k), x)[0]

    def direct():
        return ops.masked_mdn(xd, y, seq_len, k, want_grad=True)[1]

    def eager():
        return torch.autograd.grad(eager_mdn(x, y, seq_len, k), x)[0]

    want = eager()
    for name, call in (('wrapper', wrapper), ('direct', direct)):
        err = ((call() - want).abs().max() / want.abs().max()).item()
        assert err <= 1e-4, (name, err)
    kernels = _graph_of(direct)
    select = _graph_of(lambda: ops.mdn_select(xd, seq_len, k, d))
    legs = [('kernels', kernels.replay, REPLAY_CALLS), ('direct', direct, 1), ('wrapper', wrapper, 1), ('eager', eager, 1),
            ('select', select.replay, REPLAY_CALLS)]
    times = _time_legs(legs, args)
    n_bytes = valid * (4 * w + 4 * d) + b * t * 4 * w
    select_bytes = valid * 4 * (k + 2 * d) + b * t * (8 + 8 * d)
    record = {'K': k, 'D': d, 'W': w, 'batch': b, 'frames': t, 'valid_frames': valid, 'steps': args.steps, 'rounds': args.rounds,
              'loss_bytes': n_bytes, 'select_bytes': select_bytes}
    for name, _, _ in legs:
        ms = statistics.median(times[name])
        record['ms_' + name] = round(ms, 5)
        record['ms_%s_min_max' % name] = [round(min(times[name]), 5), round(max(times[name]), 5)]
    for name, size in (('kernels', n_bytes), ('direct', n_bytes), ('wrapper', n_bytes), ('select', select_bytes)):
        record['TBps_' + name] = round(size / (record['ms_' + name] * 1e-3) / 1e12, 4)
        record['share_of_copy_rate_' + name] = round(size / (record['ms_' + name] * 1e-3) / COPY_RATE, 4)
    record['eager_over_wrapper'] = round(record['ms_eager'] / record['ms_wrapper'], 2)
    record['eager_over_kernels'] = round(record['ms_eager'] / record['ms_kernels'], 2)
    return record


def measure_f0gru(args, dev):
    """The shipped GRU F0 model's step, lf0 as masked MSE and as an 8-component mixture: eager launches, the two in turn per round."""
    feats_np = synthetic.make_acoustic_batch(BATCH, FRAMES, streams=(('lf0', 3, 'mse'),), with_raw=True)
    legs = []
    for n_components in (0, 8):
        torch.manual_seed(synthetic.REFERENCE_SEED)
        model = models.GRUF0Model(precision=args.precision, n_components=n_components).to(dev)
        own = model.state_dict()
        for key, value in synthetic.gru_f0_state(output_dim=model.streams[0].width).items():
            own[key].copy_(torch.from_numpy(value))
        synthetic.acoustic_normalisers(model, device=dev)
        model.mode = 'train'
        model.metrics.reset_state('train')
        features = data.to_device(feats_np, dev, bf16_tables=model.bf16_table_features())
        optimizer = optim.Adam(model.parameters(), lr=0.01, fused_loop=True)

        def step(model=model, optimizer=optimizer, features=features):
            optimizer.zero_grad()
            loss, _ = model(features)
            F_hip.backward(loss)
            optimizer.step()
            return loss

        assert np.isfinite(step().item())
        legs.append(('n_components_%d' % n_components, step, 1))
    times = _time_legs(legs, args)
    record = {'f0gru_step': '%d x %d frames, %s, eager launches' % (BATCH, FRAMES, args.precision), 'steps': args.steps, 'rounds': args.rounds}
    for name, _, _ in legs:
        record['ms_' + name] = round(statistics.median(times[name]), 4)
        record['ms_%s_min_max' % name] = [round(min(times[name]), 4), round(max(times[name]), 4)]
    record['mixture_over_mse'] = round(record['ms_n_components_8'] / record['ms_n_components_0'], 3)
    return record


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--steps', type=int, default=50)
    parser.add_argument('--rounds', type=int, default=7)
    parser.add_argument('--warmup', type=int, default=20)
    parser.add_argument('--precision', default='bf16', choices=['bf16', 'fp32', 'bf16x3'])
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mdn.py measures on an MI355X: no device found')
    dev = torch.device('cuda:0')
    for k, d in SHAPES:
        print(json.dumps(measure_loss(k, d, args, dev)), flush=True)
    print(json.dumps(measure_f0gru(args, dev)), flush=True)


if __name__ == '__main__':
    main()
