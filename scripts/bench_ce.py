"""What losses.ce costs: forward + backward of the masked categorical cross entropy (csrc/ce.hip) at 64 x 1000 frames for C = 64, 256
and 1024 classes (one wave per row), C = 2048 (one workgroup per row) and one ragged batch, against the reference's formulation in torch
eager on the same GPU in the same run (F.cross_entropy on the transposed logits, the mask, the sums, .backward()).

Per shape: ``ce_ms`` / ``torch_ms`` = median over ``--repeats`` device-timed windows of ``--steps`` forward + backward calls through
autograd (what a training step pays, host launches included); ``kernel_ms`` = the two launches of mg_masked_ce_f32 alone, replayed
from a HIP graph (device time); ``gb_s`` = the algorithmic bytes (logits of the valid frames read once, the whole gradient written once,
the int64 targets of the valid frames) over ``kernel_ms``; ``mse_gb_s`` = the same figure for mg_masked_mse_f32 on a (B, T, C)
prediction in the same run (reads two tensors, writes one); ``hbm_frac`` = gb_s over the 8 TB/s HBM figure of the MI355X.
Prints one JSON line.

    python scripts/bench_ce.py [--steps 20] [--warmup 10] [--repeats 7] [--batch 64] [--frames 1000]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morgana_amd import losses, ops                                     # noqa: E402

HBM_BYTES_PER_S = 8e12
REPLAY_CALLS = 10


def _median_ms(call, steps, warmup, repeats):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    windows = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            call()
        e1.record()
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) / steps)
    return statistics.median(windows)


def _graphed_ms(call, args):
    """Device time of one ``call``: REPLAY_CALLS of them captured into one HIP graph, the replay timed."""
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
    return _median_ms(graph.replay, args.steps, args.warmup, args.repeats) / REPLAY_CALLS


def _torch_ce(x, y, seq_len):
    frame = F.cross_entropy(x.transpose(1, 2), y, reduction='none').unsqueeze(-1)
    mask = (torch.arange(frame.shape[1], device=x.device)[None, :] < seq_len[:, None]).to(frame.dtype).unsqueeze(-1)
    return torch.mean(torch.sum(frame * mask, dim=1) / torch.sum(mask, dim=1))


def _measure(b, t, c, ragged, args, dev):
    rng = np.random.RandomState(c + ragged)
    x = torch.randn(b, t, c, device=dev, requires_grad=True)
    y = torch.from_numpy(rng.randint(0, c, size=(b, t))).to(dev)
    lens = rng.randint(t // 2, t + 1, size=b) if ragged else np.full(b, t)
    lens[0] = t
    seq_len = torch.from_numpy(lens.astype(np.int64)).to(dev)
    valid = int(lens.sum())

    def ours():
        x.grad = None
        losses.ce(x, y, seq_len).backward()

    def eager():
        x.grad = None
        _torch_ce(x, y, seq_len).backward()

    ours()
    got, got_grad = losses.ce(x, y, seq_len).item(), x.grad.clone()
    eager()
    want = _torch_ce(x, y, seq_len).item()
    assert abs(got - want) <= 1e-4 * abs(want), (got, want)
    assert (got_grad - x.grad).abs().max().item() <= 1e-4 * x.grad.abs().max().item()

    ce_ms = _median_ms(ours, args.steps, args.warmup, args.repeats)
    torch_ms = _median_ms(eager, args.steps, args.warmup, args.repeats)
    xd = x.detach()
    kernel_ms = _graphed_ms(lambda: ops.masked_ce(xd, y, seq_len, want_grad=True), args)
    target = torch.randn(b, t, c, device=dev)
    mse_ms = _graphed_ms(lambda: ops.masked_mse(xd, target, seq_len, want_grad=True), args)
    ce_bytes = valid * c * 4 + b * t * c * 4 + valid * 8
    mse_bytes = 3 * b * t * c * 4
    gb_s = ce_bytes / (kernel_ms * 1e-3) / 1e9
    return {'shape': '%dx%dx%d%s' % (b, t, c, ' ragged' if ragged else ''), 'valid_frames': valid, 'ce_ms': round(ce_ms, 4),
            'torch_ms': round(torch_ms, 4), 'speedup': round(torch_ms / ce_ms, 2), 'kernel_ms': round(kernel_ms, 4),
            'algorithmic_mb': round(ce_bytes / 1e6, 1), 'gb_s': round(gb_s, 1), 'hbm_frac': round(gb_s * 1e9 / HBM_BYTES_PER_S, 3),
            'mse_kernel_ms': round(mse_ms, 4), 'mse_gb_s': round(mse_bytes / (mse_ms * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--frames', type=int, default=1000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ce.py needs an MI355X'
    dev = 'cuda:0'
    torch.manual_seed(0)
    shapes = [(64, False), (256, False), (1024, False), (2048, False), (256, True)]
    result = {'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats, 'hbm_gb_s': HBM_BYTES_PER_S / 1e9,
              'shapes': [_measure(args.batch, args.frames, c, ragged, args, dev) for c, ragged in shapes]}
    print(json.dumps(result))


if __name__ == '__main__':
    main()
