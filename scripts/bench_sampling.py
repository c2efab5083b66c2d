"""What a draw of the latent surface samplers costs (morgana_amd.sampling, csrc/sampling.hip): ``rsample((rows,))`` of the sphere and the
ellipsoid sampler at rows = 64, 4 096, 65 536 and D = 16, 64, against the reference's formulation (sampling.py) written in torch ops
on the same GPU in the same run (randn / norm / divide; rand / sin / cos / cumprod / cat).

Per sampler and shape: ``eager_ms`` / ``torch_eager_ms`` = median over ``--repeats`` device-timed windows of ``--steps`` calls from the
host (launches included: what a caller of ``rsample`` pays); ``graph_ms`` / ``torch_graph_ms`` = the same call captured REPLAY_CALLS
times into one HIP graph, the replay timed, per call (device time).  Our replays draw new noise each time (the device step counter);
torch's captured generator does too.  Recorded, not gated: the samplers are not in the training step.  Prints one JSON line.

    python scripts/bench_sampling.py [--steps 50] [--warmup 10] [--repeats 7]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morgana_amd import ops, sampling                                   # noqa: E402

REPLAY_CALLS = 10
ROWS = (64, 4096, 65536)
DIMS = (16, 64)


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


def _torch_sphere(centre, radius, rows):
    direction = torch.randn(rows, centre.shape[0], device=centre.device)
    return centre + radius * (direction / torch.norm(direction, dim=-1, keepdim=True))


def _torch_ellipsoid(radii, rows):
    d = radii.shape[0]
    phi = torch.rand(rows, 1, device=radii.device) * (2 * math.pi)
    thetas = torch.rand(rows, max(0, d - 2), device=radii.device) * math.pi
    angles = torch.cat((phi, thetas), dim=-1)
    cumprod_sin = torch.cumprod(torch.sin(angles), dim=-1)
    cos = torch.cos(angles)
    pad = torch.ones_like(cumprod_sin[..., [0]])
    return radii * torch.cat((pad, cumprod_sin), dim=-1) * torch.cat((cos, pad), dim=-1)


def _measure(kind, rows, d, args, dev):
    centre = torch.randn(d, device=dev)
    radii = torch.rand(d, device=dev) + 0.5
    if kind == 'sphere':
        sampler = sampling.UniformSphereSurfaceSampler(centre, 2.0)
        radius = torch.full((1,), 2.0, device=dev)
        theirs = lambda: _torch_sphere(centre, radius, rows)
        dist = (sampler.rsample((rows,)) - centre).norm(dim=-1)
        assert (dist - 2.0).abs().max().item() < 1e-4
    else:
        sampler = sampling.UniformEllipsoidSurfaceApproximateSampler(centre, radii)
        theirs = lambda: _torch_ellipsoid(radii, rows)
        assert ((sampler.rsample((rows,)) / radii).norm(dim=-1) - 1.0).abs().max().item() < 1e-4
    ours = lambda: sampler.rsample((rows,))
    with torch.no_grad():
        result = {'sampler': kind, 'rows': rows, 'D': d,
                  'eager_ms': round(_median_ms(ours, args.steps, args.warmup, args.repeats), 4),
                  'torch_eager_ms': round(_median_ms(theirs, args.steps, args.warmup, args.repeats), 4),
                  'graph_ms': round(_graphed_ms(ours, args), 4),
                  'torch_graph_ms': round(_graphed_ms(theirs, args), 4)}
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_sampling.py needs an MI355X'
    dev = 'cuda:0'
    torch.manual_seed(0)
    ops.dropout_state(dev)
    result = {'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats, 'replay_calls': REPLAY_CALLS,
              'shapes': [_measure(kind, rows, d, args, dev) for kind in ('sphere', 'ellipsoid') for rows in ROWS for d in DIMS]}
    print(json.dumps(result))


if __name__ == '__main__':
    main()
