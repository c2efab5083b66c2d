#!/usr/bin/env python
"""Cost of the duration quantiser (``ops.quantise_durations``, csrc/durations.hip).  Prints ONE JSON line.  Not part of bench.py.  Runs
on the GPU only: there is no CPU path.

A resident prediction of 64 items, P = 80 phones of S = 1 and S = 5 states, in the normalised space of a mean-variance normaliser
(gamma-distributed durations), ragged ``n_phones``, a ``total`` per item.  Legs, in turns:
    carry, nearest              the one launch, as ``ops.quantise_durations`` makes it;
    carry_fitted                the same with ``total`` (two walks over the item);
    carry_replayed              the carry launch captured into a HIP graph and replayed: the device's share of a call, without the Python
                                wrapper and its four output allocations (the other legs are timed as Python issues them);
    data_carry                  through ``data.quantise_durations`` with the normaliser object (the operands' look-up and checks on the host);
    eager_nearest               the nearest rule as a composition of eager torch ops on the same device (denormalise in float64, clamp, round
                                to 16 fractional bits, shift, clamp, mask, two sums);
    eager_carry                 the carry rule likewise (``cumsum``, shift, ``cummax``, ``diff``).
The eager legs are the yardstick a user without the kernel would write; they are checked against the launch's bits here.
Warmed, then ``--rounds`` rounds, the legs alternating inside each round, each timed by device events around enough repetitions to
fill ``--fill`` seconds; the median round and the spread between rounds are reported.  No threshold: there is no earlier kernel.

Every step is a child process of its own under its own time limit (``--limit`` seconds); after a step that fails or runs out of
time nothing more is started.

    python scripts/bench_durations.py [--states 1,5] [--rounds 5] [--fill 0.3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCH, PHONES = 64, 80
LO, HI = 1, 200


def timed(call, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / reps


def kernel_worker(states, rounds, fill):
    import numpy as np
    import torch
    from morgana_amd import data, ops
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    frames = rng.gamma(2.0, 4.0 if states == 1 else 1.5, size=(BATCH, PHONES, states)) + 0.05
    mean, std_dev = (6.0 + rng.rand(states)).astype(np.float32), (4.0 + rng.rand(states)).astype(np.float32)
    pred = torch.from_numpy(((frames - mean) / std_dev).astype(np.float32)).to(dev)
    n_phones_np = rng.randint(PHONES // 2, PHONES + 1, size=BATCH).astype(np.int64)
    n_phones_np[0] = PHONES
    n_phones = torch.from_numpy(n_phones_np).to(dev)
    total = torch.from_numpy((n_phones_np * states * (9 if states == 1 else 4)).astype(np.int64)).to(dev)
    p0, p1 = torch.from_numpy(mean).to(dev), torch.from_numpy(std_dev).to(dev)
    normaliser = data.MeanVarianceNormaliser('dur').set_params({'mean': mean, 'std_dev': std_dev})
    valid = (torch.arange(PHONES, device=dev)[None, :] < n_phones[:, None])[:, :, None].expand(BATCH, PHONES, states).reshape(BATCH, -1)
    floor = torch.arange(1, PHONES * states + 1, device=dev, dtype=torch.int64)[None, :] * LO

    def fixed():
        x = pred.double() * p1.double() + p0.double()
        x = torch.where((x >= 0) & torch.isfinite(x), x, torch.zeros_like(x)).clamp(max=float(HI))
        return torch.floor(x * 65536.0 + 0.5).long().reshape(BATCH, -1) * valid

    def eager_nearest():
        d = (((fixed() + 32768) >> 16).clamp(min=LO) * valid).reshape(BATCH, PHONES, states)
        return d, d.sum(dim=2), d.sum(dim=(1, 2))

    def eager_carry():
        rounded = (torch.cumsum(fixed(), dim=1) + 32768) >> 16
        ends = floor + torch.cummax(rounded - floor, dim=1)[0].clamp(min=0)
        d = (torch.diff(ends, dim=1, prepend=torch.zeros((BATCH, 1), dtype=torch.int64, device=dev)) * valid).reshape(BATCH, PHONES, states)
        return d, d.sum(dim=2), d.sum(dim=(1, 2))

    def launch(rounding, fitted=False):
        return lambda: ops.quantise_durations(pred, n_phones=n_phones, p0=p0, p1=p1, lo=LO, hi=HI, rounding=rounding,
                                              total=total if fitted else None)

    legs = {'carry': launch('carry'), 'nearest': launch('nearest'), 'carry_fitted': launch('carry', True),
            'data_carry': lambda: data.quantise_durations(pred, n_phones=n_phones, normaliser=normaliser, min_frames=LO, max_frames=HI),
            'eager_nearest': eager_nearest, 'eager_carry': eager_carry}
    # the bare launch replayed from a captured graph: the device's share of a call, without the Python wrapper and its four allocations
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed = launch('carry')()
    legs['carry_replayed'] = graph.replay
    same = (all(torch.equal(a, b) for a, b in zip(legs['carry']()[:3], eager_carry())) and
            all(torch.equal(a, b) for a, b in zip(legs['nearest']()[:3], eager_nearest())) and
            all(torch.equal(a, b) for a, b in zip(legs['carry'](), legs['data_carry']())))
    graph.replay()
    same = same and all(torch.equal(a, b) for a, b in zip(legs['carry'](), replayed))
    fitted = legs['carry_fitted']()
    exact = int(((fitted[2] == total) | ((fitted[3] & ops.DUR_FLAG_PUSHED) != 0)).sum().item())
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
    record = {'states': states, 'batch_x_phones': [BATCH, PHONES], 'eager_legs_and_data_leg_equal_the_launch': bool(same),
              'fitted_items_at_their_total_or_flagged': [exact, BATCH], 'reps': reps}
    for name in legs:
        record[name] = {'us': round(statistics.median(times[name]) * 1e6, 2),
                        'us_min_max': [round(min(times[name]) * 1e6, 2), round(max(times[name]) * 1e6, 2)]}
    record['eager_carry_over_carry'] = round(statistics.median(times['eager_carry']) / statistics.median(times['carry']), 2)
    record['eager_nearest_over_nearest'] = round(statistics.median(times['eager_nearest']) / statistics.median(times['nearest']), 2)
    return record


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--states', default='1,5')
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--fill', type=float, default=0.3)
    parser.add_argument('--limit', type=float, default=120.0)
    parser.add_argument('--worker', default=None, help=argparse.SUPPRESS)
    args = parser.parse_args()
    if args.worker is not None:
        print(json.dumps(kernel_worker(int(args.worker), args.rounds, args.fill)))
        return
    record = {'kernel': [], 'stopped_at': None}
    for step in args.states.split(','):                   # the parent never opens the device: every step is a fresh process
        command = [sys.executable, os.path.abspath(__file__), '--worker', step, '--rounds', str(args.rounds), '--fill', str(args.fill)]
        try:
            done = subprocess.run(command, stdout=subprocess.PIPE, universal_newlines=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            record['stopped_at'] = '%s: over %.0f s' % (step, args.limit)
            break
        if done.returncode != 0:
            record['stopped_at'] = '%s: exit status %d' % (step, done.returncode)
            break
        record['kernel'].append(json.loads(done.stdout.strip().splitlines()[-1]))
    print(json.dumps(record), flush=True)
    if record['stopped_at'] is not None:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
