"""What speaker-dependent normalisers cost: ms per training step of the shipped GRU F0 model (f0gru) and LSTM acoustic model (lstm) at
the shapes of bench.py (64 x 1000 frames, bf16, per-step MLPG + metrics) with SHARED normalisers and with SPEAKER-DEPENDENT ones
(8 speakers: the per-item denormalise, the row gather and MLPG's per-item variances), eager and replayed as HIP graphs.  Every
configuration is timed ``--repeats`` times in one process in the order shared -> speaker -> shared, so that the difference can be
read against the run-to-run spread of the shared step itself.  Prints one JSON line (and writes it to ``--out``).

    python scripts/bench_speakers.py [--steps 50] [--warmup 20] [--repeats 5] [--workloads f0gru lstm] [--out profiles/speakers_bench.json]
    python scripts/bench_speakers.py --only lstm-speaker      # the speaker-dependent lstm step alone, for a kernel trace of it
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

N_SPEAKERS = 8


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


WORKLOADS = {
    'f0gru': (models.GRUF0Model, synthetic.gru_f0_state, (('lf0', 3, 'mse'),)),
    'lstm': (models.LSTMAcousticModel, synthetic.lstm_acoustic_state, synthetic.ACOUSTIC_STREAMS),
}


def _build(workload, speakers, args, dev):
    cls, state_fn, streams = WORKLOADS[workload]
    feats_np = synthetic.make_acoustic_batch(args.batch, args.frames, streams=streams, with_raw=True)
    model = cls(precision=args.precision, speaker_id_list='speakers.scp' if speakers else None).to(dev)
    own = model.state_dict()
    for key, value in state_fn().items():
        own[key].copy_(torch.from_numpy(value))
    if speakers:
        synthetic.speaker_acoustic_normalisers(model, n_speakers=N_SPEAKERS, device=dev)
        feats_np['speaker_id'], _ = synthetic.speaker_batch_ids(args.batch, n_speakers=N_SPEAKERS)
    else:
        synthetic.acoustic_normalisers(model, device=dev)
    model.mode = 'train'
    model.metrics.reset_state('train')
    features = data.to_device(feats_np, dev, bf16_tables=model.bf16_table_features(), normalisers=model.normalisers)
    return model, features


def _measure(workload, speakers, args, dev):
    model, features = _build(workload, speakers, args, dev)
    optimizer = optim.Adam(model.parameters(), lr=0.01, fused_loop=True)

    def step():
        optimizer.zero_grad()
        loss, _ = model(features)
        F_hip.backward(loss)
        optimizer.step()

    eager = [_time(step, args.steps, args.warmup if i == 0 else 3) for i in range(args.repeats)]
    graphed = graphs.GraphedTrainStep(model, optimizer, features)
    replay = [_time(graphed, args.steps, args.warmup if i == 0 else 3) for i in range(args.repeats)]
    del model, features, optimizer, graphed
    gc.collect()
    torch.cuda.empty_cache()
    return {'eager_ms': [round(v, 4) for v in eager], 'graph_ms': [round(v, 4) for v in replay]}


def _summary(shared_runs, speaker_run):
    out = {}
    for kind in ('eager_ms', 'graph_ms'):
        shared = [v for run in shared_runs for v in run[kind]]
        speaker = speaker_run[kind]
        mid = lambda xs: sorted(xs)[len(xs) // 2]
        out[kind] = {'shared_median': mid(shared), 'shared_min': min(shared), 'shared_max': max(shared),
                     'speaker_median': mid(speaker), 'speaker_min': min(speaker), 'speaker_max': max(speaker),
                     'difference_of_medians': round(mid(speaker) - mid(shared), 4), 'shared_spread': round(max(shared) - min(shared), 4)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--precision', default='bf16', choices=['fp32', 'bf16x3', 'bf16'])
    ap.add_argument('--workloads', nargs='+', default=['f0gru', 'lstm'], choices=sorted(WORKLOADS))
    ap.add_argument('--only', default=None, help="'<workload>-speaker' or '<workload>-shared': time that step alone (for a kernel trace)")
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_speakers.py measures on an MI355X: no device found')
    dev = 'cuda:0'
    torch.manual_seed(0)
    if args.only:
        workload, _, which = args.only.partition('-')
        print(json.dumps({args.only: _measure(workload, which == 'speaker', args, dev)}))
        return
    result = {'shape': '%dx%d' % (args.batch, args.frames), 'precision': args.precision, 'steps': args.steps, 'warmup': args.warmup,
              'repeats': args.repeats, 'speakers': N_SPEAKERS, 'order': ['shared', 'speaker', 'shared']}
    for workload in args.workloads:
        first = _measure(workload, False, args, dev)
        speaker = _measure(workload, True, args, dev)
        second = _measure(workload, False, args, dev)
        result[workload] = {'shared_first': first, 'speaker': speaker, 'shared_second': second, 'summary': _summary([first, second], speaker)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
