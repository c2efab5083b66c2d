#!/usr/bin/env python
"""Synthesise waveforms from a directory of features with the package's WORLD-style synthesiser
(``viz.synthesis.synthesise_files``: csrc/synth.hip) - the step the reference did with ``world_with_reaper_f0.synthesis``.

    python scripts/synthesise.py IN_DIR OUT_DIR ID_LIST --sample-rate 48000 [--frame-period 5] [--alpha A] [--fft-size F]
                                 [--f0-window 7] [--max-batch-mib 256] [--overwrite] [--device cuda:0]

Reads, for the ids of ``ID_LIST`` (one per line), either ``IN_DIR/f0/{id}.npy``, ``IN_DIR/sp/{id}.npy`` and ``IN_DIR/ap/{id}.npy`` (an
analyser's arrays; taken when ``IN_DIR/sp`` exists) or ``IN_DIR/lf0``, ``vuv``, ``mcep`` and ``bap`` (what a model's
``analysis_for_valid_batch`` writes under ``feats/``), and writes ``OUT_DIR/{id}.wav`` (16-bit PCM).  ``--alpha`` and ``--fft-size``
apply to the coded features and default to Merlin's and WORLD's values for the rate.  An output that exists is refused unless
``--overwrite`` is given.  Prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morgana_amd import viz  # noqa: E402


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('in_dir')
    parser.add_argument('out_dir')
    parser.add_argument('id_list')
    parser.add_argument('--sample-rate', type=int, required=True)
    parser.add_argument('--frame-period', type=float, default=5.)
    parser.add_argument('--alpha', type=float, default=None)
    parser.add_argument('--fft-size', type=int, default=None)
    parser.add_argument('--f0-window', type=int, default=7)
    parser.add_argument('--max-batch-mib', type=int, default=256)
    parser.add_argument('--overwrite', action='store_true')
    parser.add_argument('--device', default='cuda:0')
    args = parser.parse_args()
    with open(args.id_list) as f:
        ids = [line.strip() for line in f if line.strip()]
    started = time.time()
    samples = viz.synthesis.synthesise_files(ids, args.in_dir, args.out_dir, args.sample_rate, frame_period=args.frame_period,
                                             alpha=args.alpha, fft_size=args.fft_size, f0_window=args.f0_window, device=args.device,
                                             max_batch_bytes=args.max_batch_mib << 20, overwrite=args.overwrite)
    print(json.dumps({'utterances': len(ids), 'samples': samples, 'seconds_of_audio': round(samples / float(args.sample_rate), 3),
                      'out_dir': args.out_dir, 'seconds': round(time.time() - started, 3)}))


if __name__ == '__main__':
    main()
