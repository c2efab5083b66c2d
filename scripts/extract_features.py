#!/usr/bin/env python
"""Code the spectra and aperiodicities of a corpus into the ``mcep`` and ``bap`` features the acoustic models read
(``data.extract_world_features``: csrc/analysis.hip) - the step ``tts_data_tools`` did with ``pysptk.sp2mc`` and
``pyworld.code_aperiodicity`` after the waveform analysis, which stays the user's.

    python scripts/extract_features.py IN_DIR OUT_DIR ID_LIST --sample-rate 48000 [--n-mcep 60] [--alpha A] [--n-bands N]
                                       [--max-batch-mib 256] [--overwrite] [--device cuda:0]

Reads ``IN_DIR/sp/{id}.npy`` and ``IN_DIR/ap/{id}.npy`` ((frames, fft_size / 2 + 1), float32 or float64, as an analyser such as
``pyworld.wav2world`` writes them) for the ids of ``ID_LIST`` (one per line) and writes ``OUT_DIR/mcep/{id}.npy`` and
``OUT_DIR/bap/{id}.npy``, float32.  ``--alpha`` defaults to Merlin's value for the rate, ``--n-bands`` to WORLD's rule.  ``lf0``, ``vuv``,
deltas and counters need no files: the loaders compute them from ``f0`` and ``dur``.  Prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morgana_amd import data  # noqa: E402


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('in_dir')
    parser.add_argument('out_dir')
    parser.add_argument('id_list')
    parser.add_argument('--sample-rate', type=int, required=True)
    parser.add_argument('--n-mcep', type=int, default=60)
    parser.add_argument('--alpha', type=float, default=None)
    parser.add_argument('--n-bands', type=int, default=None)
    parser.add_argument('--max-batch-mib', type=int, default=256)
    parser.add_argument('--overwrite', action='store_true')
    parser.add_argument('--device', default='cuda:0')
    args = parser.parse_args()
    with open(args.id_list) as f:
        ids = [line.strip() for line in f if line.strip()]
    started = time.time()
    frames = data.extract_world_features(ids, args.in_dir, args.out_dir, args.sample_rate, n_mcep=args.n_mcep, alpha=args.alpha,
                                         n_bands=args.n_bands, device=args.device, max_batch_bytes=args.max_batch_mib << 20,
                                         overwrite=args.overwrite)
    print(json.dumps({'utterances': len(ids), 'frames': frames, 'out_dir': args.out_dir, 'seconds': round(time.time() - started, 3)}))


if __name__ == '__main__':
    main()
