#!/usr/bin/env python
"""Fit normaliser parameter files to a corpus of ``.npy`` features (``data.fit_normalisers``: per-column statistics on the device,
csrc/colstats.hip) - the files ``data.Normalisers`` and ``load_params`` read, which the reference takes from ``tts_data_tools``.

    python scripts/fit_normalisers.py DATA_ROOT DATA_DIR ID_LIST NAME:KIND[:deltas[=compute]][:from=F0][:counters=DUR[,full|phone]] [NAME:KIND... ...]
                                      [--speaker-id-list FILE] [--out-dir DIR] [--batch-size 64] [--ddof 0] [--device cuda:0]

``KIND`` is ``mvn`` or ``minmax``; ``:deltas`` also fits ``{NAME}_deltas`` from the files of ``DATA_ROOT/DATA_DIR/NAME_deltas``;
``:deltas=compute`` fits it without such files: the deltas are computed on the device from the statics (csrc/deltas.hip; default
windows, replicated edges - ``data.compute_deltas``).  ``:from=F0`` (``lf0:mvn:deltas=compute:from=f0``) fits a continuous log-F0 feature
without ``NAME`` files: the raw F0 track ``DATA_ROOT/DATA_DIR/F0/*.npy`` is read and interpolated on the device (csrc/f0.hip -
``data.continuous_lf0``), the statistics cover every frame, and its deltas are always computed.  ``:counters=DUR``
(``counters:minmax:counters=dur``, ``counters:minmax:counters=state_dur,full``) fits a frame-level positional feature without ``NAME`` files:
the integer durations ``DATA_ROOT/DATA_DIR/DUR/*.npy`` - ``(P, 1)`` phone or ``(P, S)`` state durations - are read and the counters computed
on the device (csrc/counters.hip - ``data.frame_counters``; ``,full`` the nine columns, the default, ``,phone`` the three); such a feature
has no deltas.  Features are read from ``DATA_ROOT/DATA_DIR/NAME/*.npy``
for the ids of ``DATA_ROOT/ID_LIST``.  With ``--speaker-id-list`` (relative to DATA_ROOT) every normaliser is speaker dependent: the
speaker of an utterance is read from ``DATA_ROOT/DATA_DIR/speaker_id/*.txt`` and the files go to ``{speaker}/``.  The files are
written under ``DATA_ROOT/OUT_DIR`` (default: DATA_DIR, where the reference's ``--normalisation_dir train`` looks for them).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morgana_amd import data  # noqa: E402

CLASSES = {('mvn', False): data.MeanVarianceNormaliser, ('minmax', False): data.MinMaxNormaliser,
           ('mvn', True): data.SpeakerDependentMeanVarianceNormaliser, ('minmax', True): data.SpeakerDependentMinMaxNormaliser}


def parse_spec(spec, speaker_id_list):
    """``NAME:KIND[:deltas[=compute]][:from=F0][:counters=DUR[,KIND]]`` -> (name, normaliser, 'file' or 'compute', what the feature is
    computed from: None - its own files -, the raw F0 track's name, or a ``data.CountersSpec`` naming the durations)."""
    name, _, rest = spec.partition(':')
    kind, _, options = rest.partition(':')
    options = options.split(':') if options else []
    counters = [option[len('counters='):] for option in options if option.startswith('counters=')]
    if counters:
        dur_name, comma, counters_kind = counters[0].partition(',')
        if (not name or kind not in ('mvn', 'minmax') or len(options) > 1 or not dur_name or dur_name == name or (comma and not counters_kind)
                or (counters_kind or 'full') not in ('full', 'phone')):
            raise SystemExit('cannot read %r: expected NAME:KIND:counters=DUR, NAME:KIND:counters=DUR,full or NAME:KIND:counters=DUR,phone, DUR '
                             'another feature name, KIND mvn or minmax, and no other option (counters have no deltas)' % spec)
        cls = CLASSES[kind, speaker_id_list is not None]
        extra = (speaker_id_list,) if speaker_id_list is not None else ()
        return name, cls(name, *extra), 'file', data.CountersSpec(source=dur_name, kind=counters_kind or 'full')
    source = [option[len('from='):] for option in options if option.startswith('from=')]
    deltas = [option for option in options if not option.startswith('from=')]
    if (not name or kind not in ('mvn', 'minmax') or len(deltas) > 1 or len(source) > 1 or (deltas and deltas[0] not in ('deltas', 'deltas=compute'))
            or (source and (not source[0] or source[0] == name))):
        raise SystemExit('cannot read %r: expected NAME:KIND, NAME:KIND:deltas or NAME:KIND:deltas=compute, each optionally followed by '
                         ':from=F0 (another feature name), KIND mvn or minmax' % spec)
    if source and deltas == ['deltas']:
        raise SystemExit('cannot read %r: the deltas of a feature computed from %r are computed too: write deltas=compute' % (spec, source[0]))
    cls = CLASSES[kind, speaker_id_list is not None]
    extra = (speaker_id_list,) if speaker_id_list is not None else ()
    return name, cls(name, *extra, use_deltas=bool(deltas)), 'compute' if deltas == ['deltas=compute'] else 'file', source[0] if source else None


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('data_root')
    parser.add_argument('data_dir')
    parser.add_argument('id_list')
    parser.add_argument('features', nargs='+', metavar='NAME:KIND[:deltas[=compute]][:from=F0][:counters=DUR[,full|phone]]')
    parser.add_argument('--speaker-id-list', default=None)
    parser.add_argument('--out-dir', default=None)
    parser.add_argument('--batch-size', type=int, default=64)
    parser.add_argument('--ddof', type=int, default=0)
    parser.add_argument('--device', default='cuda:0')
    args = parser.parse_args()
    specs = [parse_spec(spec, args.speaker_id_list) for spec in args.features]
    normalisers = {name: normaliser for name, normaliser, _, _ in specs}
    sources = {}
    for name, normaliser, deltas, computed_from in specs:
        if computed_from is None:
            sources[name] = data.NumpyBinarySource(name, use_deltas=normaliser.use_deltas, deltas=deltas)
        elif isinstance(computed_from, data.CountersSpec):
            sources[name] = data.FrameCountersSource(name, dur_name=computed_from.source, kind=computed_from.kind)
        else:
            sources[name] = data.ContinuousLF0Source(name, f0_name=computed_from, vuv_name=name + '_vuv', use_deltas=normaliser.use_deltas)
    for name, _, _, computed_from in specs:               # the durations counters are computed from, unless they are fitted as well
        if isinstance(computed_from, data.CountersSpec) and computed_from.source not in sources:
            sources[computed_from.source] = data.NumpyBinarySource(computed_from.source)
    if args.speaker_id_list is not None:
        sources[data.SPEAKER_ID_KEY] = data.StringSource(data.SPEAKER_ID_KEY)
    dataset = data.FilesDataset(sources, args.data_dir, args.id_list, normalisers, data_root=args.data_root)
    out_dir = args.data_dir if args.out_dir is None else args.out_dir
    results = data.fit_normalisers(dataset, normalisers, device=args.device, batch_size=args.batch_size, out_dir=out_dir,
                                   data_root=args.data_root, ddof=args.ddof)
    print(json.dumps({'utterances': len(dataset), 'out_dir': os.path.join(args.data_root, out_dir),
                      'frames': {key: int(result['count'][:, 0].sum()) for key, result in results.items()},
                      'features': {key: int(result['count'].shape[1]) for key, result in results.items()}}))


if __name__ == '__main__':
    main()
