"""The normaliser and loader side of ``morgana.data`` in front of the HIP kernels.

Reference behaviour: morgana/data.py - ``normalise_mvn`` / ``denormalise_mvn`` :533-538, ``normalise_minmax`` /
``denormalise_minmax`` :579-590, the normaliser classes :252-386, :541-616 (here: one affine-map class driven by a table of
kinds, ``FeatureNormaliser``), ``collate_fn`` :159-224, ``FilesDataset`` :60-157, ``ToDeviceWrapper`` :648-663.

As in the reference, every function works on NumPy arrays (loader side, host arithmetic: data.py:119-127) and on
torch tensors (model side, README.rst:87); device tensors go through the fused HIP elementwise kernel.
"""
import json
import os

import numpy as np
import torch

from . import ops


class _NormFn(torch.autograd.Function):
    """out = kernel(x; p0, p1).  d out / d x is the per-column scale (1/(std+eps), std, 1/scale or scale)."""

    @staticmethod
    def forward(ctx, x, p0, p1, kind):
        ctx.kind = kind
        ctx.save_for_backward(p0, p1)
        return ops.normalise(x, p0, p1, kind)

    @staticmethod
    def backward(ctx, grad):
        p0, p1 = ctx.saved_tensors
        kind = ctx.kind
        if kind == ops.NORM_MVN:
            scale = 1.0 / (p1 + 1e-8)
        elif kind == ops.DENORM_MVN:
            scale = p1
        else:
            scale = p1 - p0
            scale = torch.where(scale.abs() <= 1e-8, torch.ones_like(scale), scale)
            if kind == ops.NORM_MINMAX:
                scale = 1.0 / scale
        return grad * scale, None, None, None


class _ItemNormFn(torch.autograd.Function):
    """out = kernel(x; row item_row[b] of the tables p0, p1).  d out / d x is the same per-column scale as ``_NormFn``'s, taken from
    the item's row: one launch of the per-item kernel in its gradient mode."""

    @staticmethod
    def forward(ctx, x, p0, p1, item_row, kind):
        ctx.kind = kind
        ctx.save_for_backward(p0, p1, item_row)
        return ops.normalise_items(x, p0, p1, item_row, kind)

    @staticmethod
    def backward(ctx, grad):
        p0, p1, item_row = ctx.saved_tensors
        return ops.normalise_items_backward(grad, p0, p1, item_row, ctx.kind), None, None, None, None


def _device_norm(feature, p0, p1, kind):
    if not feature.is_cuda:
        raise RuntimeError('morgana_amd normalisers take NumPy arrays (host, loader side) or device tensors; '
                           'got a CPU torch tensor (there is no CPU fallback for the device path)')
    p0 = p0.to(device=feature.device, dtype=torch.float32).reshape(-1)
    p1 = p1.to(device=feature.device, dtype=torch.float32).reshape(-1)
    return _NormFn.apply(feature, p0, p1, kind)


# One table describes every normalisation this package knows: a normaliser is an AFFINE map per feature column,
#     normalise(x) = (x - offset) / divisor        denormalise(y) = y * multiplier + offset,
# and a kind says how (offset, divisor, multiplier) follow from its two stored parameter vectors, which JSON file holds them and
# which op code of the device kernel (mg_normalise_f32) computes the same map.  Reference arithmetic: data.py:533-538 (mvn),
# :579-590 (minmax; a zero range divides by one).
def _minmax_range(mmin, mmax):
    span = mmax - mmin
    return np.where(np.abs(span) <= 1e-8, np.ones_like(span), span)


_KINDS = {
    'mvn': {'params': ('mean', 'std_dev'), 'file': '{name}_mvn.json', 'forward': ops.NORM_MVN, 'inverse': ops.DENORM_MVN,
            'affine': lambda mean, std_dev: (mean, std_dev + 1e-8, std_dev)},
    'minmax': {'params': ('mmin', 'mmax'), 'file': '{name}_minmax.json', 'forward': ops.NORM_MINMAX, 'inverse': ops.DENORM_MINMAX,
               'affine': lambda mmin, mmax: (mmin, _minmax_range(mmin, mmax), _minmax_range(mmin, mmax))},
}


def _apply_kind(kind, feature, p0, p1, inverse):
    """The map of ``kind`` (or its inverse) over the last axis of ``feature``: NumPy on the host (the loader side, data.py:119-127),
    the HIP elementwise kernel for device tensors (the model side, README.rst:87)."""
    spec = _KINDS[kind]
    if isinstance(feature, np.ndarray):
        offset, divisor, multiplier = spec['affine'](p0, p1)
        if inverse:
            return (feature * multiplier[..., None, :]) + offset[..., None, :]
        return (feature - offset[..., None, :]) / divisor[..., None, :]
    return _device_norm(feature, p0, p1, spec['inverse' if inverse else 'forward'])


def normalise_mvn(feature, mean, std_dev):
    return _apply_kind('mvn', feature, mean, std_dev, inverse=False)


def denormalise_mvn(feature, mean, std_dev):
    return _apply_kind('mvn', feature, mean, std_dev, inverse=True)


def normalise_minmax(feature, mmin, mmax):
    return _apply_kind('minmax', feature, mmin, mmax, inverse=False)


def denormalise_minmax(feature, mmin, mmax):
    return _apply_kind('minmax', feature, mmin, mmax, inverse=True)


class _ParamGroup(object):
    """The two parameter vectors of one normaliser (its statics, or its deltas): float32 NumPy arrays for the host path and the same
    values as torch tensors on ``device`` for the device path."""

    def __init__(self, kind, values, device='cpu'):
        names = _KINDS[kind]['params']
        missing = [n for n in names if n not in values]
        if missing:
            raise KeyError('normaliser parameters %s missing (have %s)' % (missing, sorted(values)))
        self.host = {n: np.asarray(values[n], dtype=np.float32) for n in values}
        self.torch = {n: torch.tensor(v).to(device) for n, v in self.host.items()}

    @classmethod
    def from_json(cls, kind, path, device='cpu'):
        with open(path, 'r') as f:
            return cls(kind, json.load(f), device=device)


def _write_params_json(path, host_params):
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'w') as f:
        json.dump({name: [float(v) for v in np.asarray(values).reshape(-1)] for name, values in host_params.items()}, f)


class FeatureNormaliser(object):
    """A named feature's normaliser: ``kind`` (a row of ``_KINDS``) + up to two parameter groups (the feature itself; its deltas when
    ``use_deltas``).  Public surface of the reference's normalisers (data.py:252-386): ``normalise`` / ``denormalise`` on NumPy arrays
    and tensors, ``fetch_params``, ``load_params`` from ``{name}_<kind>.json``, the ``params`` / ``params_torch`` / ``delta_params`` /
    ``delta_params_torch`` dictionaries; ``set_params`` installs values directly (synthetic runs have no JSON files)."""

    kind = None

    def __init__(self, name, use_deltas=False):
        if self.kind not in _KINDS:
            raise NotImplementedError('FeatureNormaliser is abstract: use MeanVarianceNormaliser or MinMaxNormaliser')
        self.name = name
        self.use_deltas = use_deltas
        self._groups = {}                                 # False -> the feature's parameters, True -> its deltas'

    # -- parameters ------------------------------------------------------------------------------------------------------------------
    def _view(self, deltas, side):
        group = self._groups.get(bool(deltas))
        return None if group is None else getattr(group, side)

    params = property(lambda self: self._view(False, 'host'))
    params_torch = property(lambda self: self._view(False, 'torch'))
    delta_params = property(lambda self: self._view(True, 'host'))
    delta_params_torch = property(lambda self: self._view(True, 'torch'))

    def fetch_params(self, data_type=np.ndarray, deltas=False):
        return self._view(deltas, 'torch' if data_type == torch.Tensor else 'host')

    def set_params(self, params, delta_params=None, device='cpu'):
        self._groups[False] = _ParamGroup(self.kind, params, device=device)
        if self.use_deltas and delta_params is not None:
            self._groups[True] = _ParamGroup(self.kind, delta_params, device=device)
        return self

    def load_params(self, data_dir, data_root='.', device='cpu'):
        pattern = _KINDS[self.kind]['file']
        for deltas in ((False, True) if self.use_deltas else (False,)):
            file_name = pattern.format(name=self.name + ('_deltas' if deltas else ''))
            self._groups[deltas] = _ParamGroup.from_json(self.kind, os.path.join(data_root, data_dir, file_name), device=device)

    def save_params(self, data_dir, data_root='.'):
        """The inverse of ``load_params``: ``{name}_<kind>.json`` (and ``{name}_deltas_<kind>.json``) under ``data_root/data_dir``, the
        same keys, plain lists of numbers.  A float32 written as its exact decimal value comes back bit for bit."""
        pattern = _KINDS[self.kind]['file']
        for deltas in ((False, True) if self.use_deltas else (False,)):
            group = self._groups.get(deltas)
            if group is None:
                raise RuntimeError('normaliser %r has no %sparameters to save: call set_params or fit_normalisers first' % (
                    self.name, 'delta ' if deltas else ''))
            file_name = pattern.format(name=self.name + ('_deltas' if deltas else ''))
            _write_params_json(os.path.join(data_root, data_dir, file_name), group.host)

    # -- the map ---------------------------------------------------------------------------------------------------------------------
    def _map(self, feature, deltas, inverse):
        values = self.fetch_params(type(feature), deltas=deltas)
        if values is None:
            raise RuntimeError('normaliser %r has no %sparameters: call load_params or set_params first' % (
                self.name, 'delta ' if deltas else ''))
        p0, p1 = (values[n] for n in _KINDS[self.kind]['params'])
        return _apply_kind(self.kind, feature, p0, p1, inverse)

    def normalise(self, feature, deltas=False):
        return self._map(feature, deltas, inverse=False)

    def denormalise(self, feature, deltas=False):
        return self._map(feature, deltas, inverse=True)


class MeanVarianceNormaliser(FeatureNormaliser):
    """Zero mean / unit variance; ``mean`` / ``std_dev`` from ``{name}_mvn.json`` (data.py:541-564)."""
    kind = 'mvn'


class MinMaxNormaliser(FeatureNormaliser):
    """Range [0, 1]; ``mmin`` / ``mmax`` from ``{name}_minmax.json`` (data.py:593-616)."""
    kind = 'minmax'


_FeatureNormaliser = FeatureNormaliser      # the reference's name for the base class

SPEAKER_ID_KEY, SPEAKER_INDEX_KEY = 'speaker_id', 'speaker_index'


def _read_id_list(path):
    with open(path, 'r') as f:
        return [line.strip() for line in f if line.strip()]


class _SpeakerDependentNormaliser(FeatureNormaliser):
    """One parameter group per speaker (data.py:388-530): ``{speaker_id}/{name}_<kind>.json`` for every name of ``speaker_id_list``;
    ``normalise`` / ``denormalise`` / ``fetch_params`` take the speakers of the batch items (a list of names, or one name), and
    ``params`` / ``params_torch`` / ``delta_params`` / ``delta_params_torch`` are keyed by speaker.  The arithmetic is the shared
    classes' (the ``_KINDS`` table); what differs is WHICH parameter row an item gets.

    Host side (NumPy features): the rows are gathered into (B, D) arrays and broadcast, as in the reference.  Device side: the
    parameters of all speakers live on the device once, stacked as (S, D) tables in ``speaker_ids`` order, and the per-item kernel
    (``ops.normalise_items``) picks row ``index[b]`` for item b.  ``speaker_ids`` may then also be that index itself - an integer tensor
    (B,) of rows of ``self.speaker_ids``, what the loaders put into ``features['speaker_index']``.  Names are resolved on the host and
    uploaded; inside a HIP graph capture that upload would be baked into the graph and go stale with the next batch, so names are
    refused there (RuntimeError -> ``GraphedStepCache`` runs such a step as ordinary launches): pass the index."""

    def __init__(self, name, speaker_id_list, use_deltas=False):
        super(_SpeakerDependentNormaliser, self).__init__(name, use_deltas=use_deltas)
        self.speaker_id_list = speaker_id_list
        self.speaker_ids = None
        self._tables = {}                                 # (deltas, device) -> (p0 table, p1 table), each (S, D) float32

    # -- parameters ------------------------------------------------------------------------------------------------------------------
    def _view(self, deltas, side):
        groups = self._groups.get(bool(deltas))
        if groups is None:
            return None if deltas else {}
        return {speaker: getattr(group, side) for speaker, group in groups.items()}

    def _install(self, deltas, groups):
        self._groups[bool(deltas)] = groups
        self._tables = {key: value for key, value in self._tables.items() if key[0] != bool(deltas)}

    def set_params(self, params, delta_params=None, device='cpu'):
        """``params`` (and ``delta_params``): {speaker: {parameter name: vector}}.  Sets ``speaker_ids`` to the keys' order unless it
        is set already."""
        if self.speaker_ids is None:
            self.speaker_ids = list(params)
        self._install(False, {spk: _ParamGroup(self.kind, params[spk], device=device) for spk in self.speaker_ids})
        if self.use_deltas and delta_params is not None:
            self._install(True, {spk: _ParamGroup(self.kind, delta_params[spk], device=device) for spk in self.speaker_ids})
        return self

    def load_params(self, data_dir, data_root='.', device='cpu'):
        if self.speaker_ids is None:
            self.speaker_ids = _read_id_list(os.path.join(data_root, self.speaker_id_list))
        pattern = _KINDS[self.kind]['file']
        for deltas in ((False, True) if self.use_deltas else (False,)):
            file_name = pattern.format(name=self.name + ('_deltas' if deltas else ''))
            self._install(deltas, {spk: _ParamGroup.from_json(self.kind, os.path.join(data_root, data_dir, spk, file_name), device=device)
                                   for spk in self.speaker_ids})

    def save_params(self, data_dir, data_root='.'):
        """The inverse of ``load_params``: ``{speaker_id}/{name}_<kind>.json`` (and its ``_deltas`` twin) for every speaker."""
        pattern = _KINDS[self.kind]['file']
        for deltas in ((False, True) if self.use_deltas else (False,)):
            groups = self._groups.get(deltas)
            if not groups:
                raise RuntimeError('normaliser %r has no %sparameters to save: call set_params or fit_normalisers first' % (
                    self.name, 'delta ' if deltas else ''))
            file_name = pattern.format(name=self.name + ('_deltas' if deltas else ''))
            for spk in self.speaker_ids:
                _write_params_json(os.path.join(data_root, data_dir, spk, file_name), groups[spk].host)

    def _names(self, speaker_ids):
        """Speaker names of the batch items from a name, a list of names or an integer index array / tensor (host side)."""
        if isinstance(speaker_ids, torch.Tensor):
            speaker_ids = speaker_ids.detach().cpu().numpy()
        if isinstance(speaker_ids, np.ndarray) and speaker_ids.dtype.kind in 'iu':
            return [self.speaker_ids[int(i)] for i in speaker_ids.reshape(-1)]
        if isinstance(speaker_ids, np.ndarray):
            speaker_ids = speaker_ids.reshape(-1).tolist()
        return list(speaker_ids) if isinstance(speaker_ids, (list, tuple)) else [speaker_ids]

    def fetch_params(self, speaker_ids, data_type=np.ndarray, deltas=False):
        """{parameter name: (B, D)} for the speakers of B batch items - (D,) when there is one (data.py:460-501); an unknown speaker is
        a KeyError."""
        per_speaker = self._view(deltas, 'torch' if data_type == torch.Tensor else 'host')
        if per_speaker is None:
            raise RuntimeError('normaliser %r has no delta parameters: call load_params or set_params first' % self.name)
        rows = [per_speaker[speaker] for speaker in self._names(speaker_ids)]
        stack = torch.stack if data_type == torch.Tensor else np.stack
        return {n: rows[0][n] if len(rows) == 1 else stack([row[n] for row in rows]) for n in rows[0]}

    # -- device side -----------------------------------------------------------------------------------------------------------------
    def tables(self, device, deltas=False):
        """The two (S, D) float32 parameter tables on ``device``, rows in ``speaker_ids`` order (built on first use, then kept)."""
        device = torch.device(device)
        key = (bool(deltas), str(device))
        if key not in self._tables:
            groups = self._groups.get(bool(deltas))
            if not groups:
                raise RuntimeError('normaliser %r has no %sparameters: call load_params or set_params first' % (
                    self.name, 'delta ' if deltas else ''))
            self._tables[key] = tuple(torch.from_numpy(np.stack([groups[spk].host[n] for spk in self.speaker_ids])).to(device)
                                      for n in _KINDS[self.kind]['params'])
        return self._tables[key]

    def speaker_rows(self, speaker_ids):
        """Rows of ``self.speaker_ids`` for a name or a list of names (host side; KeyError for an unknown speaker)."""
        lookup = {speaker: row for row, speaker in enumerate(self.speaker_ids or ())}
        return [lookup[speaker] for speaker in self._names(speaker_ids)]

    def speaker_index(self, speaker_ids, device):
        """The (B,) int32 row index on ``device`` the per-item kernels take: an integer tensor passes through, names are resolved on
        the host and uploaded - not while the current stream is being captured into a graph (see the class docstring)."""
        if isinstance(speaker_ids, torch.Tensor):
            if speaker_ids.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
                raise TypeError('speaker index must be an integer tensor, got %s' % speaker_ids.dtype)
            return speaker_ids.reshape(-1).to(device=device, dtype=torch.int32)
        device = torch.device(device)
        if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("normaliser %r: pass features['%s'], not speaker NAMES, while a HIP graph is being captured (an index "
                               "built from names here would be baked into the graph and go stale with the next batch)"
                               % (self.name, SPEAKER_INDEX_KEY))
        return torch.tensor(self.speaker_rows(speaker_ids), dtype=torch.int32).to(device)

    # -- the map ---------------------------------------------------------------------------------------------------------------------
    def _map(self, feature, speaker_ids, deltas, inverse):
        if isinstance(feature, np.ndarray):
            values = self.fetch_params(speaker_ids, np.ndarray, deltas=deltas)
            p0, p1 = (values[n] for n in _KINDS[self.kind]['params'])
            return _apply_kind(self.kind, feature, p0, p1, inverse)
        if not feature.is_cuda:
            raise RuntimeError('morgana_amd normalisers take NumPy arrays (host, loader side) or device tensors; '
                               'got a CPU torch tensor (there is no CPU fallback for the device path)')
        p0, p1 = self.tables(feature.device, deltas=deltas)
        index = self.speaker_index(speaker_ids, feature.device)
        single = feature.dim() == 2                       # one (T, D) sequence and one speaker
        batched = feature[None] if single else feature
        if index.numel() != batched.shape[0]:
            raise ValueError('%d speakers for a batch of %d items' % (index.numel(), batched.shape[0]))
        out = _ItemNormFn.apply(batched, p0, p1, index, _KINDS[self.kind]['inverse' if inverse else 'forward'])
        return out[0] if single else out

    def normalise(self, feature, speaker_ids, deltas=False):
        return self._map(feature, speaker_ids, deltas, inverse=False)

    def denormalise(self, feature, speaker_ids, deltas=False):
        return self._map(feature, speaker_ids, deltas, inverse=True)


class SpeakerDependentMeanVarianceNormaliser(_SpeakerDependentNormaliser):
    """Per-speaker zero mean / unit variance; ``{speaker_id}/{name}_mvn.json`` (data.py:567-576)."""
    kind = 'mvn'


class SpeakerDependentMinMaxNormaliser(_SpeakerDependentNormaliser):
    """Per-speaker range [0, 1]; ``{speaker_id}/{name}_minmax.json`` (data.py:619-628)."""
    kind = 'minmax'


def _speaker_order(normalisers):
    """The one ``speaker_ids`` order all speaker-dependent normalisers of ``normalisers`` share (None if there is none): the loaders
    write ONE ``speaker_index`` per batch, so the (S, D) tables of every normaliser must have their rows in the same order."""
    order = None
    for name, normaliser in (normalisers or {}).items():
        if not isinstance(normaliser, _SpeakerDependentNormaliser):
            continue
        if normaliser.speaker_ids is None:
            raise ValueError('speaker-dependent normaliser %r has no parameters: call load_params or set_params first' % name)
        if order is None:
            order = list(normaliser.speaker_ids)
        elif list(normaliser.speaker_ids) != order:
            raise ValueError('speaker-dependent normaliser %r lists its speakers in another order than the others of this dict: '
                             'one speaker_index per batch needs one order' % name)
    return order


def speaker_index_of(speaker_ids, order):
    """Positions of the names ``speaker_ids`` in ``order`` as an int32 array (KeyError for an unknown speaker)."""
    lookup = {speaker: row for row, speaker in enumerate(order)}
    return np.array([lookup[speaker] for speaker in speaker_ids], dtype=np.int32)


class Normalisers(dict):
    """name -> normaliser, every member's parameters loaded from ``data_root/normalisation_dir`` on construction (data.py:225-247)."""

    def __init__(self, normaliser_sources, normalisation_dir, data_root='.', device='cpu'):
        super(Normalisers, self).__init__(normaliser_sources)
        self.normalisation_dir = os.path.join(data_root, normalisation_dir)
        self.device = device
        for normaliser in self.values():
            normaliser.load_params(self.normalisation_dir, device=device)


FRAME_COUNT_KEY = 'n_frames'


def _host_total(value):
    """Sum of a host-side length vector as a python int, or None if the lengths are already on a device (reading them back would
    cost a synchronisation)."""
    if isinstance(value, np.ndarray):
        return int(value.sum())
    if isinstance(value, torch.Tensor) and not value.is_cuda:
        return int(value.sum().item())
    return None


BF16_TABLE_SUFFIX = '__bf16_table'
X3_TABLE_SUFFIX = '__x3_table'         # the [hi | lo] pair planes of precision 'bf16x3' (ops.split_pair); asked for as 'name:x3'


def add_bf16_table(features, key='normalised_lab', extra_rows=None):
    """Loader-side half of bf16 mode: ``features[key + '__bf16_table']`` = the (B*P + extra_rows, pad_ld(F)) bf16 copy of the phone-level
    feature ``features[key]`` (B, P, F) that the first Linear's loader reads (zero padded columns, ``extra_rows`` zero rows = what
    padding frames gather in the phone-rate step).  Made ONCE when the batch is loaded - it is data preparation, like the
    float32 cast of data.py:127 - instead of one cast kernel over the 49 MB table in every training step.  The fp32 feature stays
    in the dict (the reference's key, and the operand of fp32 mode); models fall back to casting it themselves when this entry is
    missing."""
    key, _, kind = key.partition(':')
    x = features[key]
    if extra_rows is None:
        extra_rows = ops.PHONE_RATE_EXTRA
    if kind == 'x3':
        # precision 'bf16x3': the table as a [hi | lo] pair of bf16 planes (x = hi + lo to 16 significant bits) - the operand of the
        # fused step's first layer and of its weight gradient (functional.F0StackX3Fn)
        features[key + X3_TABLE_SUFFIX] = ops.split_pair(x.reshape(-1, x.shape[-1]), extra_rows=extra_rows)
    else:
        features[key + BF16_TABLE_SUFFIX] = ops.cast_pad_bf16(x.reshape(-1, x.shape[-1]), extra_rows=extra_rows)
    return features


def to_device(features, device, bf16_tables=(), normalisers=None):
    """``ToDeviceWrapper.to_device`` over a feature dict (data.py:648-663); numpy arrays are uploaded too.

    ``normalisers``: when it holds speaker-dependent normalisers and the batch carries ``speaker_id`` (the list of names), the batch
    also gets ``speaker_index``: int32 (B,), the names' rows in the normalisers' ``speaker_ids``.

    ``bf16_tables``: names of phone-level features whose bf16 operand table the batch should carry (``add_bf16_table``; what a
    bf16-precision model's ``bf16_table_features()`` names) - the loader-side half of bf16 mode.

    One addition the reference's dict does not have: ``n_frames_total``, the python int sum of ``n_frames`` taken while the lengths
    are still on the host - it sizes the packed-frame layout of ragged batches (``utils.FrameLayout``) without a device -> host read.
    Models work without it (the build may carry a precomputed packed layout next to the reference's keys)."""
    out = {}
    for key, value in features.items():
        if isinstance(value, np.ndarray):
            value = torch.from_numpy(value)
        out[key] = value.to(device) if isinstance(value, torch.Tensor) else value
    total = _host_total(features.get(FRAME_COUNT_KEY))
    if total is not None and FRAME_COUNT_KEY + '_total' not in out:
        out[FRAME_COUNT_KEY + '_total'] = total
    for key in bf16_tables or ():
        name, _, kind = key.partition(':')
        if name in out and name + (X3_TABLE_SUFFIX if kind == 'x3' else BF16_TABLE_SUFFIX) not in out:
            add_bf16_table(out, key)
    order = _speaker_order(normalisers)
    if order is not None and SPEAKER_ID_KEY in out and SPEAKER_INDEX_KEY not in out:
        # next to the reference's list of names: their rows in the normalisers' tables, on the device (what a captured step reads)
        out[SPEAKER_INDEX_KEY] = torch.from_numpy(speaker_index_of(out[SPEAKER_ID_KEY], order)).to(device)
    return out


_TO_TORCH_DTYPE = {np.dtype('float16'): torch.float16, np.dtype('float32'): torch.float32,
                   np.dtype('float64'): torch.float64, np.dtype('int8'): torch.int8, np.dtype('int16'): torch.int16,
                   np.dtype('int32'): torch.int32, np.dtype('int64'): torch.int64, np.dtype('bool'): torch.bool,
                   np.dtype('uint8'): torch.uint8,
                   int: torch.int64, float: torch.float32, bool: torch.bool}


def collate_fn(batch):
    """List of per-utterance feature dicts -> batched dict (reference: ``FilesDataset.collate_fn``, data.py:159-224).

    Sequence features (ndarray, ndim > 1) are zero padded to ``(B, max_len, feat_dim)``; 1-d arrays and python scalars
    become ``(B, ...)`` tensors (ints -> int64); anything else (names) stays a list.
    """
    batch_size = len(batch)
    out = {}
    for key in batch[0].keys():
        items = [item[key] for item in batch]
        first = items[0]
        if isinstance(first, np.ndarray) and first.ndim > 1:
            max_len = max(len(x) for x in items)
            dtype = _TO_TORCH_DTYPE[first.dtype]
            # padded in NumPy (a slice assignment per utterance; a torch.tensor + indexed copy per utterance was 1 ms of a 256-utterance batch)
            batched = np.zeros((batch_size, max_len) + tuple(first.shape[1:]), dtype=first.dtype)
            for i, x in enumerate(items):
                batched[i, :x.shape[0]] = x
            out[key] = torch.from_numpy(batched).to(dtype)
        elif isinstance(first, np.ndarray) and first.dtype in _TO_TORCH_DTYPE:
            out[key] = torch.tensor(np.stack(items), dtype=_TO_TORCH_DTYPE[first.dtype])
        elif not isinstance(first, np.ndarray) and type(first) in _TO_TORCH_DTYPE:
            out[key] = torch.tensor(items, dtype=_TO_TORCH_DTYPE[type(first)])
        else:
            out[key] = items
    return out


def load_utterance(features, normalisers):
    """One utterance as ``FilesDataset.__getitem__`` yields it (data.py:106-154): every feature that has a normaliser also
    gets its ``normalised_`` twin, computed on the host in NumPy and cast to float32 (data.py:119-127)."""
    out = dict(features)
    for name, normaliser in normalisers.items():
        if name in features:
            who = (features[SPEAKER_ID_KEY],) if isinstance(normaliser, _SpeakerDependentNormaliser) else ()
            out['normalised_' + name] = normaliser.normalise(features[name], *who).astype(np.float32)
    return out


DELTAS_SUFFIX = '_deltas'


def _default_windows():
    from .viz import synthesis                            # (imported here: viz imports this package's ops on its own)
    return synthesis.DEFAULT_WINDOWS


class DeltaSpec(object):
    """How the delta features of one named feature are computed: ``windows`` - [(l, u, coefficients)], as ``viz.synthesis.MLPG`` takes
    them, default ``viz.synthesis.DEFAULT_WINDOWS`` (static, delta, delta-delta) - and ``edge``, see ``compute_deltas``."""

    def __init__(self, windows=None, edge='replicate'):
        if edge not in ops.DELTAS_EDGES:
            raise ValueError("edge must be 'replicate' or 'zero', got %r" % (edge,))
        windows = _default_windows() if windows is None else windows
        self.windows = tuple((int(l), int(u), tuple(float(c) for c in coeff)) for l, u, coeff in windows)
        for w, (l, u, coeff) in enumerate(self.windows):
            if l < 0 or u < 0 or len(coeff) != l + u + 1:
                raise ValueError('window %d: %d coefficients for extents l=%d, u=%d' % (w, len(coeff), l, u))
        self.edge = edge

    def __repr__(self):
        return 'DeltaSpec(windows=%r, edge=%r)' % (self.windows, self.edge)


def _host_deltas(feature, spec):
    """The arithmetic of mg_deltas_f32 in NumPy for one (len, D) item: per window the products coefficient * x in float64, taps in
    ascending order, the first product starting the sum, each later one added with one rounding; the sum rounded once to float32."""
    x = np.asarray(feature)
    if x.ndim != 2:
        raise ValueError('compute_deltas: a host feature must be one (frames, features) array, got shape %s' % (x.shape,))
    n, d = x.shape
    wide = x.astype(np.float32).astype(np.float64)
    out = np.zeros((n, len(spec.windows) * d), dtype=np.float32)
    if n == 0:
        return out
    frames = np.arange(n)
    for w, (l, u, coeff) in enumerate(spec.windows):
        acc, opened = np.zeros((n, d)), np.zeros(n, dtype=bool)
        for k, c in enumerate(coeff):
            taps = frames - l + k
            inside = (taps >= 0) & (taps < n)
            use = np.ones(n, dtype=bool) if spec.edge == 'replicate' else inside
            with np.errstate(all='ignore'):
                term = np.float64(c) * wide[np.clip(taps, 0, n - 1)]
                summed = np.where(opened[:, None], acc + term, term)
            acc = np.where(use[:, None], summed, acc)
            opened |= use
        with np.errstate(all='ignore'):
            out[:, w * d:(w + 1) * d] = acc.astype(np.float32)
    return out


def _not_an_array(what, x):
    """``x`` is no NumPy array: it must be a tensor ..."""
    if not isinstance(x, torch.Tensor):
        raise TypeError('%s takes a NumPy array or a device tensor, got %s' % (what, type(x)))


def _on_device(what, x):
    """... and, once its shape has been checked, on the device."""
    if not x.is_cuda:
        from ._lib import MorganaHipError
        raise MorganaHipError('%s takes NumPy arrays (host) or device tensors; got a tensor on %s (no CPU fallback for the '
                              'device path)' % (what, x.device))


def _device_lengths(lengths, device):
    return lengths.to(device=device, dtype=torch.int64).reshape(-1)


def _host_or_batched(what, x, seq_len, noun):
    """The argument of an operator with a host form and a device form -> (batched, seq_len, single).  A NumPy array is one whole item
    for the host form: (None, None, True).  A device tensor (frames, features) or (batch, frames, features) comes back as a batch with
    its int64 lengths on its device (every frame, without ``seq_len``); ``single``: the caller strips the batch dimension again."""
    if isinstance(x, np.ndarray):
        if seq_len is not None:
            raise ValueError('%s: seq_len goes with a batched device tensor; a host array is one whole item' % what)
        return None, None, True
    _not_an_array(what, x)
    if x.requires_grad:
        raise RuntimeError('%s has no backward: detach the %s first' % (what, noun))
    if x.dim() not in (2, 3):
        raise ValueError('%s: a tensor must be (frames, features) or (batch, frames, features), got %s' % (what, tuple(x.shape)))
    single = x.dim() == 2
    if single and seq_len is not None:
        raise ValueError('%s: seq_len goes with a batched (batch, frames, features) tensor' % what)
    _on_device(what, x)
    batched = x[None] if single else x
    if seq_len is None:
        seq_len = torch.full((batched.shape[0],), batched.shape[1], dtype=torch.int64, device=batched.device)
    else:
        seq_len = _device_lengths(seq_len, batched.device)
    return batched, seq_len, single


def compute_deltas(feature, windows=None, edge='replicate', seq_len=None):
    """Delta features ``[window 0 | window 1 | ...]`` of a feature: column ``w*D + d`` at frame t is ``sum_k coeff[w][k] x[t - l_w + k, d]``,
    row t of the window matrix ``W_w`` that MLPG inverts (morgana/viz/synthesis.py:8-36).  ``windows`` defaults to
    ``viz.synthesis.DEFAULT_WINDOWS``: the result is then ``[static | delta | delta-delta]``, the layout of the ``{name}_deltas`` files.

    A NumPy ``(len, D)`` array is computed on the host; a device tensor ``(B, T, D)`` - with ``seq_len`` (B,), frames past it are not
    read and come back as zeros - or ``(T, D)`` goes through the HIP kernel (csrc/deltas.hip).  Both accumulate every element in
    float64, taps in ascending order, and round once to float32: the same bits.  There is no backward: a tensor that requires grad is
    refused.

    ``edge``: what a tap outside the item reads.  'replicate' (default): the item's first / last frame, the Merlin convention;
    'zero': nothing, which is exactly ``W_w`` (MLPG of the result with unit variances gives the feature back).  Which of the two the
    ``{name}_deltas`` files of ``tts_data_tools`` were written with could not be verified - the package is not vendored with the
    reference - so it stays an argument."""
    spec = DeltaSpec(windows, edge)
    batched, seq_len, single = _host_or_batched('compute_deltas', feature, seq_len, 'feature')
    if batched is None:
        return _host_deltas(feature, spec)
    out, _ = ops.deltas(batched, spec.windows, seq_len=seq_len, edge=spec.edge, t=batched.shape[1])
    return out[0] if single else out


def _delta_specs_of(utterances, delta_specs):
    """The {feature name: DeltaSpec} a loader applies: the argument, or what the data sources of a ``FilesDataset`` ask for."""
    if delta_specs is None:
        return utterances.delta_specs() if isinstance(utterances, FilesDataset) else {}
    return dict(delta_specs)


VUV_KEY = 'vuv'


class F0Spec(object):
    """How the continuous log-F0 of one named feature is computed (``continuous_lf0``): ``source`` - the key of the raw F0 track in the
    utterances, ``vuv`` - the key the voicing flag is written under, and the operator's ``log_input`` / ``voiced_above`` / ``fill``."""

    def __init__(self, source='f0', vuv=VUV_KEY, log_input=False, voiced_above=None, fill=0.):
        if not source or not vuv:
            raise ValueError('F0Spec: source=%r and vuv=%r must be feature names' % (source, vuv))
        self.source, self.vuv, self.log_input = source, vuv, bool(log_input)
        self.voiced_above = ops.f0_voiced_above(voiced_above, self.log_input)
        self.fill = float(np.float32(fill))

    def __repr__(self):
        return 'F0Spec(source=%r, vuv=%r, log_input=%r, voiced_above=%r, fill=%r)' % (
            self.source, self.vuv, self.log_input, self.voiced_above, self.fill)


def _host_continuous_lf0(f0, spec):
    """The arithmetic of mg_continuous_lf0_f32 in NumPy for one (len, D) item: the comparison in float32, the logarithm and the three
    operations of the interpolation in float64, in the kernel's order, one rounding to float32."""
    x = np.asarray(f0)
    if x.ndim != 2:
        raise ValueError('continuous_lf0: a host track must be one (frames, features) array, got shape %s' % (x.shape,))
    x = x.astype(np.float32)
    n, d = x.shape
    with np.errstate(all='ignore'):
        voiced = x > np.float32(spec.voiced_above)            # False for a NaN
        wide = x.astype(np.float64)
        logs = wide if spec.log_input else np.log(np.where(voiced, wide, 1.0))
    lf0 = np.full((n, d), np.float32(spec.fill), dtype=np.float32)
    frames = np.arange(n)
    for c in range(d):
        at = np.flatnonzero(voiced[:, c])
        if at.size == 0:
            continue
        pos = np.searchsorted(at, frames)                     # voiced frames before t: at[pos - 1] < t <= at[pos]
        a, b = at[np.clip(pos - 1, 0, at.size - 1)], at[np.clip(pos, 0, at.size - 1)]
        la, lb = logs[a, c], logs[b, c]
        with np.errstate(all='ignore'):
            w = (frames - a).astype(np.float64) / np.where(b > a, b - a, 1).astype(np.float64)
            between = la + (lb - la) * w
        value = np.where(pos == 0, lb, np.where(pos == at.size, la, between))
        value = np.where(voiced[:, c], logs[:, c], value)
        with np.errstate(all='ignore'):
            lf0[:, c] = value.astype(np.float32)
    return lf0, voiced.astype(np.float32)


def continuous_lf0(f0, seq_len=None, log_input=False, voiced_above=None, fill=0.):
    """``(lf0, vuv)`` of a raw F0 track: the two features every F0 model of the reference reads and gets as files from
    ``tts_data_tools`` (models/f0_test_model.py, models/RNN_SPSS.py).  Per item and per column:

    * ``vuv[t] = 1.0`` where ``f0[t] > voiced_above`` (a NaN is unvoiced), else 0.0.  ``voiced_above`` defaults to 0.0 - extractors
      write 0 where unvoiced - and, with ``log_input``, to -1e9, so that the HTS / Merlin marker -1e10 reads as unvoiced.
    * ``lf0[t] = log(f0[t])`` on a voiced frame (``f0[t]`` itself with ``log_input``: the track is a log-F0 track already); on an
      unvoiced frame between the nearest voiced frames a < t < b it is ``l[a] + (l[b] - l[a]) * ((t - a) / (b - a))``; before the first
      voiced frame it holds that frame's value, behind the last one that one's; an item without a voiced frame is ``fill``.

    A NumPy ``(len, D)`` array is computed on the host; a device tensor ``(B, T, D)`` - with ``seq_len`` (B,), frames past it are not
    read and come back as zeros - or ``(T, D)`` goes through the HIP kernel (csrc/f0.hip).  Both take the logarithm and the
    interpolation in float64, in this order without contraction, and round once to float32; with ``log_input`` there is no
    transcendental and the two give the same bits, otherwise they differ by what the two ``log`` implementations differ.  A voiced
    value that is not finite (or whose logarithm is not) propagates by the formula.  There is no backward: a tensor that requires grad
    is refused.

    Holding the edge values is ``np.interp``'s convention.  Whether the ``lf0`` files of ``tts_data_tools`` were written that way could
    not be verified - the package is not vendored with the reference - so this is a stated choice, not a matched one."""
    spec = F0Spec(log_input=log_input, voiced_above=voiced_above, fill=fill)
    batched, seq_len, single = _host_or_batched('continuous_lf0', f0, seq_len, 'track')
    if batched is None:
        return _host_continuous_lf0(f0, spec)
    lf0, _, vuv, _ = ops.continuous_lf0(batched, seq_len=seq_len, t=batched.shape[1], log_input=spec.log_input,
                                        voiced_above=spec.voiced_above, fill=spec.fill)
    return (lf0[0], vuv[0]) if single else (lf0, vuv)


def _f0_specs_of(utterances, f0_specs):
    """The {feature name: F0Spec} a loader applies: the argument, or what the data sources of a ``FilesDataset`` ask for."""
    if f0_specs is None:
        return utterances.f0_specs() if isinstance(utterances, FilesDataset) else {}
    return dict(f0_specs)


def _check_f0_specs(f0_specs, first):
    """Refuse a first utterance that carries what ``f0_specs`` computes, or lacks what they read."""
    taken = set()
    for name, spec in f0_specs.items():
        for key in (name, spec.vuv):
            if key in first:
                raise ValueError('%r is in the utterances and in f0_specs: it is read from files or computed, not both' % key)
            if key in taken:
                raise ValueError('f0_specs write %r twice' % key)
            taken.add(key)
        if spec.source not in first:
            raise KeyError('f0_specs read %r for %r, which the utterances do not have' % (spec.source, name))
        track = first[spec.source]
        if not (isinstance(track, np.ndarray) and track.ndim == 2 and track.dtype == np.float32):
            raise TypeError('f0_specs read %r, which is not a float32 (frames, features) array' % spec.source)


class CountersSpec(object):
    """How the frame-level positional features of one named feature are computed (``frame_counters``): ``source`` - the key of the integer
    durations in the utterances, ``(P,)`` / ``(P, 1)`` phone durations or ``(P, S)`` state durations - and ``kind``, 'full' (9 columns) or
    'phone' (3 columns)."""

    def __init__(self, source='dur', kind='full'):
        if not source:
            raise ValueError('CountersSpec: source=%r must be a feature name' % (source,))
        if kind not in ops.COUNTERS_KINDS:
            raise ValueError("CountersSpec: kind must be 'full' or 'phone', got %r" % (kind,))
        self.source, self.kind = source, kind

    @property
    def columns(self):
        return ops.COUNTERS_KINDS[self.kind][1]

    def __repr__(self):
        return 'CountersSpec(source=%r, kind=%r)' % (self.source, self.kind)


def _host_durations(dur, what='frame_counters'):
    """Integer durations ``(P,)``, ``(P, 1)`` or ``(P, S)`` as a non-negative int64 ``(P, S)`` array."""
    d = np.asarray(dur)
    if not np.issubdtype(d.dtype, np.integer):
        raise TypeError('%s: durations must be integers, got %s' % (what, d.dtype))
    if d.ndim == 1:
        d = d.reshape(-1, 1)
    if d.ndim != 2 or d.shape[1] == 0:
        raise ValueError('%s: host durations must be (phones,), (phones, 1) or (phones, states), got shape %s' % (what, np.shape(dur)))
    if (d < 0).any():
        raise ValueError('%s: negative durations' % what)
    return d.astype(np.int64)


_HOST_COUNTERS_CHUNK = 1 << 18


def _host_frame_counters(dur, kind):
    """The arithmetic of mg_frame_counters_f32 in NumPy for one item: integers in int64, every quotient one float64 division rounded
    once to float32, integer columns converted directly."""
    if kind not in ops.COUNTERS_KINDS:
        raise ValueError("frame_counters: kind must be 'full' or 'phone', got %r" % (kind,))
    d = _host_durations(dur)
    n_phones, n_states = d.shape
    flat = d.ravel()
    ends = np.cumsum(flat)                                # of every segment, in (phone, state) order
    starts = ends - flat
    phone_starts, phone_lens = starts[::n_states], d.sum(axis=1)
    total = int(flat.sum())
    out = np.empty((total, ops.COUNTERS_KINDS[kind][1]), dtype=np.float32)

    def ratio(num, den):
        return (num.astype(np.float64) / den.astype(np.float64)).astype(np.float32)

    for lo in range(0, total, _HOST_COUNTERS_CHUNK):      # (in chunks of frames: the temporaries of a very long item stay small)
        frame = np.arange(lo, min(lo + _HOST_COUNTERS_CHUNK, total))
        segment = np.searchsorted(ends, frame, side='right')        # the first segment that ends behind the frame: empty ones are stepped over
        phone = segment // n_states
        n_p, j = phone_lens[phone], frame - phone_starts[phone]
        rows = out[frame[0]:frame[-1] + 1]
        if kind == 'phone':
            rows[:, 0], rows[:, 1], rows[:, 2] = ratio(j + 1, n_p), ratio(n_p - j, n_p), n_p
            continue
        n_s, i, state = flat[segment], frame - starts[segment], segment - phone * n_states
        rows[:, 0], rows[:, 1], rows[:, 2] = ratio(i + 1, n_s), ratio(n_s - i, n_s), n_s
        rows[:, 3], rows[:, 4], rows[:, 5] = state + 1, n_states - state, n_p
        rows[:, 6], rows[:, 7], rows[:, 8] = ratio(n_s, n_p), ratio(n_p - j, n_p), ratio(j + 1, n_p)
    return out


def frame_counters(dur, kind='full', seq_len=None, n_phones=None, max_len=None):
    """Frame-level positional features from durations: the ``counters`` feature the acoustic models of the reference read
    (models/RNN_SPSS.py:65) and get as files from ``tts_data_tools``.  ``dur[p, s]`` are integer durations in frames of P phones with S
    sub-phone states each (S = 1: a phone-level alignment, 5: HTS state alignments).  Segment (p, s) starts at ``start[p, s]``, the sum
    of all durations before it in (p, s) order; a zero-length segment or phone owns no frame.  For frame t of segment (p, s), with
    ``i = t - start[p, s]``, ``n_s = dur[p, s]``, ``j = t - start[p, 0]`` and ``n_p = sum_s dur[p, s]``:

    ``kind='full'``, 9 columns: ``(i+1)/n_s``, ``(n_s-i)/n_s``, ``n_s``, ``s+1``, ``S-s``, ``n_p``, ``n_s/n_p``, ``(n_p-j)/n_p``, ``(j+1)/n_p`` -
    fraction through the state forwards and backwards, state length, state index forwards and backwards, phone length, the state's
    share of the phone, fraction through the phone backwards and forwards.  This is Merlin's ``subphone_feats='full'``.
    ``kind='phone'``, 3 columns: ``(j+1)/n_p``, ``(n_p-j)/n_p``, ``n_p`` - Merlin's ``minimal_phoneme``; state boundaries play no part.

    Every quotient is taken in float64 from the two integers and rounded once to float32; integer columns are converted directly.  For
    phone lengths below 2^24 that is the correctly rounded float32 of the exact rational (double rounding through 53 bits is innocuous
    for a quotient of two 24-bit operands); above that no exactness claim is made.

    A NumPy integer array ``(P,)``, ``(P, 1)`` or ``(P, S)`` is computed on the host and gives ``(sum of durations, C)``; negative
    durations are refused there.  A device int64 tensor ``(B, P)`` or ``(B, P, S)`` goes through the HIP kernel (csrc/counters.hip), read
    in place through its strides, and gives ``(B, T, C)``: the same bits.  On the device a negative duration owns no frame (as in
    ``upsample_to_repetitions``), ``n_phones`` (B,) drops the phones from ``n_phones[b]`` on, and the frames of item b below
    ``min(T, its sum of durations, seq_len[b])`` hold counters, all others zeros.  ``max_len`` supplies T when the caller knows it (the
    padded target length); without it T is the largest sum of durations, at the cost of one device -> host read.  There is no backward.

    That 'full' is what the ``counters`` files of ``tts_data_tools`` hold - nine columns, in Merlin's order - could not be verified: the
    package is not vendored with the reference.  It is a stated choice, not a matched one."""
    if isinstance(dur, np.ndarray):
        if seq_len is not None or n_phones is not None or max_len is not None:
            raise ValueError('frame_counters: seq_len, n_phones and max_len go with a batched device tensor; a host array is one whole item')
        return _host_frame_counters(dur, kind)
    _not_an_array('frame_counters', dur)
    if dur.is_floating_point() or dur.dtype == torch.bool:
        raise TypeError('frame_counters: durations must be an integer tensor, got %s' % dur.dtype)
    if dur.dim() not in (2, 3):
        raise ValueError('frame_counters: a tensor must be (batch, phones) or (batch, phones, states), got %s' % (tuple(dur.shape),))
    _on_device('frame_counters', dur)
    dur = dur if dur.dtype == torch.int64 else dur.long()
    batch_size = dur.shape[0]
    if seq_len is not None:
        seq_len = _device_lengths(seq_len, dur.device)
    if n_phones is not None:
        n_phones = _device_lengths(n_phones, dur.device)
    if max_len is None:
        _, tmax = ops.upsample_lengths(dur.reshape(batch_size, -1))
        max_len = int(tmax.item())
    return ops.frame_counters(dur, t=int(max_len), kind=kind, seq_len=seq_len, n_phones=n_phones)[0]


def _duration_operands(normaliser, speaker_index, device=None):
    """(p0, p1, item_row) that take a normalised duration prediction back to frames: the mean and std_dev of a mean-variance
    normaliser - float32 vectors (host: ``device`` None; ``speaker_index`` then names the one speaker of a speaker-dependent
    normaliser), or on ``device`` vectors / the (speakers, S) tables with the batch's int32 row index.  Three Nones without one."""
    if normaliser is None:
        if speaker_index is not None:
            raise ValueError('quantise_durations: speaker_index goes with a speaker-dependent normaliser')
        return None, None, None
    if not isinstance(normaliser, FeatureNormaliser) or normaliser.kind != 'mvn':
        raise TypeError('quantise_durations: normaliser must be a MeanVarianceNormaliser or a SpeakerDependentMeanVarianceNormaliser, '
                        'got %r' % (normaliser,))
    dependent = isinstance(normaliser, _SpeakerDependentNormaliser)
    if dependent and speaker_index is None:
        raise KeyError("quantise_durations: the normaliser of %r is speaker-dependent: it needs speaker_index (features['%s'])"
                       % (normaliser.name, SPEAKER_INDEX_KEY))
    if not dependent and speaker_index is not None:
        raise ValueError('quantise_durations: speaker_index goes with a speaker-dependent normaliser')
    if device is None:
        prm = normaliser.fetch_params(speaker_index, np.ndarray) if dependent else normaliser.fetch_params(np.ndarray)
        if not prm:
            raise RuntimeError('normaliser %r has no parameters: call load_params, set_params or fit_normalisers first' % normaliser.name)
        mean, std_dev = (np.asarray(prm[n], dtype=np.float32) for n in _KINDS['mvn']['params'])
        if mean.ndim != 1:
            raise ValueError('quantise_durations: a host array is one item of one speaker, got %r' % (speaker_index,))
        return mean, std_dev, None
    if dependent:
        p0, p1 = normaliser.tables(device)
        return p0, p1, normaliser.speaker_index(speaker_index, device)
    prm = normaliser.fetch_params(torch.Tensor)
    if prm is None:
        raise RuntimeError('normaliser %r has no parameters: call load_params, set_params or fit_normalisers first' % normaliser.name)
    p0, p1 = (prm[n].to(device=device, dtype=torch.float32).reshape(-1) for n in _KINDS['mvn']['params'])
    return p0, p1, None


def _host_quantise_durations(pred, p0, p1, log_input, scale, lo, hi, carry, total):
    """The arithmetic of mg_quantise_durations_f32 in NumPy for one item (P, S): one float64 rounding per step up to the 16-bit
    fixed-point value, int64 from there on, the carry rule in its closed form -> (dur (P, S), phone_dur (P,), n_frames, flags)."""
    n_states = pred.shape[1]
    flags = 0
    with np.errstate(all='ignore'):
        x = pred.astype(np.float64)
        if p0 is not None:
            x = x * p1.astype(np.float64)[None, :] + p0.astype(np.float64)[None, :]
        if log_input:
            x = np.exp(x)
        x = (x * np.float64(scale)).ravel()
        bad = ~(x >= 0.) | np.isinf(x)
        if bad.any():
            flags |= ops.DUR_FLAG_INVALID
        x = np.minimum(np.where(bad, 0., x), np.float64(hi))
        q = np.floor(x * 65536. + .5).astype(np.int64)
        if total is not None:
            whole = int(q.sum())
            if whole > 0 and total > 0:
                ratio = np.float64(float(total << 16)) / np.float64(whole)
                q = np.minimum(np.floor(q.astype(np.float64) * ratio + .5), np.float64(hi << 16)).astype(np.int64)
            else:
                flags |= ops.DUR_FLAG_NO_FIT
    if carry:
        rounded = (np.cumsum(q) + 32768) >> 16
        floor = np.arange(1, q.size + 1, dtype=np.int64) * lo
        ends = floor + np.maximum(np.maximum.accumulate(rounded - floor), 0) if q.size else floor
        dur = np.diff(ends, prepend=np.int64(0))
        if q.size and int(ends[-1]) != (int(q.sum()) + 32768) >> 16:
            flags |= ops.DUR_FLAG_PUSHED
    else:
        dur = np.maximum((q + 32768) >> 16, lo)
    dur = dur.astype(np.int64).reshape(-1, n_states)
    return dur, dur.sum(axis=1), int(dur.sum()), flags


def quantise_durations(pred, n_phones=None, normaliser=None, speaker_index=None, log_input=False, scale=1., min_frames=1, max_frames=None,
                       rounding='carry', total=None):
    """Integer durations in frames from a duration model's real-valued prediction - what ``upsample_to_repetitions``,
    ``frame_counters`` and the acoustic models take as ``dur``.  ``pred[p, s]``: P phones of S sub-phone states, in the normalised space
    of ``normaliser`` (a ``MeanVarianceNormaliser`` or, with ``speaker_index``, a ``SpeakerDependentMeanVarianceNormaliser``: the value in
    frames is ``pred * std_dev + mean`` in float64), in frames without one.  ``log_input``: that value is a log-duration; ``scale``: a
    speaking-rate factor on the durations.  A NaN, infinite or negative value counts as 0 (flag ``ops.DUR_FLAG_INVALID``), a value above
    ``max_frames`` (default and largest: 2^20) as ``max_frames``.  Every value is then rounded to 16 fractional bits
    (``floor(x * 65536 + 0.5)``), and the rest is integer arithmetic over the segments in (p, s) order:

    ``rounding='nearest'``: ``max(min_frames, round(x))`` for every segment on its own, Merlin's rule.  The boundaries drift from the
    predicted ones like a random walk and the utterance length is whatever the errors add up to.
    ``rounding='carry'`` (default): the rounding error is carried along.  Segment i ends at ``max(the rounded predicted end, the previous
    end + min_frames)``: where every value is at least ``min_frames`` every boundary lies within half a frame of the predicted one and
    the length is the rounded predicted length; ``ops.DUR_FLAG_PUSHED`` says that the minimum pushed the length out.

    ``total``: the length to fit the item to, for example its natural ``n_frames``: the values are scaled by ``total / their sum``
    before the rounding, so that (with 'carry', where no scaled value lies below ``min_frames``) the durations add up to ``total``
    exactly.  ``ops.DUR_FLAG_NO_FIT`` and no scaling where ``total <= 0`` or the values add up to 0.

    A NumPy float array ``(P,)`` or ``(P, S)`` is one item computed on the host (``total`` an int, ``speaker_index`` the speaker's name)
    and gives ``(dur shaped like pred, phone_dur (P,), n_frames, flags)`` with the last two python ints.  A device float32 tensor
    ``(B, P)`` or ``(B, P, S)`` goes through the HIP kernel (csrc/durations.hip), read in place through its strides, with ``n_phones``
    (B,) dropping the phones from ``n_phones[b]`` on (never read, durations 0), ``total`` (B,) int64 and ``speaker_index`` (B,) the
    batch's ``features['speaker_index']``; it gives ``(dur int64 shaped like pred, phone_dur int64 (B, P), n_frames int64 (B,),
    flags int32 (B,))``: the same bits, except that ``exp`` of a ``log_input`` may differ in its last place between the host's and the
    device's library, which matters only for a value within 2^-49 (relative) of a rounding boundary.  There is no backward."""
    scale, lo, hi, code = ops.duration_arguments('quantise_durations', scale, min_frames, max_frames, rounding)
    if isinstance(pred, np.ndarray):
        if n_phones is not None:
            raise ValueError('quantise_durations: n_phones goes with a batched device tensor; a host array is one whole item')
        if not np.issubdtype(pred.dtype, np.floating):
            raise TypeError('quantise_durations: the prediction must be a float array, got %s' % pred.dtype)
        if pred.ndim not in (1, 2) or (pred.ndim == 2 and pred.shape[1] == 0):
            raise ValueError('quantise_durations: a host array must be (phones,) or (phones, states), got shape %s' % (pred.shape,))
        if total is not None:
            if isinstance(total, bool) or not isinstance(total, (int, np.integer)):
                raise TypeError('quantise_durations: total of a host array must be an int, got %r' % (total,))
            total = int(total)
        p0, p1, _ = _duration_operands(normaliser, speaker_index)
        item = pred.astype(np.float32).reshape(pred.shape[0], -1)
        if p0 is not None and (p0.size != item.shape[1] or p1.size != item.shape[1]):
            raise ValueError('quantise_durations: the normaliser has %d / %d parameters, the prediction %d states per phone'
                             % (p0.size, p1.size, item.shape[1]))
        dur, phone_dur, n_frames, flags = _host_quantise_durations(item, p0, p1, bool(log_input), scale, lo, hi, code == ops.DUR_ROUNDINGS['carry'],
                                                                    total)
        return dur.reshape(pred.shape), phone_dur, n_frames, flags
    _not_an_array('quantise_durations', pred)
    if pred.requires_grad:
        raise RuntimeError('quantise_durations has no backward: detach the prediction first')
    if pred.dim() not in (2, 3):
        raise ValueError('quantise_durations: a tensor must be (batch, phones) or (batch, phones, states), got %s' % (tuple(pred.shape),))
    _on_device('quantise_durations', pred)
    pred = pred if pred.dtype == torch.float32 else pred.float()
    if n_phones is not None:
        n_phones = _device_lengths(n_phones, pred.device)
    if total is not None:
        if not isinstance(total, torch.Tensor):
            raise TypeError('quantise_durations: total of a device batch must be a (batch,) tensor, got %s' % type(total))
        total = _device_lengths(total, pred.device)
    p0, p1, item_row = _duration_operands(normaliser, speaker_index, pred.device)
    return ops.quantise_durations(pred, n_phones=n_phones, p0=p0, p1=p1, item_row=item_row, log_input=log_input, scale=scale, lo=lo, hi=hi,
                                  rounding=rounding, total=total)


def _counter_specs_of(utterances, counter_specs):
    """The {feature name: CountersSpec} a loader applies: the argument, or what the data sources of a ``FilesDataset`` ask for."""
    if counter_specs is None:
        return utterances.counter_specs() if isinstance(utterances, FilesDataset) else {}
    return dict(counter_specs)


def _check_counter_specs(counter_specs, first):
    """Refuse a first utterance that carries what ``counter_specs`` computes, or lacks the durations they read."""
    for name, spec in counter_specs.items():
        if name in first:
            raise ValueError('%r is in the utterances and in counter_specs: it is read from files or computed, not both' % name)
        if spec.source not in first:
            raise KeyError('counter_specs read %r for %r, which the utterances do not have' % (spec.source, name))
        dur = first[spec.source]
        if not (isinstance(dur, np.ndarray) and dur.ndim in (1, 2) and np.issubdtype(dur.dtype, np.integer)):
            raise TypeError('counter_specs read %r, which is not an integer (phones,), (phones, 1) or (phones, states) array' % spec.source)


def _host_frame_total(dur):
    """Frames the durations of one utterance add up to, a negative duration owning none (what the kernel counts)."""
    return int(np.clip(np.asarray(dur), 0, None).sum())


class _Staging(object):
    """Pinned host staging for the loader's packed features: per (device, feature) TWO buffers used in turn - the copy of the batch
    before last has certainly been issued when a buffer comes round again, and its event says when it has finished - grown
    geometrically, never returned.  (``tensor.pin_memory()`` per batch allocates and page-locks 49 MB every time: with the fresh
    ``np.concatenate`` result in front of it, 80 ms of a C2 batch's 82.)"""

    def __init__(self):
        self._slots = {}
        self._turn = {}

    def take(self, device, key, n_bytes):
        turn = self._turn.get((device, key), 0)
        self._turn[(device, key)] = 1 - turn
        slot = self._slots.get((device, key, turn))
        if slot is not None and slot[1] is not None:
            slot[1].synchronize()                         # the H2D copy that last read this buffer
        if slot is None or slot[0].numel() < n_bytes:
            size = max(int(n_bytes * 1.25), 1 << 16)
            slot = [torch.empty(size, dtype=torch.uint8).pin_memory(), None]
            self._slots[(device, key, turn)] = slot
        return slot

    def clear(self):
        self._slots.clear()
        self._turn.clear()


_STAGING = _Staging()
HOST_PACK_THREADS = max(1, min(8, (os.cpu_count() or 2) // 2))


def _pack_pinned(items, device, key, dtype=np.float32):
    """``np.concatenate(items)`` of 2-D float32 arrays (``dtype``: of another element type - mg_host_pack copies bytes) into a pinned
    staging buffer (mg_host_pack: threaded memcpy), its asynchronous copy to ``device`` and the row offsets (int64, ``len(items) + 1``)
    beside it.  Returns (packed device tensor, offsets device tensor, host lengths)."""
    import ctypes
    from . import _lib
    width = items[0].shape[1]
    lens = np.array([x.shape[0] for x in items], dtype=np.int64)
    total = int(lens.sum())
    n_off = len(items) + 1
    off_bytes = (n_off * 8 + 63) // 64 * 64
    dtype = np.dtype(dtype)
    if dtype not in (np.float32, np.float64):
        raise TypeError('_pack_pinned packs float32 or float64 rows, got %s' % dtype)
    n_bytes = off_bytes + total * width * dtype.itemsize
    slot = _STAGING.take(str(device), key, n_bytes)
    host = slot[0]
    offsets_host = host[:n_off * 8].view(torch.int64)
    offsets_host[0] = 0
    offsets_host[1:] = torch.from_numpy(np.cumsum(lens))
    arrays = [x if (x.flags['C_CONTIGUOUS'] and x.dtype == dtype) else np.ascontiguousarray(x, dtype=dtype) for x in items]
    srcs = (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
    sizes = (ctypes.c_int64 * len(arrays))(*[a.nbytes for a in arrays])
    lib = _lib.load()
    _lib.check(lib.mg_host_pack(ctypes.cast(srcs, ctypes.c_void_p), ctypes.cast(sizes, ctypes.c_void_p), len(arrays),
                                ctypes.c_void_p(host.data_ptr() + off_bytes), ctypes.c_int64(host.numel() - off_bytes), HOST_PACK_THREADS),
               'mg_host_pack')
    staged = host[:n_bytes].to(device, non_blocking=True)                       # ONE copy across PCIe: offsets + rows
    slot[1] = torch.cuda.Event()
    slot[1].record(torch.cuda.current_stream(device))
    offsets = staged[:n_off * 8].view(torch.int64)
    packed = staged[off_bytes:].view(torch.float64 if dtype == np.float64 else torch.float32).view(total, width)
    return packed, offsets, lens


def _small_to_device(plain, device):
    """The batch's small host tensors (durations, lengths, ...) to ``device`` as ONE asynchronous copy out of pinned staging.  A
    ``tensor.to(device)`` from pageable memory is a synchronous copy on the current stream: it returns when everything queued there
    has run - the 49 MB feature copy in front of it included - so the host could not pack the next batch beside this one's transfer."""
    device = torch.device(device)
    tensors = [(k, v.contiguous()) for k, v in plain.items() if isinstance(v, torch.Tensor)]
    out = {k: v for k, v in plain.items() if not isinstance(v, torch.Tensor)}
    if device.type != 'cuda' or not tensors:
        out.update((k, v.to(device)) for k, v in tensors)
        return out
    spans, at = [], 0
    for _, v in tensors:
        spans.append(at)
        at += (v.numel() * v.element_size() + 63) // 64 * 64
    slot = _STAGING.take(str(device), '__small__', max(at, 64))
    host = slot[0]
    import ctypes
    for (_, v), lo in zip(tensors, spans):
        n = v.numel() * v.element_size()
        if n:
            # (memmove, not tensor.copy_: above 32 K elements a torch CPU op opens an OpenMP region on every core of the host, whose
            # workers then spin - on a box with a CPU quota that throttles the whole process for the rest of the scheduler period:
            # 90 ms stalls at random points of the loop, profiles/r5_notes_loader.txt)
            ctypes.memmove(host.data_ptr() + lo, v.data_ptr(), n)
    staged = host[:max(at, 64)].to(device, non_blocking=True)
    slot[1] = torch.cuda.Event()
    slot[1].record(torch.cuda.current_stream(device))
    for (k, v), lo in zip(tensors, spans):
        n = v.numel() * v.element_size()
        out[k] = staged[lo:lo + n].view(v.dtype).view(v.shape) if n else torch.empty(v.shape, dtype=v.dtype, device=device)
    return out


def _normaliser_operands(out, key, normaliser, device, deltas=False):
    """(kind, p0, p1, item_row) of the device passes that write a normalised twin: vectors for a plain normaliser, the (S, D) tables and
    the batch's ``speaker_index`` for a speaker-dependent one; four Nones without a normaliser."""
    if not isinstance(normaliser, FeatureNormaliser):
        return None, None, None, None
    spec = _KINDS[normaliser.kind]
    if isinstance(normaliser, _SpeakerDependentNormaliser):
        p0, p1 = normaliser.tables(device, deltas=deltas)
        return spec['forward'], p0, p1, out[SPEAKER_INDEX_KEY]
    prm = normaliser.fetch_params(torch.Tensor, deltas=deltas)
    if prm is None:
        raise RuntimeError('normaliser %r has no %sparameters: call load_params, set_params or fit_normalisers first' % (
            key, 'delta ' if deltas else ''))
    p0, p1 = (prm[n].to(device) for n in spec['params'])
    return spec['forward'], p0, p1, None


def _device_deltas(out, key, packed, offsets, t, spec, normaliser, device):
    """``out[key + '_deltas']`` (and its ``normalised_`` twin when ``normaliser`` normalises deltas) from the packed statics of ``key``
    that are on the device already: one mg_deltas_f32 launch, nothing more crosses PCIe."""
    kind = p0 = p1 = item_row = None
    if normaliser is not None and normaliser.use_deltas:
        kind, p0, p1, item_row = _normaliser_operands(out, key, normaliser, device, deltas=True)
    raw, norm = ops.deltas(packed, spec.windows, offsets=offsets, edge=spec.edge, t=t, p0=p0, p1=p1, kind=kind, item_row=item_row)
    out[key + DELTAS_SUFFIX] = raw
    if norm is not None:
        out['normalised_' + key + DELTAS_SUFFIX] = norm


def _device_f0(out, name, spec, packed, offsets, t, normaliser, delta_spec, device):
    """``out[name]``, ``out['normalised_' + name]`` (where ``normaliser`` is one) and ``out[spec.vuv]`` from the packed raw F0 track that
    is on the device: one mg_continuous_lf0_f32 launch, which also leaves the packed continuous track when deltas follow
    (``_device_deltas`` on that track: one more launch).  The raw track itself is not emitted."""
    kind, p0, p1, item_row = _normaliser_operands(out, name, normaliser, device)
    lf0, norm, vuv, track = ops.continuous_lf0(packed, offsets=offsets, t=t, want_packed=delta_spec is not None, log_input=spec.log_input,
                                               voiced_above=spec.voiced_above, fill=spec.fill, p0=p0, p1=p1, kind=kind, item_row=item_row)
    out[name], out[spec.vuv] = lf0, vuv
    if norm is not None:
        out['normalised_' + name] = norm
    if delta_spec is not None:
        _device_deltas(out, name, track, offsets, t, delta_spec, normaliser, device)


def _device_counters(out, name, spec, batch, normaliser, device):
    """``out[name]`` and - where ``normaliser`` is one - ``out['normalised_' + name]`` from the durations ``out[spec.source]`` that are on
    the device already: one mg_frame_counters_f32 launch, nothing more crosses PCIe.  With ``n_frames`` in the utterances the output is
    as long as every other frame-level feature of the batch and cut to each utterance's ``n_frames``; otherwise it is as long as the
    largest sum of durations (taken on the host)."""
    dur = out[spec.source]
    dur = dur if dur.dtype == torch.int64 else dur.long()
    if FRAME_COUNT_KEY in batch[0]:
        t, seq_len = max(int(item[FRAME_COUNT_KEY]) for item in batch), out[FRAME_COUNT_KEY].reshape(-1)
        seq_len = seq_len if seq_len.dtype == torch.int64 else seq_len.long()
    else:
        t, seq_len = max(_host_frame_total(item[spec.source]) for item in batch), None
    kind, p0, p1, item_row = _normaliser_operands(out, name, normaliser, device)
    raw, norm = ops.frame_counters(dur, t=t, kind=spec.kind, seq_len=seq_len, p0=p0, p1=p1, norm_kind=kind, item_row=item_row)
    out[name] = raw
    if norm is not None:
        out['normalised_' + name] = norm


def collate_to_device(batch, normalisers, device, bf16_tables=(), delta_specs=None, f0_specs=None, counter_specs=None):
    """``load_utterance`` + ``collate_fn`` + ``to_device`` for a list of RAW per-utterance feature dicts, with the float
    sequence features normalised and zero padded on the device (reference: data.py:119-127, 159-224, 648-663).

    Every float32 sequence feature travels as ONE packed host buffer (utterances back to back, pinned when possible) and one
    kernel pass (mg_pad_normalise_f32) writes the padded raw feature and - where ``normalisers`` has its name - the
    ``normalised_`` twin; the host never touches per-frame data beyond the concatenation.  Other features (integer
    durations, scalars, names) take the ordinary collate path.  Same values as the reference's host pipeline to fp32
    rounding of the normaliser arithmetic (the host version divides in float32 NumPy as well).

    ``bf16_tables``: names of normalised phone-level features (``'normalised_lab'``) whose bf16 operand table the SAME pass writes
    (``mg_pad_normalise_bf16_f32``): the batch then carries ``name + '__bf16_table'`` and a bf16-precision model's training step
    launches no cast of the phone table (reference: the float32 cast on load, data.py:127).

    ``delta_specs``: {feature name: ``DeltaSpec``}.  The packed statics uploaded for such a feature also give ``name_deltas`` and -
    where its normaliser has ``use_deltas`` - ``normalised_name_deltas``, computed on the device by one more launch
    (mg_deltas_f32, csrc/deltas.hip): no ``{name}_deltas`` file is read and nothing is uploaded twice.  A batch that already
    carries ``name_deltas`` is refused (ValueError): it is one or the other.

    ``f0_specs``: {feature name: ``F0Spec``}.  The raw F0 track ``spec.source`` is uploaded once and one launch (mg_continuous_lf0_f32,
    csrc/f0.hip) writes ``name`` - the continuous log-F0 - ``normalised_name`` where ``name`` has a normaliser, and ``spec.vuv``; when
    ``delta_specs`` names the feature too, the same launch leaves the packed continuous track and the delta launch reads that.  The raw
    track is not emitted.  A batch that already carries ``name`` or ``spec.vuv`` is refused (ValueError): each is read or computed.

    ``counter_specs``: {feature name: ``CountersSpec``}.  Once the integer features are on the device one launch (mg_frame_counters_f32,
    csrc/counters.hip) writes ``name`` - the frame-level positional features of the durations ``spec.source`` - and ``normalised_name``
    where ``name`` has a normaliser (plain or speaker dependent): no ``{name}`` file is read and nothing more is uploaded.  The output is
    as long as the batch's largest ``n_frames`` and cut to each utterance's ``n_frames`` when the utterances carry it, so that it agrees
    with every other frame-level feature; otherwise as long as the largest sum of durations.  A batch that already carries ``name`` is
    refused (ValueError): a feature is read or computed, not both; durations that are missing are a KeyError."""
    device = torch.device(device)
    bf16_tables = tuple(bf16_tables or ())
    delta_specs = dict(delta_specs or {})
    f0_specs = dict(f0_specs or {})
    counter_specs = dict(counter_specs or {})
    _check_f0_specs(f0_specs, batch[0])
    _check_counter_specs(counter_specs, batch[0])
    f0_sources = {}                                       # raw track -> the features computed from it
    for name, spec in f0_specs.items():
        f0_sources.setdefault(spec.source, []).append(name)
    for name in delta_specs:
        if name + DELTAS_SUFFIX in batch[0]:
            raise ValueError('%r is in the utterances and in delta_specs: deltas are read from files or computed, not both' % (
                name + DELTAS_SUFFIX))
        if name not in batch[0] and name not in f0_specs:
            raise KeyError('delta_specs names %r, which the utterances do not have' % name)
    out, rest = {}, []
    order = _speaker_order(normalisers)
    if order is not None:
        if SPEAKER_ID_KEY not in batch[0]:
            raise KeyError("speaker-dependent normalisers need a '%s' entry in every utterance" % SPEAKER_ID_KEY)
        # uploaded first (pinned staging, asynchronous): the per-item passes below read it
        speaker_index = torch.from_numpy(speaker_index_of([item[SPEAKER_ID_KEY] for item in batch], order))
        out[SPEAKER_INDEX_KEY] = _small_to_device({SPEAKER_INDEX_KEY: speaker_index}, device)[SPEAKER_INDEX_KEY]
    for key in batch[0].keys():
        first = batch[0][key]
        if not (isinstance(first, np.ndarray) and first.ndim == 2 and first.dtype == np.float32):
            rest.append(key)
            continue
        items = [item[key] for item in batch]
        if device.type == 'cuda':
            # pinned staging kept from batch to batch, packed by host threads, one H2D copy for rows and offsets
            packed, offsets, lens = _pack_pinned(items, device, key)
        else:
            lens = np.array([x.shape[0] for x in items], dtype=np.int64)
            offsets = torch.from_numpy(np.concatenate(([0], np.cumsum(lens))).astype(np.int64))
            packed = torch.from_numpy(np.ascontiguousarray(np.concatenate(items, axis=0)))
        if key in f0_sources:
            for name in f0_sources[key]:
                _device_f0(out, name, f0_specs[name], packed, offsets, int(lens.max()),
                           normalisers.get(name) if normalisers is not None else None, delta_specs.get(name), device)
            continue
        kind = p0 = p1 = None
        normaliser = normalisers.get(key) if normalisers is not None else None
        if isinstance(normaliser, _SpeakerDependentNormaliser):
            # the per-item pass: row speaker_index[b] of the (S, D) tables for utterance b.  (A bf16 table of such a feature is
            # made by the add_bf16_table pass at the end.)
            p0, p1 = normaliser.tables(device)
            out[key], out['normalised_' + key] = ops.pad_normalise_items(packed, offsets, int(lens.max()), p0, p1, out[SPEAKER_INDEX_KEY],
                                                                         _KINDS[normaliser.kind]['forward'])
            if key in delta_specs:
                _device_deltas(out, key, packed, offsets, int(lens.max()), delta_specs[key], normaliser, device)
            continue
        if isinstance(normaliser, FeatureNormaliser):
            spec, prm = _KINDS[normaliser.kind], normaliser.fetch_params(torch.Tensor)
            kind, (p0, p1) = spec['forward'], (prm[n].to(device) for n in spec['params'])
        if kind is not None and 'normalised_' + key in bf16_tables:
            raw, norm, table = ops.pad_normalise(packed, offsets, int(lens.max()), p0, p1, kind, bf16_extra_rows=ops.PHONE_RATE_EXTRA)
            out['normalised_' + key + BF16_TABLE_SUFFIX] = table
        else:
            raw, norm = ops.pad_normalise(packed, offsets, int(lens.max()), p0, p1, kind)
        out[key] = raw
        if norm is not None:
            out['normalised_' + key] = norm
        if key in delta_specs:
            _device_deltas(out, key, packed, offsets, int(lens.max()), delta_specs[key], normaliser, device)
    for name in delta_specs:
        if name + DELTAS_SUFFIX not in out:
            raise TypeError('delta_specs names %r, which is not a float32 (frames, features) array: its deltas are computed by the '
                            'device pass of such features' % name)
    if rest:
        plain = collate_fn([{key: item[key] for key in rest} for item in batch])
        total = _host_total(plain.get(FRAME_COUNT_KEY))
        if total is not None:
            out[FRAME_COUNT_KEY + '_total'] = total          # see to_device
        for key in rest:                                  # integer sequence features with a normaliser (dur) stay on the host path
            normaliser = normalisers.get(key) if normalisers is not None else None
            if normaliser is not None and isinstance(batch[0][key], np.ndarray):
                sd = isinstance(normaliser, _SpeakerDependentNormaliser)
                plain['normalised_' + key] = collate_fn([{key: normaliser.normalise(
                    item[key], *((item[SPEAKER_ID_KEY],) if sd else ())).astype(np.float32)} for item in batch])[key]
        out.update(_small_to_device(plain, device))
    for name, spec in counter_specs.items():
        _device_counters(out, name, spec, batch, normalisers.get(name) if normalisers is not None else None, device)
    for key in bf16_tables:                               # features that did not take the fused pass (no normaliser, host path; pair planes)
        name, _, kind = key.partition(':')
        suffix = X3_TABLE_SUFFIX if kind == 'x3' else BF16_TABLE_SUFFIX
        if name in out and isinstance(out[name], torch.Tensor) and out[name].is_cuda and name + suffix not in out:
            add_bf16_table(out, key)
    return out


class NumpyBinarySource(object):
    """``{data_dir}/{name}/{base_name}.npy`` -> ``{name: array}``: the loader half of the un-vendored
    ``tts_data_tools.data_sources.NumpyBinarySource`` the reference's models name in ``train_data_sources``
    (models/f0_test_model.py:60-69).  ``FilesDataset`` only needs a ``use_deltas`` attribute and a call
    ``(base_name, data_dir) -> dict`` (data.py:93, :135, :142).  Arrays come back as stored: float32 ``(len, D)`` sequence
    features, integer ``(P, 1)`` durations.

    ``use_deltas`` says that the feature has a delta stream ``{name}_deltas``; ``deltas`` says where it comes from.  ``'file'`` (the
    default, the reference's behaviour): ``{data_dir}/{name}_deltas/{base_name}.npy`` is loaded next to the statics - a file
    ``tts_data_tools`` wrote.  ``'compute'``: only ``{name}`` is loaded and the source carries a ``DeltaSpec(windows, edge)`` in
    ``delta_spec``; ``FilesDataset.__getitem__`` then computes the deltas on the host (``compute_deltas``) and the device loaders
    (``DeviceBatches``, ``collate_to_device``, ``fit_normalisers``) compute them on the device from the statics they upload anyway, so
    no ``_deltas`` file is needed and a quarter of the bytes is read, packed and copied.  ``windows`` / ``edge``: see ``compute_deltas``."""

    def __init__(self, name, use_deltas=False, ext='npy', deltas='file', windows=None, edge='replicate'):
        if deltas not in ('file', 'compute'):
            raise ValueError("deltas must be 'file' or 'compute', got %r" % (deltas,))
        if deltas == 'compute' and not use_deltas:
            raise ValueError("deltas='compute' goes with use_deltas=True")
        self.name, self.use_deltas, self.ext, self.deltas = name, use_deltas, ext, deltas
        self.delta_spec = DeltaSpec(windows, edge) if deltas == 'compute' else None

    def file_path(self, base_name, data_dir, name=None):
        return os.path.join(data_dir, name or self.name, '{}.{}'.format(base_name, self.ext))

    def __call__(self, base_name, data_dir):
        features = {self.name: np.load(self.file_path(base_name, data_dir))}
        if self.use_deltas and self.delta_spec is None:
            deltas = self.name + '_deltas'
            features[deltas] = np.load(self.file_path(base_name, data_dir, deltas))
        return features


class ContinuousLF0Source(object):
    """``{data_dir}/{f0_name}/{base_name}.npy`` -> ``{f0_name: array}``: the data source of a continuous log-F0 feature ``name`` (and its
    voicing flag ``vuv_name``) for a corpus that holds an extractor's raw F0 track - 0 where unvoiced - and not the ``lf0`` / ``vuv``
    files of ``tts_data_tools``.  Only the raw track is loaded.  The source carries ``f0_spec`` (an ``F0Spec``: ``log_input``,
    ``voiced_above``, ``fill`` - see ``continuous_lf0``): ``FilesDataset.__getitem__`` computes ``name`` and ``vuv_name`` on the host, the
    device loaders (``DeviceBatches``, ``collate_to_device``, ``fit_normalisers``) on the device from the one column they upload.

    ``use_deltas``: the feature has a delta stream ``{name}_deltas``.  Deltas of a computed feature are always computed: the source
    then carries ``delta_spec = DeltaSpec(windows, edge)`` as ``NumpyBinarySource(..., deltas='compute')`` does."""

    def __init__(self, name='lf0', f0_name='f0', vuv_name=VUV_KEY, use_deltas=False, windows=None, edge='replicate', ext='npy',
                 log_input=False, voiced_above=None, fill=0.):
        if len({name, f0_name, vuv_name}) != 3:
            raise ValueError('ContinuousLF0Source: name=%r, f0_name=%r and vuv_name=%r must differ' % (name, f0_name, vuv_name))
        self.name, self.f0_name, self.vuv_name, self.use_deltas, self.ext = name, f0_name, vuv_name, use_deltas, ext
        self.f0_spec = F0Spec(source=f0_name, vuv=vuv_name, log_input=log_input, voiced_above=voiced_above, fill=fill)
        self.delta_spec = DeltaSpec(windows, edge) if use_deltas else None

    def file_path(self, base_name, data_dir):
        return os.path.join(data_dir, self.f0_name, '{}.{}'.format(base_name, self.ext))

    def __call__(self, base_name, data_dir):
        track = np.load(self.file_path(base_name, data_dir)).astype(np.float32, copy=False)      # (WORLD writes float64 tracks)
        return {self.f0_name: track.reshape(-1, 1) if track.ndim == 1 else track}


class FrameCountersSource(object):
    """The data source of a frame-level positional feature ``name`` (``counters``) for a corpus that holds durations and not the
    ``counters`` files of ``tts_data_tools``: it loads NO file.  ``dur_name`` is a feature another data source provides - ``'dur'``, or a
    ``'state_dur'`` ``(P, S)`` array loaded by ``NumpyBinarySource('state_dur')``.  The source carries ``counter_spec`` (a ``CountersSpec``:
    ``kind`` - see ``frame_counters``): ``FilesDataset.__getitem__`` computes the feature on the host, the device loaders (``DeviceBatches``,
    ``collate_to_device``, ``fit_normalisers``) on the device from the durations they upload anyway."""

    use_deltas = False

    def __init__(self, name='counters', dur_name='dur', kind='full'):
        if name == dur_name:
            raise ValueError('FrameCountersSource: name=%r and dur_name=%r must differ' % (name, dur_name))
        self.name, self.dur_name = name, dur_name
        self.counter_spec = CountersSpec(source=dur_name, kind=kind)

    def __call__(self, base_name, data_dir):
        return {}


class TextSource(object):
    """``{data_dir}/{name}/{base_name}.txt`` holding one number -> ``{name: int}`` (or float): the sentence-level counts
    (``n_frames``, ``n_phones``) of the reference's data layout (README.rst:139-150)."""

    use_deltas = False

    def __init__(self, name, ext='txt'):
        self.name, self.ext = name, ext

    def __call__(self, base_name, data_dir):
        with open(os.path.join(data_dir, self.name, '{}.{}'.format(base_name, self.ext))) as f:
            text = f.read().strip()
        try:
            return {self.name: int(text)}
        except ValueError:
            return {self.name: float(text)}


class StringSource(object):
    """``{data_dir}/{name}/{base_name}.txt`` -> ``{name: its text}``: the ``speaker_id`` data source a corpus with speaker-dependent
    normalisers defines (data.py:85, :134-136)."""

    use_deltas = False

    def __init__(self, name, ext='txt'):
        self.name, self.ext = name, ext

    def __call__(self, base_name, data_dir):
        with open(os.path.join(data_dir, self.name, '{}.{}'.format(base_name, self.ext))) as f:
            return {self.name: f.read().strip()}


class FilesDataset(object):
    """File-backed utterances in front of ``DeviceBatches``: the reference's ``FilesDataset`` (data.py:60-157) - same constructor
    arguments, id-list handling (joined to ``data_root``, not to the split directory: data.py:100) and checks (:89-94).

    ``dataset[i]`` is what the reference's ``__getitem__`` returns: the features of every data source plus, for each feature with a
    normaliser, its ``normalised_`` twin computed on the host in NumPy and cast to float32 (:119-127, :144-150).
    ``dataset.raw(i)`` is the same utterance WITHOUT the twins - what ``DeviceBatches`` takes, because ``collate_to_device`` pads
    and normalises on the device in one pass.  With a speaker-dependent normaliser a data source named ``speaker_id`` must exist
    (:88-91); it is read first and its value handed to those normalisers (:119-136).

    A data source that computes its deltas (``NumpyBinarySource(..., deltas='compute')``) yields statics only: ``raw`` has no
    ``name_deltas``, ``__getitem__`` adds it (and its normalised twin) with the host form of ``compute_deltas``, and the device
    loaders take ``delta_specs()`` and compute it on the device.

    A ``ContinuousLF0Source`` yields the raw F0 track only: ``raw`` has ``f0``, ``__getitem__`` adds ``lf0`` and ``vuv`` with the host
    form of ``continuous_lf0``, then the deltas and the normalised twins, in that order, and the device loaders take ``f0_specs()``.

    A ``FrameCountersSource`` loads nothing: ``raw`` does not have ``counters``, ``__getitem__`` adds it with the host form of
    ``frame_counters`` from the durations another source loaded, before the normalised twins, and the device loaders take
    ``counter_specs()``."""

    def __init__(self, data_sources, data_dir, id_list, normalisers, data_root='.'):
        for name, normaliser in normalisers.items():
            if isinstance(normaliser, _SpeakerDependentNormaliser) and SPEAKER_ID_KEY not in data_sources:
                raise KeyError(f"{name} is a speaker-dependent normaliser, but no 'speaker_id' data_source was defined")
            if name in data_sources and normaliser.use_deltas and not data_sources[name].use_deltas:
                raise ValueError(f'To normalise deltas of {name}, set `data_source.use_deltas` to True.')
        self.data_sources = data_sources
        self.data_root = data_root
        self.data_dir = os.path.join(data_root, data_dir)
        self.id_list = os.path.join(data_root, id_list)
        with open(self.id_list, 'r') as f:
            self.file_ids = [line.strip() for line in f if line.strip()]
        self.normalisers = normalisers

    def __len__(self):
        return len(self.file_ids)

    def delta_specs(self):
        """{feature name: DeltaSpec} of the data sources that compute their deltas."""
        return {name: source.delta_spec for name, source in self.data_sources.items() if getattr(source, 'delta_spec', None) is not None}

    def f0_specs(self):
        """{feature name: F0Spec} of the data sources that compute a continuous log-F0 from a raw F0 track."""
        return {name: source.f0_spec for name, source in self.data_sources.items() if getattr(source, 'f0_spec', None) is not None}

    def counter_specs(self):
        """{feature name: CountersSpec} of the data sources that compute frame-level positional features from durations."""
        return {name: source.counter_spec for name, source in self.data_sources.items() if getattr(source, 'counter_spec', None) is not None}

    def raw(self, index):
        base_name = self.file_ids[index]
        features = {'name': base_name}
        if SPEAKER_ID_KEY in self.data_sources:           # first, so that the normalisers of the other features can use it
            features.update(self.data_sources[SPEAKER_ID_KEY](base_name, self.data_dir))
        for name, data_source in self.data_sources.items():
            if name != SPEAKER_ID_KEY:
                features.update(data_source(base_name, self.data_dir))
        return features

    def __getitem__(self, index):
        features = self.raw(index)
        f0_specs = self.f0_specs()
        _check_f0_specs(f0_specs, features)
        for name, spec in f0_specs.items():
            features[name], features[spec.vuv] = _host_continuous_lf0(features[spec.source], spec)
        for name, spec in self.delta_specs().items():
            features[name + DELTAS_SUFFIX] = compute_deltas(features[name], spec.windows, spec.edge)
        counter_specs = self.counter_specs()
        _check_counter_specs(counter_specs, features)
        for name, spec in counter_specs.items():
            features[name] = _host_frame_counters(features[spec.source], spec.kind)
        for name in self.data_sources:
            normaliser = self.normalisers.get(name)
            if normaliser is None or name == SPEAKER_ID_KEY:
                continue
            who = (features[SPEAKER_ID_KEY],) if isinstance(normaliser, _SpeakerDependentNormaliser) else ()
            features['normalised_' + name] = normaliser.normalise(features[name], *who).astype(np.float32)
            if normaliser.use_deltas:
                deltas = name + '_deltas'
                features['normalised_' + deltas] = normaliser.normalise(features[deltas], *who, deltas=True).astype(np.float32)
        return features

    collate_fn = staticmethod(collate_fn)


def batch(data_generator, batch_size=32, shuffle=True, num_data_threads=0, device='cuda:0', bf16_tables=(), delta_specs=None,
          f0_specs=None, counter_specs=None):
    """The reference's ``data.batch`` (data.py:29-57) for a ``FilesDataset``: a loader of device-resident batches.  Files are read
    on the calling thread as each batch is formed (``num_data_threads`` is accepted for signature compatibility; worker
    subprocesses are the reference's answer to a host-bound collate, which here runs on the device)."""
    rng = np.random.RandomState(torch.initial_seed() % (2 ** 32)) if shuffle else None
    return DeviceBatches(data_generator, batch_size, data_generator.normalisers, device, shuffle=rng, bf16_tables=bf16_tables,
                         delta_specs=delta_specs, f0_specs=f0_specs, counter_specs=counter_specs)


class DeviceBatches(object):
    """The DataLoader + ``ToDeviceWrapper`` of the reference (data.py:50-55, :648-663): an iterable of feature dicts on ``device``,
    each batch padded and normalised there by ``collate_to_device``.  ``utterances`` is a ``FilesDataset`` (read lazily, batch by
    batch, through ``raw``) or a sequence of utterances that are already in host memory.

    ``bf16_tables``, ``delta_specs``, ``f0_specs``, ``counter_specs``: see ``collate_to_device``; ``delta_specs=None`` / ``f0_specs=None`` /
    ``counter_specs=None`` take what the data sources of a ``FilesDataset`` ask for (``FilesDataset.delta_specs`` / ``f0_specs`` /
    ``counter_specs``).  ``utterances`` is a sequence of RAW per-utterance feature dicts (what a ``_DataSource`` returns: float32 ``(len, D)``
    arrays, integer ``dur``, python ints, the name); ``normalisers`` maps feature names to normalisers (``Normalisers`` or a
    dict).  Batches are contiguous slices in the given order, or a fresh permutation per epoch from ``shuffle`` = a
    ``numpy.random.RandomState`` (the reference shuffles with torch's global generator, data.py:50); the last, smaller batch
    is kept, as ``DataLoader`` does by default.  ``ExperimentBuilder.train_epoch`` takes it like any other loader."""

    def __init__(self, utterances, batch_size, normalisers, device, shuffle=None, bf16_tables=(), delta_specs=None, f0_specs=None,
                 counter_specs=None):
        if batch_size <= 0:
            raise ValueError('batch_size must be positive, got %r' % (batch_size,))
        self.utterances = utterances if isinstance(utterances, FilesDataset) else list(utterances)
        self.batch_size = int(batch_size)
        self.normalisers = normalisers
        self.device = torch.device(device)
        self.shuffle = shuffle
        self.bf16_tables = tuple(bf16_tables or ())
        self.delta_specs = _delta_specs_of(self.utterances, delta_specs)
        self.f0_specs = _f0_specs_of(self.utterances, f0_specs)
        self.counter_specs = _counter_specs_of(self.utterances, counter_specs)

    def use_bf16_tables(self, names):
        """The loader half of bf16 mode: every batch from now on carries the bf16 operand tables of these (normalised, phone-level)
        features - ``ExperimentBuilder`` asks for what its model's ``bf16_table_features()`` names."""
        self.bf16_tables = tuple(names or ())
        return self

    def __len__(self):
        return (len(self.utterances) + self.batch_size - 1) // self.batch_size

    def resident(self):
        """One pass of this loader kept on the device: the list of its batches (operand tables included).  A corpus of this model
        family fits the 288 GB of an MI355X many times over, and a host loader cannot feed the step (a C2 batch is 49 MB of float32
        over PCIe: >= 1 ms against a 0.1 ms step) - so later epochs take the list: ``ExperimentBuilder.train_epoch(use_graphs=True)``
        replays ``graph_group`` consecutive batches per graph launch, read where they lie.  The batches keep this pass's composition
        and order (a ``shuffle`` applies to the pass that builds the list)."""
        return list(iter(self))

    def __iter__(self):
        order = np.arange(len(self.utterances))
        if self.shuffle is not None:
            order = self.shuffle.permutation(len(self.utterances))
        for start in range(0, len(order), self.batch_size):
            fetch = self.utterances.raw if isinstance(self.utterances, FilesDataset) else self.utterances.__getitem__
            batch = [fetch(int(i)) for i in order[start:start + self.batch_size]]
            yield collate_to_device(batch, self.normalisers, self.device, bf16_tables=self.bf16_tables, delta_specs=self.delta_specs,
                                    f0_specs=self.f0_specs, counter_specs=self.counter_specs)


class ColumnStats(object):
    """Running per-column statistics of one feature on the device: the (groups, 5, dim) float64 state of ``ops.column_stats`` -
    count, mean, M2 = sum (x - mean)^2, min, max - updated in place batch after batch and read by the host once, in ``result``.
    ``groups`` > 1: one row per speaker, every item assigned by ``item_row``.  There is no CPU path: ``device`` must be a HIP device.

    Two states of disjoint data merge by the same Chan update the kernel uses (a multi-rank fit would do that on the host; not
    built here)."""

    FIELDS = ('count', 'mean', 'M2', 'mmin', 'mmax')

    def __init__(self, dim, groups=1, device='cuda:0'):
        from ._lib import MorganaHipError
        device = torch.device(device)
        if device.type != 'cuda':
            raise MorganaHipError('ColumnStats accumulates on an MI355X device, got %s (there is no CPU fallback)' % device)
        if dim <= 0 or groups <= 0:
            raise ValueError('ColumnStats: dim=%r and groups=%r must be positive' % (dim, groups))
        self.dim, self.groups = int(dim), int(groups)
        self.state = torch.zeros((self.groups, len(self.FIELDS), self.dim), dtype=torch.float64, device=device)

    @classmethod
    def from_state(cls, state):
        """A ColumnStats around an existing (groups, 5, dim) float64 state (a tensor on any device, or an array): for reading it."""
        self = cls.__new__(cls)
        state = state if isinstance(state, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(state, dtype=np.float64))
        if state.dim() != 3 or state.shape[1] != len(cls.FIELDS) or state.dtype != torch.float64:
            raise ValueError('ColumnStats state must be float64 (groups, %d, dim), got %s %s' % (
                len(cls.FIELDS), state.dtype, tuple(state.shape)))
        self.groups, self.dim, self.state = int(state.shape[0]), int(state.shape[2]), state
        return self

    def update_packed(self, packed, offsets, item_row=None, max_rows=None):
        """Rows (N, dim) float32 of B items back to back and their ``offsets`` (B + 1,) int64, as ``_pack_pinned`` makes them."""
        ops.column_stats(self.state, packed, offsets=offsets, item_row=item_row, max_rows=max_rows)
        return self

    def update_padded(self, x, seq_len, item_row=None):
        """A padded (B, T, dim) float32 batch and its ``seq_len`` (B,) int64 - what a resident batch holds; frames past the length
        are not read."""
        ops.column_stats(self.state, x, seq_len=seq_len, item_row=item_row)
        return self

    def result(self, ddof=0):
        """The one device-to-host read.  float64 arrays ``count``, ``mean``, ``var``, ``std_dev``, ``mmin``, ``mmax``, each
        (groups, dim); ``var = M2 / (count - ddof)`` floored at 0.  A group that saw no frame (count == 0) has NaN everywhere else,
        and so has ``var`` where ``count - ddof <= 0``.

        ``ddof=0`` (population variance) is the default because that is what the parameter files of ``tts_data_tools`` are
        believed to hold; this could not be verified - the package is not vendored with the reference - so it stays an argument."""
        host = self.state.detach().cpu().numpy()
        count, mean, m2, mmin, mmax = (host[:, i].copy() for i in range(len(self.FIELDS)))
        seen = count > 0
        nan = np.full_like(mean, np.nan)
        denom = count - ddof
        with np.errstate(divide='ignore', invalid='ignore'):
            var = np.where(seen & (denom > 0), np.maximum(m2 / np.where(denom > 0, denom, 1.0), 0.0), nan)
        return {'count': count, 'mean': np.where(seen, mean, nan), 'var': var, 'std_dev': np.sqrt(var),
                'mmin': np.where(seen, mmin, nan), 'mmax': np.where(seen, mmax, nan)}

    def params(self, kind, group=0, ddof=0, result=None):
        """The parameter vectors of a normaliser of ``kind`` ('mvn': mean, std_dev; 'minmax': mmin, mmax) for one group, rounded once
        from float64 to float32."""
        result = self.result(ddof) if result is None else result
        return {name: result[name][group].astype(np.float32) for name in _KINDS[kind]['params']}


def _fit_rows(utterance, key):
    value = np.asarray(utterance[key])
    if value.ndim == 1:
        value = value.reshape(-1, 1)
    if value.ndim != 2:
        raise ValueError('fit_normalisers: feature %r of utterance %r is not a (frames, features) array' % (key, utterance.get('name')))
    return value


def fit_normalisers(utterances, normalisers, device='cuda:0', batch_size=64, out_dir=None, data_root='.', ddof=0, delta_specs=None,
                    f0_specs=None, counter_specs=None):
    """Fit the parameters of ``normalisers`` (a ``Normalisers`` or a dict name -> normaliser of any of the four classes) to a corpus:
    the step that produces the ``{name}_mvn.json`` / ``{name}_minmax.json`` files (the reference gets them from ``tts_data_tools``).

    ``utterances``: a ``FilesDataset`` (read through ``raw``: its normalisers need no parameters yet) or a sequence of raw utterance
    dicts.  Batch by batch every named feature - and ``name + '_deltas'`` where ``use_deltas`` - is packed (``_pack_pinned``; integer
    arrays such as ``dur`` go through float32, exact below 2^24) and one ``ColumnStats`` per feature is updated on ``device``;
    speaker-dependent normalisers get one state row per speaker of their id list.  One read per feature at the end, then
    ``set_params`` on every normaliser and, with ``out_dir``, ``save_params(out_dir, data_root)``.

    ``delta_specs``: {feature name: ``DeltaSpec``}, default what the data sources of a ``FilesDataset`` ask for.  ``name + '_deltas'`` of
    such a feature is not read from the utterances: mg_deltas_f32 (csrc/deltas.hip) writes it, packed as the statics are, from the
    statics uploaded for ``name``, and ``ColumnStats.update_packed`` reads that.  An utterance that carries it anyway is refused.

    ``f0_specs``: {feature name: ``F0Spec``}, default what the data sources of a ``FilesDataset`` ask for.  ``name`` is not read from the
    utterances: the raw F0 track ``spec.source`` is uploaded and mg_continuous_lf0_f32 (csrc/f0.hip) writes the packed continuous
    log-F0, over which the statistics of ``name`` - and, through mg_deltas_f32, of ``name + '_deltas'``, which must then be in
    ``delta_specs`` - are taken: ALL frames, the interpolated ones included, the Merlin convention.

    ``counter_specs``: {feature name: ``CountersSpec``}, default what the data sources of a ``FilesDataset`` ask for.  ``name`` is not read
    from the utterances: the durations ``spec.source`` are uploaded, mg_frame_counters_f32 (csrc/counters.hip) writes the padded
    counters and ``ColumnStats.update_padded`` reads the frames below each utterance's sum of durations - what a ``counters`` file of the
    utterance would hold.  Such a feature has no deltas.

    Raises ValueError before anything is set or written if a listed speaker has no frame or a fitted parameter is not finite.
    ``ddof``: see ``ColumnStats.result``.  Returns {feature: ColumnStats.result()} (the ``_deltas`` features under their own names)."""
    from ._lib import MorganaHipError
    device = torch.device(device)
    if device.type != 'cuda':
        raise MorganaHipError('fit_normalisers runs on an MI355X device, got %s (there is no CPU fallback)' % device)
    if batch_size <= 0:
        raise ValueError('batch_size must be positive, got %r' % (batch_size,))
    for normaliser in normalisers.values():
        if isinstance(normaliser, _SpeakerDependentNormaliser) and normaliser.speaker_ids is None:
            normaliser.speaker_ids = _read_id_list(os.path.join(data_root, normaliser.speaker_id_list))
    order = _speaker_order(normalisers)
    features = []                                         # (feature key, normaliser, is the deltas group)
    for name, normaliser in normalisers.items():
        features.append((name, normaliser, False))
        if normaliser.use_deltas:
            features.append((name + '_deltas', normaliser, True))
    from_files = isinstance(utterances, FilesDataset)
    fetch = utterances.raw if from_files else utterances.__getitem__
    delta_specs = _delta_specs_of(utterances, delta_specs)
    for name in delta_specs:
        if name not in normalisers or not normalisers[name].use_deltas:
            raise ValueError('delta_specs names %r, which has no normaliser with use_deltas' % name)
    f0_specs = {name: spec for name, spec in _f0_specs_of(utterances, f0_specs).items() if name in normalisers}
    for name in f0_specs:
        if normalisers[name].use_deltas and name not in delta_specs:
            raise ValueError('%r is computed from %r: its deltas are computed too, name it in delta_specs' % (name, f0_specs[name].source))
    counter_specs = {name: spec for name, spec in _counter_specs_of(utterances, counter_specs).items() if name in normalisers}
    for name in counter_specs:
        if normalisers[name].use_deltas:
            raise ValueError('%r is computed from the durations %r: it has no deltas' % (name, counter_specs[name].source))
    stats = {}
    for start in range(0, len(utterances), batch_size):
        items = [fetch(i) for i in range(start, min(start + batch_size, len(utterances)))]
        item_row = None
        if order is not None:
            if SPEAKER_ID_KEY not in items[0]:
                raise KeyError("speaker-dependent normalisers need a '%s' entry in every utterance" % SPEAKER_ID_KEY)
            index = torch.from_numpy(speaker_index_of([item[SPEAKER_ID_KEY] for item in items], order))
            item_row = _small_to_device({SPEAKER_INDEX_KEY: index}, device)[SPEAKER_INDEX_KEY]
        uploaded = {}                                     # the packed statics of this batch, for the features whose deltas are computed
        if start == 0:
            _check_f0_specs(f0_specs, items[0])
            _check_counter_specs(counter_specs, items[0])
        for key, normaliser, is_deltas in features:
            by_speaker = isinstance(normaliser, _SpeakerDependentNormaliser)
            base = key[:-len(DELTAS_SUFFIX)] if is_deltas else key
            if key in counter_specs:                      # the durations -> padded counters on the device, in place of a file's rows
                spec = counter_specs[key]
                durs = [_host_durations(item[spec.source], 'fit_normalisers') for item in items]
                lens = np.array([int(d.sum()) for d in durs], dtype=np.int64)
                small = collate_fn([{'dur': d} for d in durs])
                small['lens'] = torch.from_numpy(lens)
                small = _small_to_device(small, device)
                padded, _ = ops.frame_counters(small['dur'], t=int(lens.max()), kind=spec.kind)
                if key not in stats:
                    stats[key] = ColumnStats(padded.shape[2], groups=len(order) if by_speaker else 1, device=device)
                stats[key].update_padded(padded, small['lens'], item_row if by_speaker else None)
                continue
            if is_deltas and base in delta_specs:
                if key in items[0]:
                    raise ValueError('%r is in the utterances and in delta_specs: deltas are read from files or computed, not both' % key)
                spec, (statics, offsets, lens) = delta_specs[base], uploaded[base]
                packed, _ = ops.deltas(statics, spec.windows, offsets=offsets, edge=spec.edge, packed_rows=statics.shape[0])
            else:
                rows = [_fit_rows(item, f0_specs[key].source if key in f0_specs else key) for item in items]
                packed, offsets, lens = _pack_pinned(rows, device, 'fit:' + key)
                if key in f0_specs:                       # the raw track -> the packed continuous log-F0, in place of a file's rows
                    spec = f0_specs[key]
                    packed = ops.continuous_lf0(packed, offsets=offsets, log_input=spec.log_input, voiced_above=spec.voiced_above,
                                                fill=spec.fill)[3]
                if key in delta_specs:
                    uploaded[key] = (packed, offsets, lens)
            if key not in stats:
                stats[key] = ColumnStats(packed.shape[1], groups=len(order) if by_speaker else 1, device=device)
            stats[key].update_packed(packed, offsets, item_row if by_speaker else None, max_rows=int(lens.max()))
    if not stats:
        raise ValueError('fit_normalisers: no utterances')
    results = {key: stats[key].result(ddof) for key, _, _ in features}
    for key, normaliser, _ in features:                   # refuse before anything is installed or written
        result = results[key]
        if isinstance(normaliser, _SpeakerDependentNormaliser):
            absent = [spk for row, spk in enumerate(order) if not result['count'][row].any()]
            if absent:
                raise ValueError('fit_normalisers: feature %r has no frame of the listed speakers %s' % (key, absent))
        for name in _KINDS[normaliser.kind]['params']:
            bad = np.argwhere(~np.isfinite(result[name]))
            if bad.size:
                raise ValueError('fit_normalisers: %s of feature %r is not finite in columns %s%s' % (
                    name, key, sorted(set(int(c) for c in bad[:, 1])),
                    '' if order is None or result[name].shape[0] == 1 else ' (speakers %s)' % sorted(set(order[int(r)] for r in bad[:, 0]))))
    for name, normaliser in normalisers.items():
        if isinstance(normaliser, _SpeakerDependentNormaliser):
            own = {spk: stats[name].params(normaliser.kind, row, result=results[name]) for row, spk in enumerate(order)}
            deltas = ({spk: stats[name + '_deltas'].params(normaliser.kind, row, result=results[name + '_deltas'])
                       for row, spk in enumerate(order)} if normaliser.use_deltas else None)
        else:
            own = stats[name].params(normaliser.kind, result=results[name])
            deltas = stats[name + '_deltas'].params(normaliser.kind, result=results[name + '_deltas']) if normaliser.use_deltas else None
        normaliser.set_params(own, deltas, device=device)
    if out_dir is not None:
        for normaliser in normalisers.values():
            normaliser.save_params(out_dir, data_root)
    return results


GV_SUFFIX = '_gv'


def fit_global_variance(utterances, names, device='cuda:0', batch_size=64, out_dir=None, data_root='.', speaker_id_list=None, ddof=0):
    """Fit the statistics of the global-variance prior of ``ops.mlpg_gv`` / ``StreamModel.generate_with_gv`` to a corpus: for every
    feature of ``names`` the mean and standard deviation, over the utterances, of the per-utterance variance of each column.

    ``utterances``: a ``FilesDataset`` (read through ``raw``) or a sequence of raw utterance dicts holding the STATIC feature under its
    name, (frames, D).  Batch by batch the feature is padded and uploaded, ``losses.global_variance`` gives the (utterances, D)
    biased variances on ``device`` (an utterance of one frame counts with variance 0), and those rows - one item of one frame each -
    go into a ``ColumnStats``; ``speaker_id_list`` (a file of names under ``data_root``) keeps one state row per speaker, every
    utterance assigned by its ``speaker_id``.  One read per feature at the end.

    Returns {name + '_gv': normaliser}: an ordinary ``MeanVarianceNormaliser(name + '_gv')`` (``mean`` = the GV mean, ``std_dev``^2 =
    the GV variance), or its speaker-dependent twin, with the parameters set; with ``out_dir`` also saved by ``save_params`` as
    ``{name}_gv_mvn.json`` (``{speaker}/{name}_gv_mvn.json``), which ``load_params`` reads back bit for bit.  Raises ValueError
    before anything is written if a listed speaker has no utterance or a statistic is not finite."""
    from ._lib import MorganaHipError
    from . import losses
    device = torch.device(device)
    if device.type != 'cuda':
        raise MorganaHipError('fit_global_variance runs on an MI355X device, got %s (there is no CPU fallback)' % device)
    if batch_size <= 0:
        raise ValueError('batch_size must be positive, got %r' % (batch_size,))
    names = [names] if isinstance(names, str) else list(names)
    if not names:
        raise ValueError('fit_global_variance: no feature names')
    order = None if speaker_id_list is None else _read_id_list(os.path.join(data_root, speaker_id_list))
    fetch = utterances.raw if isinstance(utterances, FilesDataset) else utterances.__getitem__
    stats = {}
    for start in range(0, len(utterances), batch_size):
        items = [fetch(i) for i in range(start, min(start + batch_size, len(utterances)))]
        item_row = None
        if order is not None:
            if SPEAKER_ID_KEY not in items[0]:
                raise KeyError("per-speaker statistics need a '%s' entry in every utterance" % SPEAKER_ID_KEY)
            item_row = torch.from_numpy(speaker_index_of([item[SPEAKER_ID_KEY] for item in items], order)).to(device)
        for name in names:
            rows = [np.asarray(_fit_rows(item, name), dtype=np.float32) for item in items]
            lens = np.array([len(r) for r in rows], dtype=np.int64)
            if (lens <= 0).any():
                raise ValueError('fit_global_variance: feature %r of an utterance has no frame' % name)
            padded = np.zeros((len(rows), int(lens.max()), rows[0].shape[1]), dtype=np.float32)
            for i, r in enumerate(rows):
                padded[i, :len(r)] = r
            variances = losses.global_variance(torch.from_numpy(padded).to(device), torch.from_numpy(lens).to(device))      # (B, D)
            if name not in stats:
                stats[name] = ColumnStats(variances.shape[1], groups=1 if order is None else len(order), device=device)
            stats[name].update_padded(variances[:, None, :].contiguous(), torch.ones(len(rows), dtype=torch.int64, device=device), item_row)
    if not stats:
        raise ValueError('fit_global_variance: no utterances')
    results = {name: stats[name].result(ddof) for name in names}
    for name in names:                                    # refuse before anything is written
        result = results[name]
        if order is not None:
            absent = [spk for row, spk in enumerate(order) if not result['count'][row].any()]
            if absent:
                raise ValueError('fit_global_variance: feature %r has no utterance of the listed speakers %s' % (name, absent))
        for key in ('mean', 'std_dev'):
            if not np.isfinite(result[key]).all():
                raise ValueError('fit_global_variance: %s of the variances of feature %r is not finite' % (key, name))
    fitted = {}
    for name in names:
        if order is None:
            normaliser = MeanVarianceNormaliser(name + GV_SUFFIX)
            normaliser.set_params(stats[name].params('mvn', result=results[name]), device=device)
        else:
            normaliser = SpeakerDependentMeanVarianceNormaliser(name + GV_SUFFIX, speaker_id_list)
            normaliser.speaker_ids = list(order)
            normaliser.set_params({spk: stats[name].params('mvn', row, result=results[name]) for row, spk in enumerate(order)},
                                  device=device)
        if out_dir is not None:
            normaliser.save_params(out_dir, data_root)
        fitted[name + GV_SUFFIX] = normaliser
    return fitted


# ---- vocoder analysis (csrc/analysis.hip): from what an analyser such as WORLD writes (f0, sp, ap) to the features the models read.
# The opposite direction of viz.synthesis.world_features.  The coding runs ONCE per corpus (extract_world_features), not in a loader:
# re-coding 8 KB of spectrum per frame every epoch to get 240 B of features is the wrong trade.
def _analysis_device(what, *values):
    """The device of the first tensor among ``values``, else the current device; without one there is nothing to run on."""
    from ._lib import MorganaHipError
    for v in values:
        if isinstance(v, torch.Tensor):
            _on_device(what, v)
            return v.device
    if not torch.cuda.is_available():
        raise MorganaHipError('%s runs only on an MI355X device (no CPU fallback)' % what)
    return torch.device('cuda', torch.cuda.current_device())


def _analysis_upload(what, x, device, dtype=None):
    """A spectrum-like feature on the device in the float type it comes in (float32 or float64; anything else becomes float64), or
    in ``dtype``: an array is uploaded, a device tensor taken as it is."""
    if isinstance(x, torch.Tensor):
        _on_device(what, x)
        x = x.detach()
    else:
        x = torch.from_numpy(np.array(x)).to(device)
    if dtype is None:
        dtype = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float64
    return x.to(dtype=dtype)


def _analysis_batched(what, x, seq_len):
    """(padded (B, T, K) device tensor in its own float type, (B,) device lengths, (B + 1,) device offsets, rows of the packed output)
    of a feature given as (B, T, K) or (T, K) - the conventions of viz.synthesis.mcep_to_spectrum: host lengths are exact without a
    device read, device lengths leave B * T rows of which those from ``offsets[-1]`` on are not written."""
    x = _analysis_upload(what, x, _analysis_device(what, x, seq_len))
    if x.dim() == 2:
        x = x[None]
    if x.dim() != 3:
        raise ValueError('%s takes (batch_size, seq_len, bins) or (seq_len, bins), got %s' % (what, tuple(x.shape)))
    b, t = x.shape[:2]
    if seq_len is None:
        lengths, rows = torch.full((b,), t, dtype=torch.int64, device=x.device), b * t
    elif isinstance(seq_len, torch.Tensor):
        lengths, rows = seq_len.detach().reshape(-1).to(device=x.device, dtype=torch.int64).clamp(0, t), b * t
    else:
        host = np.clip(np.asarray(seq_len, dtype=np.int64).reshape(-1), 0, t)
        lengths, rows = torch.from_numpy(host).to(x.device), int(host.sum())
    if lengths.numel() != b:
        raise ValueError('%s: seq_len holds %d lengths for %d items' % (what, lengths.numel(), b))
    offsets = torch.zeros((b + 1,), dtype=torch.int64, device=x.device)
    torch.cumsum(lengths, 0, out=offsets[1:])
    return x, lengths, offsets, rows


def spectrum_to_mcep(sp, order, alpha, fft_size=None, seq_len=None, log_input=False, dtype=torch.float32):
    r"""Power spectrum to mel-cepstrum (``csrc/analysis.hip``): ``c = table (0.5 log sp)`` per frame in float64, ``table`` the one-sided
    cepstrum followed by SPTK's ``freqt(alpha)`` (``ops.mcep_analysis_table``) - ``pysptk.sp2mc`` as its source is remembered, which
    could not be checked: the package is not available.  Where the warped series does not alias (every shipped setting) it is the left
    inverse of ``viz.synthesis.mcep_to_spectrum``.

    sp : (batch_size, seq_len, fft_size / 2 + 1) or (seq_len, fft_size / 2 + 1), float32 or float64 - a NumPy array is uploaded in
    its own type, a device tensor taken as it is; order : coefficients per frame; fft_size : None is ``2 (bins - 1)``; log_input : sp is
    a log power spectrum.  Returns (mcep, offsets): the PACKED (rows, order) device tensor of ``dtype`` and the (batch_size + 1,) int64
    device offsets.  There is no host implementation: without the HIP library this raises."""
    sp, lengths, offsets, rows = _analysis_batched('spectrum_to_mcep', sp, seq_len)
    return ops.spectrum_mcep(sp, order, alpha, fft_size, seq_len=lengths, packed_rows=rows, log_input=log_input, out_dtype=dtype), offsets


def aperiodicity_to_bap(ap, sample_rate, n_bands=None, fft_size=None, seq_len=None, dtype=torch.float32):
    r"""Full-band aperiodicity to coded band aperiodicity in dB, one column per 3 kHz band (``csrc/analysis.hip``): ``20 log10(ap)``
    clamped to [-60, 0] and interpolated linearly between the two bins around 3000 (b + 1) Hz - WORLD's ``CodeAperiodicity`` as
    remembered; it could not be checked against ``pyworld``.  n_bands : None is WORLD's rule (1 at 16 kHz, 5 at 48 kHz).  Arguments and
    returns as ``spectrum_to_mcep``."""
    ap, lengths, offsets, rows = _analysis_batched('aperiodicity_to_bap', ap, seq_len)
    return ops.aperiodicity_bap(ap, int(sample_rate), n_bands, fft_size, seq_len=lengths, packed_rows=rows, out_dtype=dtype), offsets


def _analysis_items(what, x, seq_len, form):
    """A feature of several utterances as a list of per-utterance (n, columns) views.  ``form``: 'list' - a list / tuple of arrays or
    tensors, taken as it is; 'one' - one utterance, a list of one; 'padded' - a (B, T, ...) batch cut to the host lengths ``seq_len``."""
    if form == 'list':
        if not isinstance(x, (list, tuple)):
            raise TypeError('%s: f0, sp and ap come in one form: lists of utterances, one utterance or padded batches' % what)
        items = list(x)
    elif form == 'one':
        items = [x]
    else:
        if len(seq_len) != x.shape[0]:
            raise ValueError('%s: seq_len holds %d lengths for %d items' % (what, len(seq_len), x.shape[0]))
        items = [x[i, :max(int(n), 0)] for i, n in enumerate(seq_len)]
    return [v.reshape(v.shape[0], -1) for v in items]


def world_parameters(f0, sp, ap, sample_rate, n_mcep=60, alpha=None, n_bands=None, seq_len=None):
    r"""The acoustic features of the shipped models from what a WORLD-style analyser gives: the inverse of
    ``viz.synthesis.world_features``.

    f0 : (n,), sp, ap : (n, fft_size / 2 + 1) of one utterance; or lists of those, one entry per utterance (what ``world_features``
    returns, transposed: ``world_parameters(*zip(*features), sample_rate)``); or padded batches (B, T[, bins]) with seq_len (B,).  NumPy
    arrays are uploaded in their own float type, device tensors taken as they are.  alpha : None looks the rate up in
    ``viz.synthesis.MERLIN_ALPHA`` and raises for any other rate; n_bands : None is WORLD's rule (``ops.default_n_bands``).

    Returns per utterance ``(lf0 (n, 1), vuv (n, 1), mcep (n, n_mcep), bap (n, n_bands))``, float32 NumPy arrays - one tuple for one
    utterance, else a list of tuples.  ``lf0`` and ``vuv`` are ``continuous_lf0`` of ``f0``; ``mcep`` is ``spectrum_to_mcep``, ``bap`` is
    ``aperiodicity_to_bap``.  Each feature reaches the host in one copy.  There is no host implementation."""
    from .viz import synthesis
    what = 'world_parameters'
    if isinstance(seq_len, torch.Tensor):
        seq_len = seq_len.detach().reshape(-1).cpu().numpy()
    alpha = synthesis.default_alpha(sample_rate) if alpha is None else alpha
    form = 'list' if isinstance(sp, (list, tuple)) else 'one' if sp.ndim == 2 else 'padded'
    if (form == 'padded') != (seq_len is not None):
        raise ValueError('%s: seq_len goes with padded (B, T, bins) batches, and those need it' % what)
    single = form == 'one'
    f0_items, sp_items, ap_items = (_analysis_items(what, v, seq_len, form) for v in (f0, sp, ap))
    if not len(f0_items) == len(sp_items) == len(ap_items):
        raise ValueError('%s: %d, %d and %d utterances of f0, sp and ap' % (what, len(f0_items), len(sp_items), len(ap_items)))
    device = _analysis_device(what, *(f0_items + sp_items + ap_items))
    lens = np.array([v.shape[0] for v in sp_items], dtype=np.int64)
    for i, (a, b, c) in enumerate(zip(f0_items, sp_items, ap_items)):
        if a.shape[0] != b.shape[0] or c.shape != b.shape or a.shape[1] != 1:
            raise ValueError('%s: utterance %d has f0 %s, sp %s and ap %s' % (what, i, tuple(a.shape), tuple(b.shape), tuple(c.shape)))

    def packed(items, dtype=None):
        if all(isinstance(v, np.ndarray) for v in items):
            return _analysis_upload(what, np.concatenate(items) if len(items) > 1 else items[0], device, dtype)
        return torch.cat([_analysis_upload(what, v, device, dtype) for v in items])

    offsets = torch.from_numpy(np.concatenate(([0], np.cumsum(lens)))).to(device)
    _, _, vuv, lf0 = ops.continuous_lf0(packed(f0_items, torch.float32), offsets=offsets)
    mcep = ops.spectrum_mcep(packed(sp_items), n_mcep, alpha, offsets=offsets)
    bap = ops.aperiodicity_bap(packed(ap_items), int(sample_rate), n_bands, offsets=offsets)
    lf0, vuv, mcep, bap = lf0.cpu().numpy(), vuv.cpu().numpy(), mcep.cpu().numpy(), bap.cpu().numpy()
    ends = np.cumsum(lens)
    out = [(lf0[e - n:e], vuv[e - n:e], mcep[e - n:e], bap[e - n:e]) for e, n in zip(ends, lens)]
    return out[0] if single else out


def extract_world_features(ids, in_dir, out_dir, sample_rate, n_mcep=60, alpha=None, n_bands=None, device='cuda:0',
                           max_batch_bytes=256 << 20, overwrite=False):
    r"""Code a corpus: for every id read ``{in_dir}/sp/{id}.npy`` and ``{in_dir}/ap/{id}.npy`` ((n, fft_size / 2 + 1), float32 or
    float64, as an analyser wrote them) and write ``{out_dir}/mcep/{id}.npy`` (n, n_mcep) and ``{out_dir}/bap/{id}.npy`` (n, n_bands),
    float32.  ``lf0``, ``vuv``, deltas and counters need no files: ``ContinuousLF0Source``, ``deltas='compute'`` and
    ``FrameCountersSource`` make them from ``f0`` and ``dur`` at load time.

    Utterances are batched by bytes (``max_batch_bytes`` of input per batch, at least one utterance), never by count.  Per batch and
    feature the rows are packed into pinned memory and uploaded in ONE copy in the type they are stored in, coded in one launch
    (``ops.spectrum_mcep``, ``ops.aperiodicity_bap``), and exactly the packed result comes back in one more copy.  alpha, n_bands : as
    ``world_parameters``.  Refused, naming the id, before anything is written: an utterance whose sp and ap differ in length or width,
    and an output file that exists unless ``overwrite=True``.  Returns the number of frames written."""
    from ._lib import MorganaHipError
    from .viz import synthesis
    device = torch.device(device)
    if device.type != 'cuda' or not torch.cuda.is_available():
        raise MorganaHipError('extract_world_features runs on an MI355X device, got %s (there is no CPU fallback)' % device)
    alpha = synthesis.default_alpha(sample_rate) if alpha is None else alpha
    n_bands = ops.default_n_bands(sample_rate) if n_bands is None else n_bands
    ids = list(ids)
    paths = {name: os.path.join(out_dir, name) for name in ('mcep', 'bap')}
    if not overwrite:
        for utt in ids:
            for name in ('mcep', 'bap'):
                if os.path.exists(os.path.join(paths[name], '%s.npy' % utt)):
                    raise FileExistsError('extract_world_features: %s of utterance %r exists (overwrite=True replaces it)' % (name, utt))
    entries = []
    for utt in ids:                                           # memory maps: the one read of the samples is the pack into pinned memory
        sp = np.load(os.path.join(in_dir, 'sp', '%s.npy' % utt), mmap_mode='r')
        ap = np.load(os.path.join(in_dir, 'ap', '%s.npy' % utt), mmap_mode='r')
        if sp.ndim != 2 or ap.ndim != 2 or sp.shape != ap.shape:
            raise ValueError('extract_world_features: utterance %r has sp %s and ap %s' % (utt, sp.shape, ap.shape))
        for name, x in (('sp', sp), ('ap', ap)):
            if x.dtype not in (np.float32, np.float64):
                raise TypeError('extract_world_features: %s of utterance %r is %s, not float32 or float64' % (name, utt, x.dtype))
        if entries and sp.shape[1] != entries[0][1].shape[1]:
            raise ValueError('extract_world_features: utterance %r has %d bins, the first has %d' % (utt, sp.shape[1], entries[0][1].shape[1]))
        entries.append((utt, sp, ap))
    for path in paths.values():
        os.makedirs(path, exist_ok=True)
    frames, start = 0, 0
    while start < len(entries):
        stop, size = start, 0
        while stop < len(entries):                            # by bytes; one element type per feature and batch
            _, sp, ap = entries[stop]
            if stop > start and (size + sp.nbytes + ap.nbytes > max_batch_bytes or sp.dtype != entries[start][1].dtype
                                 or ap.dtype != entries[start][2].dtype):
                break
            size += sp.nbytes + ap.nbytes
            stop += 1
        chunk = entries[start:stop]
        with torch.cuda.device(device):
            sp_rows, offsets, lens = _pack_pinned([e[1] for e in chunk], device, 'extract:sp', chunk[0][1].dtype)
            mcep = ops.spectrum_mcep(sp_rows, n_mcep, alpha, offsets=offsets)
            ap_rows, offsets, _ = _pack_pinned([e[2] for e in chunk], device, 'extract:ap', chunk[0][2].dtype)
            bap = ops.aperiodicity_bap(ap_rows, int(sample_rate), n_bands, offsets=offsets)
            mcep, bap = mcep.cpu().numpy(), bap.cpu().numpy()
        ends = np.cumsum(lens)
        for (utt, _, _), e, n in zip(chunk, ends, lens):
            np.save(os.path.join(paths['mcep'], '%s.npy' % utt), mcep[e - n:e])
            np.save(os.path.join(paths['bap'], '%s.npy' % utt), bap[e - n:e])
        frames += int(lens.sum())
        start = stop
    return frames
