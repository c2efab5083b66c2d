"""The file-writing side of ``morgana.viz.io``: ``save_batched_seqs`` keeps the reference's name, arguments and error behaviour
(morgana/viz/io.py:10-56) and writes ``.npy`` files."""
import os
import wave

import numpy as np

from .. import utils


def _named_features(sequence_features, feat_names):
    """(names, tensors) of what is to be saved: a dict gives its own keys unless ``feat_names`` picks some of them; anything else
    needs ``feat_names``, one per feature."""
    if isinstance(sequence_features, dict):
        picked = list(sequence_features) if feat_names is None else list(feat_names)
        return picked, [sequence_features[key] for key in picked]
    if feat_names is None:
        raise ValueError('If sequences features is not a dictionary, then feat_names must be provided.')
    return list(feat_names), list(sequence_features)


def save_batched_seqs(sequence_features, names, out_dir, seq_len=None, feat_names=None):
    """Writes every utterance of every batched sequence feature to ``{out_dir}/feats/{feat_name}/{name}.npy``.

    sequence_features: a dict ``{feat_name: (B, T, D) tensor}``, or a list of such tensors together with ``feat_names`` (without
    them a list raises ``ValueError``); with a dict, ``feat_names`` selects the keys to save.  names: the B utterance names.
    seq_len: (B,) lengths, tensor or array - each item is cropped to its length; None saves the padded items.

    All features go through ONE ``utils.detach_batched_seqs`` call, so device tensors are packed on the device and reach the host in
    one copy, detached and squeezed as that function does.  A feature that does not come back as per-item arrays is skipped.  The
    files are written with ``np.save``: the reference writes through ``tts_data_tools.file_io.save_bin``, which is not a dependency
    here, and ``.npy`` is what ``data.NumpyBinarySource`` reads back, so saved features round-trip through this package's own loader.
    A single feature is saved per utterance like any other (the reference's zip pairs its first ITEM with the feature name)."""
    feat_names, tensors = _named_features(sequence_features, feat_names)
    root = os.path.join(out_dir, 'feats')
    os.makedirs(root, exist_ok=True)

    per_feature = utils.detach_batched_seqs(*tensors, seq_len=seq_len)
    if len(tensors) == 1:
        per_feature = [per_feature]           # a single feature comes back unwrapped

    for feat_name, items in zip(feat_names, per_feature):
        if not isinstance(items[0], np.ndarray):
            continue
        feat_dir = os.path.join(root, feat_name)
        os.makedirs(feat_dir, exist_ok=True)
        for name, item in zip(names, items):
            np.save(os.path.join(feat_dir, name + '.npy'), item)


def save_wav(path, wav, sample_rate):
    """Writes a mono waveform as 16-bit PCM with the standard library's ``wave`` (the reference writes through
    ``tts_data_tools.file_io.save_wav``, which is not a dependency here).  wav: 1-D samples - floating point in [-1, 1], scaled by
    32767, rounded and clipped; integers are taken as PCM values and clipped to int16.  A NaN sample is written as 0."""
    wav = np.asarray(wav)
    if wav.ndim != 1:
        raise ValueError('save_wav takes a 1-D (mono) waveform, got shape %s' % (wav.shape,))
    if not np.issubdtype(wav.dtype, np.integer):
        wav = np.rint(np.nan_to_num(wav.astype(np.float64), nan=0., posinf=1., neginf=-1.) * 32767.)
    pcm = np.clip(wav, -32768, 32767).astype('<i2')
    with wave.open(path, 'wb') as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(sample_rate))
        f.writeframes(pcm.tobytes())
