"""``morgana/viz/synthesis.py`` against this package: ``MLPG`` with the reference's signature and return conventions, solved on the
device (``csrc/mlpg.hip``) instead of on the host with ``bandmat``.

The reference calls this from ``predict`` of its shipped models (``models/f0_test_model.py:86-89``, ``models/RNN_SPSS.py:107-118``)
on every training step - a device -> host copy, B x D banded float64 solves in a Python loop, a host -> device copy - to feed the
LF0 / MCD metrics of ``loss``.  Here the delta streams never leave the device and nothing synchronises.

``mlpg_trajectory`` is the same solve as a differentiable layer (device tensors only), for losses taken on the trajectory itself.
"""
import os

import numpy as np
import torch

from .. import _lib, functional, ops

DEFAULT_WINDOWS = (                                  # synthesis.py:122-127
    (0, 0, np.array([1.0])),
    (1, 1, np.array([-0.5, 0.0, 0.5])),
    (1, 1, np.array([1.0, -2.0, 1.0])),
)


def _device_of(*values):
    for v in values:                                 # synthesis.py:101-112: the first tensor's device
        if isinstance(v, torch.Tensor):
            return v.device
    return None


def MLPG(means, variances, windows=None, padding_size=0, seq_len=None):
    r"""Performs maximum-likelihood parameter generation (synthesis.py:79-178).

    means : (batch_size, seq_len, feat_dim) or (seq_len, feat_dim); variances : the same shape, or (feat_dim,) global;
    windows : list of (l, u, coefficients), default static / delta / delta-delta; padding_size : frames repeated at either end
    as burn-in; seq_len : (batch_size,) lengths (frames past them come back as zeros).

    Returns the most probable trajectory, (batch_size, seq_len, feat_dim // len(windows)) or without the batch axis for a
    single sequence: a float32 tensor on the inputs' device if any input was a tensor (as the reference), else a float64 array.
    Tensors must live on the MI355X; numpy inputs are uploaded to the current device (float32, the dtype the model emits).
    There is no host implementation: without the HIP library this raises.
    """
    device = _device_of(means, variances, seq_len)
    as_tensor = device is not None
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.MorganaHipError('MLPG runs only on an MI355X device (no CPU fallback)')
        device = torch.device('cuda', torch.cuda.current_device())

    def put(x, dtype):
        if isinstance(x, torch.Tensor):
            return x.detach().to(device=device, dtype=dtype)
        return torch.as_tensor(np.ascontiguousarray(x)).to(device=device, dtype=dtype)

    means = put(means, torch.float32)
    variances = put(variances, torch.float32)
    if windows is None:
        windows = DEFAULT_WINDOWS
    using_batches = means.dim() != 2                  # :129-133
    if not using_batches:
        means = means[None]
        if variances.dim() == 2:
            variances = variances[None]               # :143-144
    if seq_len is not None:
        seq_len = put(seq_len, torch.int64).reshape(-1)
    out = ops.mlpg(means, variances, windows, padding_size=padding_size, seq_len=seq_len,
                   out_dtype=torch.float32 if as_tensor else torch.float64)
    if not using_batches:
        out = out.squeeze(0)                          # :173-174
    return out if as_tensor else out.cpu().numpy()    # :176-178


def MLPG_GV(means, variances, gv_mean, gv_variance, windows=None, padding_size=0, seq_len=None, gv_weight=1., max_iter=48):
    r"""``MLPG`` under a global-variance prior (Toda & Tokuda 2007; ``csrc/mlpg_gv.hip`` - the reference generates with ``MLPG`` only).

    means, variances, windows, padding_size, seq_len and the return conventions are ``MLPG``'s.  gv_mean, gv_variance :
    (feat_dim // len(windows),) mean and variance of the per-utterance variance of the static feature
    (``data.fit_global_variance``), or (batch_size, feat_dim // len(windows)) with one row per utterance (per-speaker statistics);
    gv_weight : the weight of the prior against the per-frame likelihood of ``MLPG`` (0: ``MLPG`` itself); max_iter : the most
    evaluations of the root search, a banded solve each.  An utterance of fewer than two frames, and any system whose search does
    not converge, comes back as ``MLPG`` gives it (``ops.mlpg_gv(..., want_info=True)`` tells which).
    """
    device = _device_of(means, variances, seq_len, gv_mean, gv_variance)
    as_tensor = device is not None
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.MorganaHipError('MLPG_GV runs only on an MI355X device (no CPU fallback)')
        device = torch.device('cuda', torch.cuda.current_device())

    def put(x, dtype):
        if isinstance(x, torch.Tensor):
            return x.detach().to(device=device, dtype=dtype)
        return torch.from_numpy(np.array(x)).to(device=device, dtype=dtype)      # a copy: a read-only array is welcome

    means = put(means, torch.float32)
    variances = put(variances, torch.float32)
    if windows is None:
        windows = DEFAULT_WINDOWS
    using_batches = means.dim() != 2
    if not using_batches:
        means = means[None]
        if variances.dim() == 2:
            variances = variances[None]
    if seq_len is not None:
        seq_len = put(seq_len, torch.int64).reshape(-1)
    if not isinstance(gv_variance, torch.Tensor) and not (np.asarray(gv_variance, np.float64) > 0).all():
        raise ValueError('gv_variance must be positive everywhere')
    out = ops.mlpg_gv(means, variances, put(gv_mean, torch.float32), put(gv_variance, torch.float32), windows,
                      padding_size=padding_size, seq_len=seq_len, gv_weight=gv_weight, max_iter=max_iter,
                      out_dtype=torch.float32 if as_tensor else torch.float64)
    if not using_batches:
        out = out.squeeze(0)
    return out if as_tensor else out.cpu().numpy()


# ---- vocoder features (csrc/vocoder.hip): models/RNN_SPSS.py:141-161 up to the call of the synthesiser
# Frequency-warping coefficients of the mel-cepstral analysis by sample rate: the values Merlin's WORLD recipes use.  What a corpus
# was analysed with is its owner's to know - pass ``alpha`` whenever it is known.
MERLIN_ALPHA = {16000: 0.58, 22050: 0.65, 44100: 0.76, 48000: 0.77}


def default_alpha(sample_rate):
    """Merlin's all-pass constant for ``sample_rate`` (``MERLIN_ALPHA``); any other rate raises: there is no formula to guess from."""
    try:
        return MERLIN_ALPHA[int(sample_rate)]
    except KeyError:
        raise ValueError('no default alpha for a sample rate of %r Hz (known: %s): pass the alpha the corpus was analysed with'
                         % (sample_rate, sorted(MERLIN_ALPHA)))


def default_fft_size(sample_rate):
    """WORLD's CheapTrick FFT size for ``sample_rate``: 2 ** ceil(log2(3 fs / 71 + 1)) (f0 floor 71 Hz) - 1024 at 16 kHz, 2048 at 48 kHz."""
    return 2 ** int(np.ceil(np.log2(3. * float(sample_rate) / 71. + 1.)))


def _upload(what, x, dtype, device):
    """(tensor on the device, the inputs' device or None): a device tensor as it is, an array uploaded to the current device."""
    if isinstance(x, torch.Tensor):
        return x.detach().to(dtype=dtype)
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.MorganaHipError('%s runs only on an MI355X device (no CPU fallback)' % what)
        device = torch.device('cuda', torch.cuda.current_device())
    return torch.from_numpy(np.array(x)).to(device=device, dtype=dtype)


def _batched(what, x, seq_len, *more):
    """The padded (B, T, D) form of a feature (a single (T, D) sequence gains the batch axis), its (B,) int64 device lengths, the
    (B + 1,) packed offsets and the rows of the packed output.  ``seq_len`` None: every item is whole, nothing is read; host lengths
    (array, list) are exact without a device read; DEVICE lengths stay on the device and the packed output has B * T rows, of which
    those from ``offsets[-1]`` on are not written."""
    device = _device_of(x, *more)
    tensors = [_upload(what, v, torch.float32, device) for v in (x,) + more]
    tensors = [v[None] if v.dim() == 2 else v for v in tensors]
    if tensors[0].dim() != 3:
        raise ValueError('%s takes (batch_size, seq_len, feat_dim) or (seq_len, feat_dim), got %s' % (what, tuple(tensors[0].shape)))
    b, t = tensors[0].shape[:2]
    dev = tensors[0].device
    if seq_len is None:
        lengths = torch.full((b,), t, dtype=torch.int64, device=dev)
        rows = b * t
    elif isinstance(seq_len, torch.Tensor):
        lengths = seq_len.detach().reshape(-1).to(device=dev, dtype=torch.int64).clamp(0, t)
        rows = b * t
    else:
        host = np.clip(np.asarray(seq_len, dtype=np.int64).reshape(-1), 0, t)
        lengths = torch.from_numpy(host).to(dev)
        rows = int(host.sum())
    if lengths.numel() != b:
        raise ValueError('%s: seq_len holds %d lengths for %d items' % (what, lengths.numel(), b))
    offsets = torch.zeros((b + 1,), dtype=torch.int64, device=dev)
    torch.cumsum(lengths, 0, out=offsets[1:])
    return tensors, lengths, offsets, rows


def mcep_to_spectrum(mcep, alpha, fft_size, seq_len=None, log=False, dtype=torch.float32):
    r"""Mel-cepstrum to power spectrum, the envelope a WORLD-style vocoder takes (``csrc/vocoder.hip``).

    mcep : (batch_size, seq_len, order) or (seq_len, order); alpha : the all-pass constant of the analysis (``default_alpha``);
    fft_size : a power of two (``default_fft_size``); seq_len : (batch_size,) lengths; log : return the log power spectrum;
    dtype : torch.float32 or torch.float64 (the float32 result widened on the device).

    ``sp[t, k] = exp(2 sum_m c[t, m] cos(m w~_k))`` at ``w_k = 2 pi k / fft_size`` warped by the all-pass of ``alpha``: in closed form
    what SPTK's ``freqt(-alpha)`` to order ``fft_size / 2`` followed by a cosine sum gives (agreement 1.5e-14, checked on the host).
    Whether the un-vendored ``tts_data_tools`` the reference calls did exactly that could not be verified: the package is not
    available.  Returns (spectrum, offsets): the PACKED (rows, fft_size / 2 + 1) device tensor - utterance b is rows
    ``offsets[b]:offsets[b + 1]`` - and the (batch_size + 1,) int64 device offsets.  NumPy arrays are uploaded (float32), as ``MLPG``
    does; the results stay on the device.  There is no host implementation: without the HIP library this raises."""
    (mcep,), lengths, offsets, rows = _batched('mcep_to_spectrum', mcep, seq_len)
    return ops.mcep_spectrum(mcep, alpha, fft_size, seq_len=lengths, packed_rows=rows, log=log, out_dtype=dtype), offsets


def bap_to_aperiodicity(bap, sample_rate, fft_size, seq_len=None, dtype=torch.float32):
    r"""Coded band aperiodicity (dB, one column per 3 kHz band: 1 at 16 kHz, 5 at 48 kHz) to the full-band aperiodicity a WORLD-style
    vocoder takes (``csrc/vocoder.hip``): values clamped to [-60, 0] dB, interpolated linearly in dB over frequency between
    (0 Hz, -60 dB), the bands at 3000 i Hz and (sample_rate / 2, 0 dB), then ``10 ** (dB / 20)``.  This is WORLD's
    ``decode_aperiodicity`` as remembered; it could not be checked against ``pyworld``.  Arguments and returns as ``mcep_to_spectrum``."""
    (bap,), lengths, offsets, rows = _batched('bap_to_aperiodicity', bap, seq_len)
    return ops.bap_aperiodicity(bap, int(sample_rate), fft_size, seq_len=lengths, packed_rows=rows, out_dtype=dtype), offsets


def smooth_f0(lf0, vuv, seq_len=None, window=7, threshold=0.5, dtype=torch.float32):
    r"""Log-F0 and voicing to the F0 track a vocoder takes (models/RNN_SPSS.py:154-157): ``exp``, then
    ``scipy.signal.savgol_filter(f0, window, 1)`` per utterance (an utterance shorter than the window is left unsmoothed, where scipy
    raises), then 0 on every frame whose ``vuv`` is not above ``threshold``.  lf0, vuv : (batch_size, seq_len, 1) or (seq_len, 1).
    Returns (f0, offsets): the packed (rows, 1) device tensor and the offsets, as ``mcep_to_spectrum``."""
    (lf0, vuv), lengths, offsets, rows = _batched('smooth_f0', lf0, seq_len, vuv)
    return ops.smooth_f0(lf0, vuv, seq_len=lengths, packed_rows=rows, window=window, threshold=threshold, out_dtype=dtype), offsets


def _world_packed(lf0, vuv, mcep, bap, sample_rate, seq_len, alpha, fft_size, f0_window):
    """``world_features`` up to its packed float64 device tensors -> (f0 (rows,), sp (rows, K), ap (rows, K), host lengths)."""
    alpha = default_alpha(sample_rate) if alpha is None else alpha
    fft_size = default_fft_size(sample_rate) if fft_size is None else fft_size
    if isinstance(seq_len, torch.Tensor):
        seq_len = seq_len.detach().reshape(-1).cpu().numpy()           # the one read of the lengths
    seq_len = np.asarray(seq_len, dtype=np.int64).reshape(-1)
    f0, _ = smooth_f0(lf0, vuv, seq_len, window=f0_window, dtype=torch.float64)
    sp, _ = mcep_to_spectrum(mcep, alpha, fft_size, seq_len, dtype=torch.float64)
    ap, _ = bap_to_aperiodicity(bap, sample_rate, fft_size, seq_len, dtype=torch.float64)
    if f0.shape[1] != 1:
        raise ValueError('world_features: lf0 and vuv must have one column, got %d' % f0.shape[1])
    frames = f0.shape[0]
    if sp.shape[0] != frames or ap.shape[0] != frames:
        raise ValueError('world_features: the features disagree about the frames (%d, %d, %d)' % (frames, sp.shape[0], ap.shape[0]))
    return f0.reshape(-1), sp, ap, seq_len


def world_features(lf0, vuv, mcep, bap, sample_rate, seq_len, alpha=None, fft_size=None, f0_window=7, as_numpy=True):
    r"""The three arrays a WORLD-style synthesiser takes for every utterance of a batch, from what an acoustic model generates.

    lf0, vuv : (batch_size, seq_len, 1); mcep : (batch_size, seq_len, order); bap : (batch_size, seq_len, bands); seq_len : (batch_size,)
    lengths; alpha : None looks the rate up in ``MERLIN_ALPHA`` (Merlin's WORLD values - what the corpus was analysed with is the
    user's to know - and raises for any other rate); fft_size : None is WORLD's CheapTrick size (``default_fft_size``).

    Returns a list of per-utterance ``(f0 (n,), sp (n, fft_size / 2 + 1), ap (n, fft_size / 2 + 1))``: float64, C-contiguous NumPy
    arrays (``pyworld.synthesize`` takes exactly these), or with ``as_numpy=False`` views of the packed float64 device tensors.
    ``seq_len`` is read once and each feature reaches the host in one copy.  The opposite direction - an analyser's ``f0``, ``sp``,
    ``ap`` to ``lf0``, ``vuv``, ``mcep``, ``bap`` - is ``data.world_parameters``."""
    f0, sp, ap, seq_len = _world_packed(lf0, vuv, mcep, bap, sample_rate, seq_len, alpha, fft_size, f0_window)
    if as_numpy:
        f0, sp, ap = f0.cpu().numpy(), sp.cpu().numpy(), ap.cpu().numpy()
    # each item's length as its feature sees it (clamped to that feature's own T): the three agree where the shapes do
    ends = np.cumsum(np.clip(seq_len, 0, lf0.shape[-2]))
    return [(f0[e - n:e], sp[e - n:e], ap[e - n:e]) for e, n in zip(ends, np.clip(seq_len, 0, lf0.shape[-2]))]


def synthesise(f0, sp, ap, sample_rate, frame_period=5.):
    r"""One utterance's waveform from ``f0 (n,)``, ``sp (n, K)`` and ``ap (n, K)`` - ``pyworld.synthesize``'s signature, on the
    device (``ops.world_synthesise``, ``csrc/synth.hip``): arrays are uploaded as float64, tensors are read as they are.  Returns the
    float64 NumPy waveform of ``floor((n - 1) S) + 1`` samples, ``S = sample_rate * frame_period / 1000``.  The noise is drawn anew on
    every call.  This follows WORLD's ``synthesis.cpp`` as remembered (without the mean removal of the noise segment that its newer
    versions have); it could not be checked against ``pyworld``.  There is no host implementation: without the HIP library this raises."""
    device = _device_of(f0, sp, ap)
    f0, sp, ap = [_upload('synthesise', v, v.dtype if isinstance(v, torch.Tensor) else torch.float64, device) for v in (f0, sp, ap)]
    if sp.dim() != 2:
        raise ValueError('synthesise takes one utterance: sp must be (frames, bins), got %s' % (tuple(sp.shape),))
    if sp.dtype not in (torch.float32, torch.float64):
        sp = sp.to(torch.float64)
    if ap.dtype not in (torch.float32, torch.float64):
        ap = ap.to(torch.float64)
    dev = sp.device
    wav, _ = ops.world_synthesise(f0.to(dev), sp, ap.to(dev), sample_rate, frame_period, offsets=[0, sp.shape[0]], out_dtype=torch.float64)
    return wav.cpu().numpy()


def synthesise_batch(lf0, vuv, mcep, bap, sample_rate, seq_len, alpha=None, fft_size=None, f0_window=7, frame_period=5.):
    r"""What an acoustic model generates, to waveforms: ``world_features(as_numpy=False)`` straight into ``ops.world_synthesise``.  The
    float64 ``sp`` and ``ap`` never leave the device; only the waveforms cross to the host.  Arguments as ``world_features`` takes
    them, ``frame_period`` in ms.  Returns the list of per-utterance float32 NumPy waveforms."""
    if isinstance(seq_len, torch.Tensor):
        seq_len = seq_len.detach().reshape(-1).cpu().numpy()           # the one read of the lengths
    seq_len = np.clip(np.asarray(seq_len, dtype=np.int64).reshape(-1), 0, lf0.shape[-2])
    f0, sp, ap, _ = _world_packed(lf0, vuv, mcep, bap, sample_rate, seq_len, alpha, fft_size, f0_window)
    offsets = np.concatenate([[0], np.cumsum(seq_len)])
    wav, _ = ops.world_synthesise(f0, sp, ap, sample_rate, frame_period, offsets=offsets.tolist())
    wav = wav.cpu().numpy()                                          # the one copy out
    ends = np.cumsum(ops.synth_sample_counts(seq_len, ops.synth_samples_per_frame(sample_rate, frame_period)))
    return [wav[e - n:e] for e, n in zip(ends, np.diff(np.concatenate([[0], ends])))]


def synthesise_files(ids, in_dir, out_dir, sample_rate, frame_period=5., alpha=None, fft_size=None, f0_window=7, device='cuda:0',
                     max_batch_bytes=256 << 20, overwrite=False):
    r"""Waveforms for a corpus of generated or analysed features (``scripts/synthesise.py``).  For every id of ``ids`` reads either
    ``in_dir/{f0,sp,ap}/{id}.npy`` (an analyser's arrays, taken when ``in_dir/sp`` exists) or ``in_dir/{lf0,vuv,mcep,bap}/{id}.npy``
    (what ``analysis_for_valid_batch`` writes) and writes ``out_dir/{id}.wav`` through ``viz.io.save_wav``.  Utterances are batched
    up to ``max_batch_bytes`` of float64 spectra on the device.  An output that exists is a FileExistsError before anything is read,
    unless ``overwrite``.  Returns the number of samples written."""
    from . import io
    ids = list(ids)
    targets = [os.path.join(out_dir, name + '.wav') for name in ids]
    existing = [t for t in targets if os.path.exists(t)]
    if existing and not overwrite:
        raise FileExistsError('%d of %d outputs exist (the first: %s): pass overwrite to replace them' % (len(existing), len(ids), existing[0]))
    analysed = os.path.isdir(os.path.join(in_dir, 'sp'))
    kinds = ('f0', 'sp', 'ap') if analysed else ('lf0', 'vuv', 'mcep', 'bap')
    if fft_size is None and not analysed:
        fft_size = default_fft_size(sample_rate)
    os.makedirs(out_dir, exist_ok=True)
    written, batch, batch_bytes = 0, [], 0

    def flush():
        nonlocal written, batch, batch_bytes
        if not batch:
            return
        lengths = [len(item[1][0]) for item in batch]
        if analysed:
            f0 = torch.from_numpy(np.concatenate([np.asarray(item[1][0], np.float64).reshape(-1) for item in batch])).to(device)
            sp, ap = [torch.from_numpy(np.concatenate([item[1][i] for item in batch], axis=0)).to(device) for i in (1, 2)]
            wav, _ = ops.world_synthesise(f0, sp, ap, sample_rate, frame_period, offsets=np.concatenate([[0], np.cumsum(lengths)]).tolist())
            wav = wav.cpu().numpy()
            ends = np.cumsum(ops.synth_sample_counts(lengths, ops.synth_samples_per_frame(sample_rate, frame_period)))
            waves = [wav[lo:hi] for lo, hi in zip(np.concatenate([[0], ends[:-1]]), ends)]
        else:
            padded = []
            for i in range(4):
                width = batch[0][1][i].reshape(lengths[0], -1).shape[1]
                x = np.zeros((len(batch), max(lengths), width), np.float32)
                for b, item in enumerate(batch):
                    x[b, :lengths[b]] = item[1][i].reshape(lengths[b], -1)
                padded.append(torch.from_numpy(x).to(device))
            waves = synthesise_batch(*padded, sample_rate, lengths, alpha=alpha, fft_size=fft_size, f0_window=f0_window,
                                     frame_period=frame_period)
        for (target, _), wav in zip(batch, waves):
            io.save_wav(target, wav, sample_rate)
            written += len(wav)
        batch, batch_bytes = [], 0

    for name, target in zip(ids, targets):
        arrays = [np.load(os.path.join(in_dir, kind, name + '.npy')) for kind in kinds]
        bins = arrays[1].shape[-1] if analysed else fft_size // 2 + 1
        cost = 2 * 8 * len(arrays[0]) * bins
        if batch and (batch_bytes + cost > max_batch_bytes or (analysed and arrays[1].shape[-1] != batch[0][1][1].shape[-1])):
            flush()
        batch.append((target, arrays))
        batch_bytes += cost
    flush()
    return written


def mlpg_trajectory(means, variances, windows=None, padding_size=0, seq_len=None, variance_grad=False):
    r"""``MLPG`` as a differentiable layer (trajectory / minimum-generation-error training; the reference's host MLPG has no gradient).

    means : (batch_size, seq_len, feat_dim) float32 device tensor; variances : (feat_dim,) global, the same shape as ``means`` or
    (batch_size, feat_dim) per item, float32 on the same device - constants: one that requires grad is a ValueError; windows,
    padding_size, seq_len as for ``MLPG``.  Device tensors only, always batched.
    variance_grad : True makes the variances a trained input as well (a stream that predicts its variance): they must be per frame,
    the same shape as ``means`` - expand a global or per-item table, autograd sums the expansion - and the backward returns both
    gradients from one pair of side-by-side solves (``functional.MLPGVarFn``).  The forward is the same launch either way.

    Returns the most probable trajectory (batch_size, seq_len, feat_dim // len(windows)), float32, zero past ``seq_len``, with a
    gradient for ``means``: one more banded solve with the forward's matrix and a window pass (``csrc/mlpg.hip``).
    """
    for name, value in (('means', means), ('variances', variances)):
        if not isinstance(value, torch.Tensor):
            raise TypeError('mlpg_trajectory takes device tensors; %s is %s (MLPG takes arrays)' % (name, type(value)))
    if variances.requires_grad and not variance_grad:
        raise ValueError('mlpg_trajectory has no gradient for its variances (they are normaliser constants): detach them, or pass '
                         'variance_grad=True with per-frame variances to train them')
    if variance_grad and variances.shape != means.shape:
        raise ValueError('mlpg_trajectory(variance_grad=True) takes per-frame variances shaped like the means %s, got %s: expand them to '
                         '(B, T, W*D) so that autograd sums the expansion' % (tuple(means.shape), tuple(variances.shape)))
    if windows is None:
        windows = DEFAULT_WINDOWS
    if seq_len is not None:
        if not isinstance(seq_len, torch.Tensor):
            raise TypeError('mlpg_trajectory takes device tensors; seq_len is %s' % type(seq_len))
        seq_len = seq_len.reshape(-1).to(device=means.device, dtype=torch.int64)
    if variance_grad:
        return functional.MLPGVarFn.apply(means, variances, windows, padding_size, seq_len)
    return functional.MLPGFn.apply(means, variances, windows, padding_size, seq_len)
