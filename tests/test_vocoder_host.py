"""K32 without a GPU: tests/vocoder_ref64.py against identities that do not share its code (an FFT, the first-order closed form, the
values at 0 and at the Nyquist bin, scipy's savgol_filter, exact anchor bins), the host-built basis table against it, the argument
checks of the three entry points through the C ABI, the defaults of viz.synthesis and viz.io.save_wav."""
import wave

import numpy as np
import pytest
import torch

import vocoder_ref64 as ref
from helpers import OFF, OUT, SEQ, TAB, X, abi_caller as _caller
from morgana_amd import _lib, ops, viz

SETTINGS = ((1, 8, 0.0), (2, 8, 0.42), (25, 512, 0.42), (60, 2048, 0.77), (61, 1024, 0.58), (128, 64, 0.3))


def _cepstra(order, frames, seed):
    rng = np.random.RandomState(seed)
    c = rng.randn(frames, order) / np.maximum(np.arange(order), 1)[None, :]
    c[:, 0] = rng.uniform(-4, 4, size=frames)
    return c


# ------------------------------------------------------------------------------------------------------------ the spectrum's reference
@pytest.mark.parametrize('order,fft_size', [(s[0], s[1]) for s in SETTINGS if s[0] <= s[1]] + [(33, 64)])
def test_log_spectrum_without_warping_is_the_real_fft(order, fft_size):
    """alpha = 0: L = Re(rfft(c, F)).  (Orders above F are left out: rfft crops its input there, the cosine sum wraps around.)"""
    c = _cepstra(order, 5, order)
    want = np.fft.rfft(c, fft_size, axis=1).real
    np.testing.assert_allclose(ref.log_spectrum(c, 0.0, fft_size), want, rtol=0, atol=1e-12 * np.abs(c).sum(axis=1).max())


@pytest.mark.parametrize('alpha', [0.0, 0.3, 0.58, 0.77])
def test_first_order_closed_form(alpha):
    """Only c_1 set: cos(w~) = ((1 + a^2) cos w - 2 a) / (1 + a^2 - 2 a cos w) of the first-order all-pass."""
    fft_size = 512
    c = np.zeros((1, 4))
    c[0, 1] = 1.7
    w = 2 * np.pi * np.arange(fft_size // 2 + 1) / fft_size
    want = 1.7 * ((1 + alpha ** 2) * np.cos(w) - 2 * alpha) / (1 + alpha ** 2 - 2 * alpha * np.cos(w))
    np.testing.assert_allclose(ref.log_spectrum(c, alpha, fft_size)[0], want, rtol=0, atol=1e-13)


@pytest.mark.parametrize('order,fft_size,alpha', SETTINGS)
def test_log_spectrum_at_zero_and_nyquist(order, fft_size, alpha):
    c = _cepstra(order, 4, 100 + order)
    L = ref.log_spectrum(c, alpha, fft_size)
    scale = np.abs(c).sum(axis=1)
    assert np.all(np.abs(L[:, 0] - c.sum(axis=1)) <= 1e-13 * scale)
    signs = (-1.0) ** np.arange(order)
    assert np.all(np.abs(L[:, -1] - (c * signs).sum(axis=1)) <= 1e-12 * scale * order)


@pytest.mark.parametrize('order,fft_size,alpha', SETTINGS)
def test_host_basis_table_is_the_reference_rounded_once(order, fft_size, alpha):
    table = ops.mcep_basis_table(order, alpha, fft_size)
    assert table.dtype == np.float32 and table.shape == (order, fft_size // 2 + 1)
    want = ref.basis(order, alpha, fft_size)
    # atan2 against atan of the quotient, and m w~ up to 128 pi: a few float64 ulps of the argument, far below float32's half ulp
    assert np.max(np.abs(table.astype(np.float64) - want)) <= 2.0 ** -24 + 1e-12


def test_basis_table_arguments():
    for bad in (0, 129, 2.0, True):
        with pytest.raises(ValueError):
            ops.mcep_basis_table(bad, 0.5, 64)
    for bad in (0, 12, 4, 16384, 64.0):
        with pytest.raises(ValueError):
            ops.mcep_basis_table(4, 0.5, bad)
    for bad in (1.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            ops.mcep_basis_table(4, bad, 64)


# --------------------------------------------------------------------------------------------------------- smoothing and aperiodicity
@pytest.mark.parametrize('window', [3, 5, 7, 11])
@pytest.mark.parametrize('extra', [0, 1, 4, 33])
def test_smoothing_against_scipy(extra, window):
    signal = pytest.importorskip('scipy.signal')
    n = window + extra                                           # scipy raises below the window
    y = np.exp(np.random.RandomState(n * window).uniform(4.0, 6.0, size=n))
    want = signal.savgol_filter(y, window, 1)
    np.testing.assert_allclose(ref.smooth(y, window), want, rtol=1e-13, atol=0)


def test_smoothing_short_items_and_window_one():
    y = np.array([100.0, 180.0, 90.0])
    np.testing.assert_array_equal(ref.smooth(y, 7), y)
    np.testing.assert_array_equal(ref.smooth(y, 1), y)
    np.testing.assert_array_equal(ref.smooth(np.zeros(0), 3), np.zeros(0))
    lf0 = np.log(y).astype(np.float32)[:, None]
    vuv = np.array([[1.0], [0.5], [0.51]], dtype=np.float32)
    got = ref.smooth_f0(lf0, vuv, 7)
    assert got[1, 0] == 0.0 and got[0, 0] == np.exp(np.float64(lf0[0, 0])) and got[2, 0] > 0


def test_aperiodicity_at_exact_anchors():
    """fs 48000, F 2048: bin 128 i is exactly 3000 i Hz and returns the clamped coded value; bin 0 is -60 dB, the last 0 dB."""
    bap = np.array([[-3.0, -70.0, 2.5, -0.0, -59.5], [-10.0, -20.0, -30.0, -40.0, -50.0]])
    ap = ref.aperiodicity(bap, 48000, 2048)
    clamped = np.clip(bap, -60.0, 0.0)
    for i in range(1, 6):
        np.testing.assert_allclose(ap[:, 128 * i], 10.0 ** (clamped[:, i - 1] / 20.0), rtol=1e-14)
    np.testing.assert_allclose(ap[:, 0], 1e-3, rtol=1e-14)
    np.testing.assert_allclose(ap[:, -1], 1.0, rtol=1e-14)
    mid = 10.0 ** ((clamped[:, 0] + clamped[:, 1]) / 2.0 / 20.0)               # bin 192 = 4500 Hz: half way in dB
    np.testing.assert_allclose(ap[:, 192], mid, rtol=1e-14)
    assert np.all(ap <= 1.0) and np.all(ap >= 1e-3 * (1 - 1e-14))


# ------------------------------------------------------------------------------------------------------------------------- the C ABI
# The addresses X, OFF, SEQ, OUT and TAB are fake: every call below must be one that is refused on the host, or has nothing to do.
INT64_MAX = 2 ** 63 - 1


def test_limits_and_tiles():
    lib = _lib.load()
    assert (_lib.MG_VOC_MAX_ORDER, _lib.MG_VOC_MAX_WINDOW) == (128, 65) and _lib.MG_VOC_MAX_ITEMS >= 1024
    assert lib.mg_vocoder_tile_frames() >= 1 and lib.mg_vocoder_tile_bins() % 64 == 0 and lib.mg_smooth_f0_chunk_rows() >= 65
    for name in ('mg_mcep_spectrum_f32', 'mg_bap_aperiodicity_f32', 'mg_smooth_f0_f32'):
        assert name in _lib.SIGNATURES


def test_spectrum_entry_point_refuses_bad_arguments_without_a_gpu():
    names = ('mcep', 'M', 'B', 'offsets', 'seq_len', 'T_in', 'basis', 'ldb', 'F', 'log_out', 'out_f64', 'packed_rows', 'out', 'stream')
    ok = (X, 60, 3, OFF, None, 0, TAB, 1025, 2048, 0, 0, 30, OUT, None)
    call, refused = _caller('mg_mcep_spectrum_f32', names, ok)
    for f in (0, 4, 12, 1000, 2047, 16384, -8):
        assert refused('power of two', F=f, ldb=1 << 20)
    assert refused('M=0', M=0) and refused('M=129', M=129) and refused('M=-1', M=-1)
    assert refused('ldb', ldb=1024)
    assert refused('exactly one of', offsets=None) and refused('exactly one of', seq_len=SEQ)
    assert refused('out must not be NULL', out=None)
    assert refused('B=-1', B=-1)
    assert refused('T_in=-1', offsets=None, seq_len=SEQ, T_in=-1)
    assert refused('at most', offsets=None, seq_len=SEQ, T_in=4, B=_lib.MG_VOC_MAX_ITEMS + 1)
    assert refused('packed_rows=-1', packed_rows=-1)
    assert refused('input must not be NULL', mcep=None)
    assert refused('basis', basis=None) and refused('basis', basis=TAB + 2)
    assert refused('aligned', mcep=X + 2) and refused('aligned', out=OUT + 2) and refused('aligned', offsets=OFF + 4)
    assert refused('aligned', out=OUT + 4, out_f64=1)
    assert call(B=0) == 0 and call(B=0, mcep=None, basis=None) == 0 and call(packed_rows=0) == 0      # nothing to do: no launch


def test_aperiodicity_entry_point_refuses_bad_arguments_without_a_gpu():
    names = ('bap', 'Nb', 'B', 'offsets', 'seq_len', 'T_in', 'fs', 'F', 'out_f64', 'packed_rows', 'out', 'stream')
    ok = (X, 5, 3, OFF, None, 0, 48000, 2048, 0, 30, OUT, None)
    call, refused = _caller('mg_bap_aperiodicity_f32', names, ok)
    assert refused('power of two', F=1000) and refused('power of two', F=4)
    assert refused('Nb=8', Nb=8)                               # 24000 Hz is fs / 2 itself
    assert refused('Nb=3', Nb=3, fs=16000) and refused('Nb=0', Nb=0) and refused('Nb=1', Nb=1, fs=6000)
    assert refused('fs=0', fs=0)
    assert refused('exactly one of', offsets=None) and refused('exactly one of', seq_len=SEQ)
    assert refused('out must not be NULL', out=None)
    assert refused('input must not be NULL', bap=None)
    assert refused('aligned', bap=X + 1)
    assert call(B=0) == 0 and call(Nb=7, B=0) == 0 and call(Nb=2, fs=16000, B=0) == 0


def test_smoothing_entry_point_refuses_bad_arguments_without_a_gpu():
    names = ('lf0', 'vuv', 'D', 'B', 'offsets', 'seq_len', 'T_in', 'window', 'threshold', 'out_f64', 'packed_rows', 'out', 'stream')
    ok = (X, TAB, 1, 3, OFF, None, 0, 7, 0.5, 0, 30, OUT, None)
    call, refused = _caller('mg_smooth_f0_f32', names, ok)
    for window in (0, 2, 6, 66, 67, -1):
        assert refused('window=%d' % window, window=window)
    assert refused('D=0', D=0)
    assert refused('NaN', threshold=float('nan'))
    assert refused('exactly one of', offsets=None) and refused('exactly one of', seq_len=SEQ)
    assert refused('out must not be NULL', out=None)
    assert refused('input must not be NULL', lf0=None) and refused('vuv', vuv=None)
    assert call(B=0) == 0 and call(B=0, window=1) == 0 and call(B=0, window=65) == 0


def test_overflow_guards_refuse_their_first_value_without_a_gpu():
    """The byte counts packed_rows x max(width, cols) and B x T_in x width must fit 64 bits.  Only the refused side of either guard is
    called: the value below it would launch."""
    names = ('mcep', 'M', 'B', 'offsets', 'seq_len', 'T_in', 'basis', 'ldb', 'F', 'log_out', 'out_f64', 'packed_rows', 'out', 'stream')
    ok = (X, 2, 3, OFF, None, 0, TAB, 5, 8, 0, 0, 30, OUT, None)
    _, refused = _caller('mg_mcep_spectrum_f32', names, ok)
    assert refused('packed_rows=', packed_rows=INT64_MAX // 8 // max(2, 5) + 1)
    # T_in is an int: only a wide row brings the guard into its range
    names = ('lf0', 'vuv', 'D', 'B', 'offsets', 'seq_len', 'T_in', 'window', 'threshold', 'out_f64', 'packed_rows', 'out', 'stream')
    width, items = 2 ** 31 - 1, 1
    ok = (X, TAB, width, items, None, SEQ, 4, 7, 0.5, 0, 1, OUT, None)
    _, refused = _caller('mg_smooth_f0_f32', names, ok)
    t_in = INT64_MAX // 4 // width // items + 1
    assert t_in < 2 ** 31
    assert refused('overflow 64 bits', T_in=t_in)


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    with pytest.raises(_lib.MorganaHipError):
        ops.mcep_spectrum(torch.zeros(2, 3, 4), 0.42, 64, seq_len=torch.tensor([3, 2]))
    with pytest.raises(_lib.MorganaHipError):
        ops.bap_aperiodicity(torch.zeros(5, 1), 16000, 1024, offsets=torch.tensor([0, 5]))
    with pytest.raises(_lib.MorganaHipError):
        ops.smooth_f0(torch.zeros(5, 1), torch.zeros(5, 1), offsets=torch.tensor([0, 5]))
    with pytest.raises(TypeError):
        ops.mcep_spectrum(np.zeros((2, 3)), 0.42, 64, offsets=np.zeros(2))
    with pytest.raises(ValueError):
        ops.spectrum_bins(48)
    with pytest.raises(_lib.MorganaHipError):               # no host implementation behind the reference-style functions either
        viz.synthesis.mcep_to_spectrum(torch.zeros(1, 3, 4), 0.42, 64)


# ----------------------------------------------------------------------------------------------------------------------- the defaults
def test_fft_size_and_alpha_defaults():
    assert viz.synthesis.default_fft_size(16000) == 1024 and viz.synthesis.default_fft_size(48000) == 2048
    assert viz.synthesis.default_fft_size(22050) == 1024 and viz.synthesis.default_fft_size(44100) == 2048
    assert viz.synthesis.default_fft_size(8000) == 512
    assert [viz.synthesis.default_alpha(r) for r in (16000, 22050, 44100, 48000)] == [0.58, 0.65, 0.76, 0.77]
    for rate in (8000, 24000, 32000):
        with pytest.raises(ValueError):
            viz.synthesis.default_alpha(rate)


def test_save_wav_round_trip(tmp_path):
    path = str(tmp_path / 'a.wav')
    wav = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -3.0, np.nan])
    viz.io.save_wav(path, wav, 22050)
    with wave.open(path, 'rb') as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 22050, 8)
        pcm = np.frombuffer(f.readframes(8), dtype='<i2')
    np.testing.assert_array_equal(pcm, [0, 16384, -16384, 32767, -32767, 32767, -32768, 0])
    viz.io.save_wav(path, np.array([1, -2, 40000], dtype=np.int64), 16000)
    with wave.open(path, 'rb') as f:
        np.testing.assert_array_equal(np.frombuffer(f.readframes(3), dtype='<i2'), [1, -2, 32767])
    with pytest.raises(ValueError):
        viz.io.save_wav(path, np.zeros((4, 2)), 16000)
