"""K33 without a GPU: tests/analysis_ref64.py against identities that do not share its code (the plain cepstrum, the left inverse of
K32's basis, the decoder of K32), the host-built table against it, the argument checks of the two entry points through the C ABI and
the defaults of the host layer."""
import numpy as np
import pytest
import torch

import analysis_ref64 as ref
import vocoder_ref64 as voc
from helpers import OFF, OUT, SEQ, TAB, X, abi_caller as _caller
from morgana_amd import _lib, data, ops

IDENTITY_SETTINGS = ((60, 0.77, 2048), (25, 0.58, 1024), (60, 0.58, 1024), (40, 0.42, 512))
ALIASING_SETTINGS = ((128, 0.77, 2048), (5, 0.58, 16))


def _log_spectra(frames, fft_size, seed):
    return np.random.RandomState(seed).uniform(-10.0, 2.5, size=(frames, fft_size // 2 + 1))


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('order,fft_size', [(1, 8), (5, 16), (33, 64), (60, 512)])
def test_restatement_without_warping_is_the_one_sided_cepstrum(order, fft_size):
    """alpha = 0: freqt copies, so c_m = g_m - the cosine-series coefficients of l, which give l back on the grid."""
    l = _log_spectra(4, fft_size, order)
    half = fft_size // 2
    full = ref.mcep_of_half_log(l, half + 1, 0.0, fft_size)
    n = np.arange(half + 1)
    cosines = np.cos(2 * np.pi * np.outer(n, n) / fft_size)              # [n, k]
    np.testing.assert_allclose(full @ cosines, l, rtol=0, atol=1e-12 * np.abs(l).max())
    # a direct sum for g_n, written out from the header
    kappa = np.where((n == 0) | (n == half), 1.0, 2.0)
    weight = np.where((n == 0) | (n == half), 1.0, 2.0)
    direct = (kappa[None, :] / fft_size) * ((l * weight[None, :]) @ cosines.T)
    np.testing.assert_allclose(full, direct, rtol=0, atol=1e-13 * np.abs(l).max())
    np.testing.assert_array_equal(ref.mcep_of_half_log(l, order, 0.0, fft_size), full[:, :order])


@pytest.mark.parametrize('order,alpha,fft_size', IDENTITY_SETTINGS)
def test_table_is_the_left_inverse_of_the_synthesis_basis(order, alpha, fft_size):
    table = ops.mcep_analysis_table(order, alpha, fft_size)
    assert table.dtype == np.float64 and table.shape == (order, fft_size // 2 + 1)
    worst = np.abs(table @ voc.basis(order, alpha, fft_size).T - np.eye(order)).max()
    print('(%d, %g, %d): max |table . basis^T - I| = %.2e' % (order, alpha, fft_size, worst))
    assert worst <= 1e-13
    assert 1.2 < np.abs(table).sum(axis=1).max() < 1.4


@pytest.mark.parametrize('order,alpha,fft_size', IDENTITY_SETTINGS + ALIASING_SETTINGS + ((1, 0.0, 8), (3, 0.42, 8), (61, 0.58, 1024),
                                                                                         (128, 0.3, 64)))
def test_table_agrees_with_the_two_step_route(order, alpha, fft_size):
    l = _log_spectra(5, fft_size, 7 * order + fft_size)
    want = ref.mcep_of_half_log(l, order, alpha, fft_size)
    got = l @ ops.mcep_analysis_table(order, alpha, fft_size).T
    worst = np.abs(got - want).max() / np.abs(want).max()
    print('(%d, %g, %d): table against irfft + freqt, relative to max |c| = %.2e' % (order, alpha, fft_size, worst))
    assert worst <= 1e-13


@pytest.mark.parametrize('order,alpha,fft_size', ALIASING_SETTINGS)
def test_aliasing_settings_are_not_identities(order, alpha, fft_size):
    """Where the warped series does not fit F / 2 + 1 terms the truncated transform is no left inverse: a property, not an error."""
    table = ops.mcep_analysis_table(order, alpha, fft_size)
    worst = np.abs(table @ voc.basis(order, alpha, fft_size).T - np.eye(order)).max()
    assert worst > 1e-4


def test_table_arguments():
    for bad in (0, 129, 2.0, True):
        with pytest.raises(ValueError):
            ops.mcep_analysis_table(bad, 0.5, 64)
    for bad in (0, 12, 4, 16384, 64.0):
        with pytest.raises(ValueError):
            ops.mcep_analysis_table(4, 0.5, bad)
    for bad in (1.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            ops.mcep_analysis_table(4, bad, 64)


@pytest.mark.parametrize('sample_rate,fft_size,bands', [(16000, 1024, 1), (48000, 2048, 5), (48000, 2048, 7)])
def test_aperiodicity_restatement_inverts_the_decoder_on_anchor_bins(sample_rate, fft_size, bands):
    rng = np.random.RandomState(bands)
    bap = rng.uniform(-59.0, -0.5, size=(6, bands))
    bap[0] = -60.0
    bap[1] = 0.0
    ap = voc.aperiodicity(bap, sample_rate, fft_size)
    back = ref.band_aperiodicity(ap, sample_rate, bands, fft_size)
    worst = np.abs(back - bap).max()
    print('%d Hz / %d / %d bands: round trip %.2e dB' % (sample_rate, fft_size, bands, worst))
    assert worst <= 1e-12


def test_aperiodicity_restatement_edges():
    ap = np.full((5, 513), 0.5)
    ap[0, 192] = 0.0
    ap[1, 192] = 1.5
    ap[2, 192] = 1e-4
    ap[3, 192] = np.nan
    ap[4, 192] = -0.5
    got = ref.band_aperiodicity(ap, 16000, 1, 1024)[:, 0]             # 3000 Hz is bin 192 exactly
    assert got[0] == -60.0 and got[1] == 0.0 and got[2] == -60.0 and np.isnan(got[3]) and np.isnan(got[4])
    off = ref.band_aperiodicity(np.full((1, 1025), 0.1), 44100, 5, 2048)
    np.testing.assert_allclose(off, -20.0, rtol=0, atol=1e-12)


# ----------------------------------------------------------------------------------------------------------------------- the defaults
def test_band_and_alpha_defaults():
    assert [ops.default_n_bands(r) for r in (16000, 22050, 44100, 48000)] == [1, 2, 5, 5]
    assert ops.default_n_bands(32000) == 4 and ops.default_n_bands(96000) == 5
    for bad in (6000, 8000, 0, 16000.0, True):
        with pytest.raises(ValueError):
            ops.default_n_bands(bad)
    sp = np.ones((3, 513))
    with pytest.raises(ValueError, match='24000'):                     # no alpha for the rate: refused before a device is looked for
        data.world_parameters(np.zeros(3), sp, sp, 24000)


def test_host_layer_without_a_device_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # the machine that runs this may have one
    sp = np.ones((3, 513))
    with pytest.raises(_lib.MorganaHipError):
        data.world_parameters(np.full(3, 120.0), sp, sp, 16000)
    with pytest.raises(_lib.MorganaHipError):
        data.spectrum_to_mcep(sp, 25, 0.58)
    with pytest.raises(_lib.MorganaHipError):
        data.aperiodicity_to_bap(sp, 16000)
    with pytest.raises(_lib.MorganaHipError):
        data.extract_world_features(['a'], '.', '.', 16000)


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    with pytest.raises(_lib.MorganaHipError):
        ops.spectrum_mcep(torch.ones(2, 3, 5, dtype=torch.float64), 3, 0.42, seq_len=torch.tensor([3, 2]))
    with pytest.raises(_lib.MorganaHipError):
        ops.aperiodicity_bap(torch.ones(5, 513), 16000, offsets=torch.tensor([0, 5]))
    with pytest.raises(_lib.MorganaHipError):                   # a host TENSOR is refused as such, with or without a device
        data.spectrum_to_mcep(torch.ones(3, 513), 25, 0.58)
    with pytest.raises(TypeError):
        ops.spectrum_mcep(np.ones((2, 5)), 3, 0.42, offsets=np.zeros(2))


# ------------------------------------------------------------------------------------------------------------------------- the C ABI
# The addresses X, OFF, SEQ, OUT and TAB are fake: every call below must be one that is refused on the host, or has nothing to do.
INT64_MAX = 2 ** 63 - 1


def test_tile_and_signatures():
    lib = _lib.load()
    assert lib.mg_analysis_tile_frames() >= 16 and lib.mg_analysis_tile_frames() % 16 == 0
    for name in ('mg_spectrum_mcep', 'mg_aperiodicity_bap'):
        assert name in _lib.SIGNATURES


def test_mcep_entry_point_refuses_bad_arguments_without_a_gpu():
    names = ('sp', 'in_f64', 'log_in', 'F', 'B', 'offsets', 'seq_len', 'T_in', 'table', 'ldt', 'M', 'out_f64', 'packed_rows', 'out', 'stream')
    ok = (X, 1, 0, 2048, 3, OFF, None, 0, TAB, 1025, 60, 0, 30, OUT, None)
    call, refused = _caller('mg_spectrum_mcep', names, ok)
    for f in (0, 4, 12, 1000, 2047, 16384, -8):
        assert refused('F=%d' % f, F=f, ldt=1 << 20)
    assert refused('M=0', M=0) and refused('M=129', M=129) and refused('M=-1', M=-1)
    assert refused('ldt=1024', ldt=1024)
    assert refused('exactly one of', offsets=None) and refused('exactly one of', seq_len=SEQ)
    assert refused('out must not be NULL', out=None)
    assert refused('B=-1', B=-1)
    assert refused('T_in=-1', offsets=None, seq_len=SEQ, T_in=-1)
    assert refused('at most', offsets=None, seq_len=SEQ, T_in=4, B=_lib.MG_VOC_MAX_ITEMS + 1)
    assert refused('packed_rows=-1', packed_rows=-1)
    assert refused('input must not be NULL', sp=None)
    assert refused('table', table=None) and refused('table', table=TAB + 4)
    assert refused('aligned', sp=X + 4) and refused('aligned', sp=X + 2, in_f64=0)
    assert refused('aligned', out=OUT + 2) and refused('aligned', out=OUT + 4, out_f64=1) and refused('aligned', offsets=OFF + 4)
    assert call(B=0) == 0 and call(B=0, sp=None, table=None) == 0 and call(packed_rows=0) == 0      # nothing to do: no launch


def test_bap_entry_point_refuses_bad_arguments_without_a_gpu():
    names = ('ap', 'in_f64', 'F', 'fs', 'Nb', 'B', 'offsets', 'seq_len', 'T_in', 'out_f64', 'packed_rows', 'out', 'stream')
    ok = (X, 0, 2048, 48000, 5, 3, OFF, None, 0, 0, 30, OUT, None)
    call, refused = _caller('mg_aperiodicity_bap', names, ok)
    assert refused('F=1000', F=1000) and refused('F=4', F=4)
    assert refused('Nb=8', Nb=8)                               # 24000 Hz is fs / 2 itself
    assert refused('Nb=3', Nb=3, fs=16000) and refused('Nb=0', Nb=0) and refused('Nb=1', Nb=1, fs=6000) and refused('Nb=-2', Nb=-2)
    assert refused('fs=0', fs=0)
    assert refused('exactly one of', offsets=None) and refused('exactly one of', seq_len=SEQ)
    assert refused('out must not be NULL', out=None)
    assert refused('B=-1', B=-1) and refused('packed_rows=-1', packed_rows=-1)
    assert refused('T_in=-1', offsets=None, seq_len=SEQ, T_in=-1)
    assert refused('input must not be NULL', ap=None)
    assert refused('aligned', ap=X + 1) and refused('aligned', ap=X + 4, in_f64=1) and refused('aligned', out=OUT + 4, out_f64=1)
    assert call(B=0) == 0 and call(Nb=7, B=0) == 0 and call(Nb=2, fs=16000, B=0) == 0 and call(packed_rows=0) == 0


def test_packed_rows_overflow_guard_refuses_its_first_value_without_a_gpu():
    """The byte count packed_rows x max(width, cols) must fit 64 bits.  Only the refused side of the guard is called: the value below
    it would launch.  (The guard on B x T_in x width cannot be reached here: T_in is an int, and at most MG_VOC_MAX_ITEMS = 4096 items
    of at most 4097 bins leave it 2^37 frames.)"""
    names = ('sp', 'in_f64', 'log_in', 'F', 'B', 'offsets', 'seq_len', 'T_in', 'table', 'ldt', 'M', 'out_f64', 'packed_rows', 'out', 'stream')
    ok = (X, 1, 0, 8, 3, OFF, None, 0, TAB, 5, 2, 0, 30, OUT, None)
    _, refused = _caller('mg_spectrum_mcep', names, ok)
    assert refused('packed_rows=', packed_rows=INT64_MAX // 8 // max(5, 2) + 1)
    assert INT64_MAX // 4 // 4097 // _lib.MG_VOC_MAX_ITEMS + 1 >= 2 ** 31
