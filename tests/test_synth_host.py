"""CPU-only: tests/synth_ref64.py held to the identities of its own definition (K34, include/morgana_hip.h), and the host side of
ops.world_synthesise - argument checks, lengths and the pulse-range plan - without a device."""
import ctypes
import math

import numpy as np
import pytest
import torch

import synth_ref64 as ref
from morgana_amd import _lib, ops

FS, PERIOD, F = 16000, 5., 1024
K = F // 2 + 1


def _formant(centre_hz=700., width_hz=150., level=1e-5):
    freq = np.arange(K) * FS / float(F)
    return level * (.2 + 4. / (1. + ((freq - centre_hz) / width_hz) ** 2))


def _full_mean(p):
    """The mean of a one-sided spectrum over all F bins of the transform."""
    return (2. * p.sum() - p[0] - p[-1]) / F


def test_minimum_phase_keeps_the_power_spectrum():
    for p in (_formant(), _formant(2500., 400., 3e-3), np.full(K, 2e-7)):
        h, _ = ref.minphase(p, F)
        assert np.max(np.abs(np.abs(h) ** 2 / p - 1.)) <= 1e-12
    h, _ = ref.minphase(_formant(), F)
    c = np.fft.irfft(np.log(h), F)                       # minimum phase: the complex cepstrum is causal
    assert np.max(np.abs(c[F // 2 + 1:])) <= 1e-12


def test_length_formula():
    for fs, period in ((16000, 5.), (22050, 5.), (8000, 10.)):
        s = ref.samples_per_frame(fs, period)
        assert [ref.n_samples(n, s) for n in (0, 1, 2)] == [0, 1, int(math.floor(s)) + 1]
        assert ops.synth_sample_counts([0, 1, 2, 41], ops.synth_samples_per_frame(fs, period)) == [ref.n_samples(n, s) for n in (0, 1, 2, 41)]
    assert ref.samples_per_frame(22050, 5.) == 110.25
    for n in (0, 1):                                     # no pulse, N zeros
        y = ref.synthesise(np.full(n, 100.), np.ones((n, K)), np.ones((n, K)), FS, PERIOD, np.ones(n))
        assert y.shape == (n,) and not y.any()


@pytest.mark.parametrize('f0', [125., 250., 500., 1000.])
def test_constant_dyadic_f0_gives_the_exact_period(f0):
    index, delta, period, voiced = ref.pulses(np.full(50, f0), FS, PERIOD, F)
    assert voiced.all() and not delta.any()              # 2^32 f0 / fs is an integer: every crossing falls on a sample
    assert np.all(np.diff(index) == FS / f0) and np.all(period[:-1] == FS / f0)
    assert index[0] == FS / f0 - 1 and period[-1] == ref.n_samples(50, 80.) - index[-1]


def test_unvoiced_pulses_and_the_clamps():
    index, _, period, voiced = ref.pulses(np.zeros(50), FS, PERIOD, F)
    assert not voiced.any() and np.all(period[:-1] == 32)                     # 500 Hz at 16 kHz
    f, v = ref.sample_f0(np.array([9000., 9000., 3., 3., 0., 100.]), FS, PERIOD, F)
    assert f[0] == FS / 2 and f[2 * 80 + 1] == FS / float(F) and f[4 * 80] == 500. and not v[4 * 80]
    assert v[4 * 80 - 41] and not v[4 * 80 - 39] and not v[4 * 80 - 40]        # w < .5, w > .5, and the tie takes both frames
    index, _, period, _ = ref.pulses(np.full(60, 1.), FS, PERIOD, F)         # held at fs / F: the period is F, never more
    assert np.all(period <= F) and np.all(period[:-1] == F)


def test_unvoiced_power_is_the_mean_of_the_envelope():
    n = 400
    p = _formant()
    total = ref.n_samples(n, 80.)
    y = ref.synthesise(np.zeros(n), np.tile(p, (n, 1)), np.full((n, K), .5), FS, PERIOD, np.random.RandomState(1).randn(total))
    y = y[F:-F]                                          # away from the ends, where responses are cut off
    # the noise shaped by G is a stationary Gaussian process of spectrum P: its power is the mean of P over the transform's bins, and
    # the mean of N squares of it has variance (2 / N) r(0)^2 sum_t rho(t)^2 with sum_t rho^2 = F sum P^2 / (sum P)^2 (Parseval)
    full = np.concatenate([p, p[-2:0:-1]])
    sigma = math.sqrt(2. * F * np.sum(full ** 2) / np.sum(full) ** 2 / len(y))
    assert abs(np.mean(y ** 2) / _full_mean(p) - 1.) <= 5. * sigma and sigma < .05


def test_voiced_power_is_the_mean_of_the_envelope():
    n, f0, a, level = 400, 250., .6, 3e-5                # a flat envelope: its mean is its value at the harmonics too
    period, r = FS / f0, a * a
    total = ref.n_samples(n, 80.)
    y = ref.synthesise(np.full(n, f0), np.full((n, K), level), np.full((n, K), a), FS, PERIOD, np.random.RandomState(2).randn(total))
    y = y[F:-F]
    # periodic part: impulses of height sqrt(T P (1 - r)) every T samples less their mean (step 6 removes the DC harmonic, 1 / T of
    # the power); noise part: white, power P r; the cross term has mean 0
    p_periodic, p_noise = level * (1. - r) * (1. - 1. / period), level * r
    sigma = math.sqrt((2. * p_noise ** 2 + 4. * p_periodic * p_noise) / len(y))
    assert abs(np.mean(y ** 2) - (p_periodic + p_noise)) <= 5. * sigma and sigma < .02 * level
    spectrum = np.abs(np.fft.rfft(y[:int(period) * 256])) ** 2
    harmonics = spectrum[256::256]
    assert np.all(harmonics > 100. * np.median(spectrum))  # a line at every multiple of f0


def test_a_nan_frame_reaches_only_the_responses_that_read_it():
    n = 60
    rng = np.random.RandomState(3)
    f0 = np.where(np.arange(n) < 30, 200., 0.)
    sp, ap = np.tile(_formant(), (n, 1)), np.full((n, K), .4)
    noise = rng.randn(ref.n_samples(n, 80.))
    clean, (index, delta, _, _) = ref.synthesise(f0, sp, ap, FS, PERIOD, noise, want_pulses=True)
    for field, frame in (('sp', 12), ('ap', 12), ('sp', 45), ('ap', 45)):          # a voiced and an unvoiced frame
        dirty_sp, dirty_ap = sp.copy(), ap.copy()
        (dirty_sp if field == 'sp' else dirty_ap)[frame, 100] = np.nan
        dirty = ref.synthesise(f0, dirty_sp, dirty_ap, FS, PERIOD, noise)
        touched = np.zeros(len(clean), bool)
        for i_m, d_m in zip(index, delta):
            j = min(int(math.floor(min(max((i_m - d_m) / 80., 0.), n - 1.))), n - 1)
            if frame in (j, min(j + 1, n - 1)):
                touched[max(i_m - F // 2 + 1, 0):i_m + F // 2 + 1] = True
        assert touched.any() and not touched.all()
        assert np.isnan(dirty[touched]).all()
        assert np.array_equal(dirty[~touched].view(np.int64), clean[~touched].view(np.int64))


def test_the_bound_is_small_against_the_signal():
    n = 30
    noise = np.random.RandomState(4).randn(ref.n_samples(n, 80.))
    y, bound = ref.synthesise(np.full(n, 180.), np.tile(_formant(), (n, 1)), np.full((n, K), .3), FS, PERIOD, noise, want_bound=True)
    assert np.all(bound > 0) and bound.max() < 1e-6 * np.abs(y).max()
    assert ref.C_FFT >= 1. + (1. + 4. * (math.sqrt(2.) + 2. ** -53))             # u more than theorem 24.2's eta / u, mu = u


def test_pulse_range_plan():
    assert ops.synth_pulse_ranges(10, 64, 3 * 8 * 64) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert ops.synth_pulse_ranges(10, 64, 1) == [(m, m + 1) for m in range(10)]          # one response at the least
    assert ops.synth_pulse_ranges(10, 64) == [(0, 10)] and ops.synth_pulse_ranges(0, 64) == [(0, 0)]
    ranges = ops.synth_pulse_ranges(100000, 1024)
    assert ranges[0] == (0, (256 << 20) // 8192) and ranges[-1][1] == 100000
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='workspace_bytes'):
            ops.synth_pulse_ranges(10, 64, bad)
    for bad in (16, 8192, 48, 64., True):
        with pytest.raises(ValueError, match='power of two'):
            ops.synth_pulse_ranges(10, bad)


def test_table_and_constants():
    table = ops.synth_table(64)
    assert table.dtype == np.float64 and table.shape == (128,)
    q = np.arange(32)
    assert np.array_equal(table[:64:2], np.cos(2. * np.pi * q / 64.)) and np.array_equal(table[1:64:2], np.sin(2. * np.pi * q / 64.))
    assert np.array_equal(table[64:], ref.dc_window(64)) and abs(table[64:].sum() - 1.) < 1e-15
    assert (ops.SYNTH_MIN_FFT, ops.SYNTH_MAX_FFT) == (32, 4096) == (_lib.MG_SYNTH_MIN_FFT, _lib.MG_SYNTH_MAX_FFT)
    assert ops.SYNTH_NOISE_SITE not in (ops.SAMPLE_SITE, ops.SPHERE_SITE, ops.ELLIPSOID_SITE, ops.MDN_COMPONENT_SITE, ops.MDN_NOISE_SITE)
    for name in ('mg_synth_noise', 'mg_synth_pulses', 'mg_synth_responses', 'mg_synth_overlap_add', 'mg_synth_lds_bytes'):
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES['mg_synth_lds_bytes'] == (ctypes.c_size_t, [ctypes.c_int])


def test_arguments_are_checked_without_a_device():
    f0, sp = torch.zeros(6), torch.ones(6, 33)
    with pytest.raises(ValueError, match='exactly one'):
        ops.world_synthesise(f0, sp, sp, 8000, 10.)
    with pytest.raises(ValueError, match='exactly one'):
        ops.world_synthesise(f0, sp, sp, 8000, 10., seq_len=[6], offsets=[0, 6])
    with pytest.raises(ValueError, match='packed'):
        ops.world_synthesise(f0, sp[None], sp[None], 8000, 10., offsets=[0, 6])
    with pytest.raises(ValueError, match='padded'):
        ops.world_synthesise(f0, sp, sp, 8000, 10., seq_len=[6])
    with pytest.raises(ValueError, match='ascending'):
        ops.world_synthesise(f0, sp, sp, 8000, 10., offsets=[0, 7])
    with pytest.raises(ValueError, match='differ in shape'):
        ops.world_synthesise(f0, sp, sp[:, :17], 8000, 10., offsets=[0, 6])
    with pytest.raises(ValueError, match='one value for each'):
        ops.world_synthesise(f0[:5], sp, sp, 8000, 10., offsets=[0, 6])
    with pytest.raises(TypeError, match='float32 or torch.float64'):
        ops.world_synthesise(f0, sp.half(), sp.half(), 8000, 10., offsets=[0, 6])
    with pytest.raises(ValueError, match='power of two'):
        ops.world_synthesise(f0, sp[:, :13], sp[:, :13], 8000, 10., offsets=[0, 6])
    with pytest.raises(ValueError, match='power of two'):
        ops.world_synthesise(f0, sp[:, :9], sp[:, :9], 8000, 10., offsets=[0, 6])          # F = 16 is below the smallest transform
    with pytest.raises(ValueError, match='sample_rate'):
        ops.world_synthesise(f0, sp, sp, 0, 10., offsets=[0, 6])
    with pytest.raises(ValueError, match='samples per frame'):
        ops.world_synthesise(f0, sp, sp, 8000, .1, offsets=[0, 6])
    with pytest.raises(ValueError, match='unvoiced pulses'):
        ops.world_synthesise(f0, sp, sp, 48000, 5., offsets=[0, 6])                        # 48 kHz / 64: 500 Hz is 96 samples
    with pytest.raises(TypeError, match='out_dtype'):
        ops.world_synthesise(f0, sp, sp, 8000, 10., offsets=[0, 6], out_dtype=torch.float16)
    with pytest.raises(ValueError, match='workspace_bytes'):
        ops.world_synthesise(f0, sp, sp, 8000, 10., offsets=[0, 6], workspace_bytes=0)
    with pytest.raises(_lib.MorganaHipError):                                               # no host implementation
        ops.world_synthesise(f0, sp, sp, 8000, 10., offsets=[0, 6])
    from morgana_amd.viz import synthesis
    if not torch.cuda.is_available():
        with pytest.raises(_lib.MorganaHipError):
            synthesis.synthesise(np.zeros(6), np.ones((6, 33)), np.ones((6, 33)), 8000, 10.)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    assert lib.mg_synth_lds_bytes(1024) == 32 * 1024 and lib.mg_synth_lds_bytes(4096) == 128 * 1024
    scale = 4294967296. / 16000.
    assert lib.mg_synth_pulses(None, 0, None, None, None, None, 80., 16000., scale, 1024, None, None, None, None, None, None) == 0    # empty
    assert lib.mg_synth_pulses(None, 1, None, None, None, None, 80., 16000., scale, 1024, None, None, None, None, None, None) == -1
    assert 'NULL' in _lib.last_error()
    for fft in (16, 8192, 96):
        assert lib.mg_synth_pulses(None, 0, None, None, None, None, 80., 16000., scale, fft, None, None, None, None, None, None) == -1
        assert 'power of two' in _lib.last_error()
        assert lib.mg_synth_responses(None, 0, None, 0, 0, *([None] * 11), 80., fft, 0, 0, None, None) == -1
        assert lib.mg_synth_overlap_add(None, 0, None, None, None, None, fft, 0, 0, 0, None, 1, 1, None, None) == -1
    assert lib.mg_synth_pulses(None, 0, None, None, None, None, 80., 16000., 2. * scale, 1024, None, None, None, None, None, None) == -1
    assert 'inc_scale' in _lib.last_error()
    assert lib.mg_synth_pulses(None, 0, None, None, None, None, .5, 16000., scale, 1024, None, None, None, None, None, None) == -1
    assert lib.mg_synth_pulses(None, 0, None, None, None, None, 80., 32000., .5 * scale, 32, None, None, None, None, None, None) == -1
    assert '500 F' in _lib.last_error()
    assert lib.mg_synth_responses(None, 0, None, 0, 1, *([None] * 11), 80., 1024, 5, 3, None, None) == -1 and 'range' in _lib.last_error()
    assert lib.mg_synth_responses(None, 0, None, 0, 1, *([None] * 11), 80., 1024, 3, 3, None, None) == 0                      # an empty range
    assert lib.mg_synth_responses(None, 0, None, 0, 1, *([None] * 11), 80., 1024, 0, 3, None, None) == -1
    assert lib.mg_synth_overlap_add(None, 1, None, None, None, None, 1024, 0, 0, 0, None, 1, 1, None, None) == 0              # no samples
    assert lib.mg_synth_overlap_add(None, 1, None, None, None, None, 1024, 0, 0, 10, None, 1, 1, None, None) == -1
    assert lib.mg_synth_noise(None, 0, 1, 2, None, None) == 0 and lib.mg_synth_noise(None, 8, 1, 2, None, None) == -1
    assert lib.mg_synth_noise(None, -1, 1, 2, None, None) == -1


def test_corpus_synthesis_refuses_existing_outputs_before_it_reads(tmp_path):
    from morgana_amd.viz import synthesis
    (tmp_path / 'out').mkdir()
    (tmp_path / 'out' / 'b.wav').write_bytes(b'kept')
    with pytest.raises(FileExistsError, match='b.wav'):
        synthesis.synthesise_files(['a', 'b'], str(tmp_path / 'missing'), str(tmp_path / 'out'), 16000)
    assert (tmp_path / 'out' / 'b.wav').read_bytes() == b'kept'
    with pytest.raises(FileNotFoundError):               # with overwrite it goes on to read - and finds no input
        synthesis.synthesise_files(['a', 'b'], str(tmp_path / 'missing'), str(tmp_path / 'out'), 16000, overwrite=True)
