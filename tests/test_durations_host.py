"""The duration quantiser on the host: data.quantise_durations' NumPy form against tests/durations_ref.py (python floats and integers,
the sequential emit rule), the closed form of the carry rule against that rule, the properties the rule is used for, the flag bits,
the condition that makes the GPU test's inputs decidable under the reference alone, and the argument refusals."""
import math

import numpy as np
import pytest

import durations_ref as ref
from morgana_amd import data, ops


def _random_item(rng, log_input=False):
    n_phones, n_states = int(rng.randint(1, 40)), int(rng.choice([1, 3, 5]))
    frames = rng.gamma(2.0, rng.choice([0.4, 1.5, 6.0]), size=(n_phones, n_states)) + 0.01
    frames[rng.rand(n_phones, n_states) < 0.1] = 0.004     # next to empty: the minimum comes into play
    if log_input:
        mean, std_dev = (1.0 + rng.rand(n_states)).astype(np.float32), (0.5 + rng.rand(n_states)).astype(np.float32)
        value = np.log(frames)
    else:
        mean, std_dev = (5.0 + rng.rand(n_states)).astype(np.float32), (2.0 + rng.rand(n_states)).astype(np.float32)
        value = frames
    pred = ((value - mean.astype(np.float64)) / std_dev.astype(np.float64)).astype(np.float32)
    return pred, mean, std_dev


def _host(pred, mean, std_dev, **kwargs):
    normaliser = None if mean is None else data.MeanVarianceNormaliser('dur').set_params({'mean': mean, 'std_dev': std_dev})
    return data.quantise_durations(pred, normaliser=normaliser, **kwargs)


def _same(host, want):
    np.testing.assert_array_equal(host[0], want.dur)
    np.testing.assert_array_equal(host[1], want.phone_dur)
    assert host[0].dtype == np.int64 and host[1].dtype == np.int64
    assert (host[2], host[3]) == (want.n_frames, want.flags)


def test_numpy_form_equals_the_reference_on_random_cases():
    rng = np.random.RandomState(1)
    checked = 0
    for k in range(300):
        log_input = k % 3 == 0
        pred, mean, std_dev = _random_item(rng, log_input)
        lo, hi = int(rng.choice([0, 1, 2])), int(rng.choice([30, 200, ref.MAX_FRAMES]))
        scale = float(rng.choice([1.0, 0.8, 1.37]))
        total = None if k % 2 else int(rng.randint(1, 40 * pred.shape[0]))
        for rounding in ('carry', 'nearest'):
            want = ref.item(pred, None, mean, std_dev, log_input=log_input, scale=scale, lo=lo, hi=hi, rounding=rounding, total=total)
            if want.undecided:
                continue
            _same(_host(pred, mean, std_dev, log_input=log_input, scale=scale, min_frames=lo, max_frames=hi, rounding=rounding, total=total),
                  want)
            checked += 1
    assert checked > 550
    flat = rng.gamma(2.0, 3.0, size=11).astype(np.float32)
    got = data.quantise_durations(flat)
    assert got[0].shape == (11,) and got[1].shape == (11,)
    _same((got[0].reshape(11, 1),) + got[1:], ref.item(flat))


def test_closed_form_equals_the_sequential_rule():
    rng = np.random.RandomState(2)
    for _ in range(3000):
        n = int(rng.randint(1, 60))
        q = [int(v) for v in (rng.gamma(1.5, rng.choice([0.3, 2.0, 9.0]), size=n) * 65536)]
        for k in rng.randint(0, n, size=n // 4):
            q[k] = 0
        lo = int(rng.choice([0, 1, 3]))
        assert ref.closed_form(q, lo) == ref.sequential(q, lo)


def test_properties_bounds_total_drift_and_exact_fit():
    rng = np.random.RandomState(3)
    for k in range(300):
        pred, _, _ = _random_item(rng)
        frames = np.abs(pred.astype(np.float64)) * 6 + (1.0 if k % 2 else 0.0)      # k odd: every value >= lo = 1
        frames = frames.astype(np.float32)
        hi = int(rng.choice([40, ref.MAX_FRAMES]))
        dur, phone_dur, n_frames, flags = data.quantise_durations(frames, min_frames=1, max_frames=hi)
        q = ref.item(frames, lo=1, hi=hi).fixed
        assert dur.min() >= 1 and dur.max() <= max(1, hi) and n_frames == dur.sum() and np.array_equal(phone_dur, dur.sum(axis=1))
        if k % 2:
            ends, predicted = np.cumsum(dur.reshape(-1)), np.cumsum(q) / 65536.0
            assert n_frames == (sum(q) + 32768) >> 16 and not flags & ops.DUR_FLAG_PUSHED
            assert np.abs(ends - predicted).max() <= 0.5
            # a total at or above the predicted one scales every value up: none falls below lo, the fit is exact
            total = int(math.ceil(float(frames.astype(np.float64).sum()))) + int(rng.randint(0, 10 * frames.size))
            if hi == ref.MAX_FRAMES:
                fitted = data.quantise_durations(frames, total=total)
                assert fitted[2] == total and fitted[3] == 0 and fitted[0].min() >= 1
        nearest = data.quantise_durations(frames, min_frames=1, max_frames=hi, rounding='nearest')
        assert nearest[0].min() >= 1 and nearest[0].max() <= max(1, hi)
    # one value a long way below the minimum pushes the length out, and says so
    pushed = data.quantise_durations(np.array([3.0, 0.0, 0.0, 0.0, 0.0, 0.2], dtype=np.float32), min_frames=1)
    assert pushed[0].tolist() == [3, 1, 1, 1, 1, 1] and pushed[2] == 8 and pushed[3] == ops.DUR_FLAG_PUSHED


def test_flag_bits():
    x = np.array([[2.5, 1.0], [4.0, 3.0]], dtype=np.float32)
    assert data.quantise_durations(x)[3] == 0
    for bad in (np.nan, np.inf, -3.0):
        y = x.copy()
        y[1, 0] = bad
        dur, _, _, flags = data.quantise_durations(y, rounding='nearest', min_frames=0)
        assert flags == ops.DUR_FLAG_INVALID and dur[1, 0] == 0
        _same(data.quantise_durations(y), ref.item(y))
    assert data.quantise_durations(x, total=0)[3] == ops.DUR_FLAG_NO_FIT
    assert data.quantise_durations(x, total=-4)[3] == ops.DUR_FLAG_NO_FIT
    assert data.quantise_durations(np.zeros((3, 1), np.float32), total=9, min_frames=0)[3] == ops.DUR_FLAG_NO_FIT
    assert data.quantise_durations(np.full((2, 2), 1e30, np.float32), max_frames=7)[0].tolist() == [[7, 7], [7, 7]]
    large = data.quantise_durations(np.array([88.8], np.float32), log_input=True, max_frames=9)                            # large, finite
    assert large[0].tolist() == [9] and large[3] == 0
    assert data.quantise_durations(np.array([800.0], np.float32), log_input=True, min_frames=0)[3] == ops.DUR_FLAG_INVALID   # exp overflows
    assert data.quantise_durations(np.array([800.0], np.float32), log_input=True)[3] == ops.DUR_FLAG_INVALID | ops.DUR_FLAG_PUSHED
    assert (ops.DUR_FLAG_INVALID, ops.DUR_FLAG_NO_FIT, ops.DUR_FLAG_PUSHED, ops.DUR_FLAG_NO_ROW) == (ref.INVALID, ref.NO_FIT, ref.PUSHED,
                                                                                                     ref.NO_ROW) == (1, 2, 4, 8)


def test_gpu_inputs_have_no_undecided_segment():
    """Every log_input case of tests/test_gpu_durations.py is decided under the reference alone: an exp that differs from math.exp by up
    to 8 units in the last place cannot change a bit of what the GPU test compares."""
    import test_gpu_durations as gpu
    n = 0
    for pred, n_phones, mean, std_dev, log_input, lo, hi in gpu.all_reference_inputs():
        for rounding in ('carry', 'nearest'):
            assert ref.batch(pred, n_phones, mean, std_dev, log_input=log_input, lo=lo, hi=hi, rounding=rounding)[4] == 0
            n += 1
    assert n == 4
    # the margin itself: a value a hair from a rounding boundary is undecided, the rest of an ordinary item is not
    x = math.log((5 * 65536 + 0.5) / 65536.0)
    assert ref.item(np.array([np.float32(x)]), log_input=True).undecided in (0, 1)
    assert ref._undecided((5 * 65536 + 0.5) / 65536.0, ref.MAX_FRAMES) and not ref._undecided(5.25, ref.MAX_FRAMES)


def test_speaker_dependent_normaliser_on_the_host():
    rng = np.random.RandomState(4)
    pred, mean, std_dev = _random_item(rng)
    normaliser = data.SpeakerDependentMeanVarianceNormaliser('dur', None).set_params(
        {'anna': {'mean': mean, 'std_dev': std_dev}, 'bert': {'mean': mean + np.float32(2), 'std_dev': std_dev * np.float32(2)}})
    _same(data.quantise_durations(pred, normaliser=normaliser, speaker_index='bert'),
          ref.item(pred, None, mean + np.float32(2), std_dev * np.float32(2)))
    with pytest.raises(KeyError):
        data.quantise_durations(pred, normaliser=normaliser)


def test_argument_refusals():
    x = np.ones((3, 2), dtype=np.float32)
    with pytest.raises(ValueError):
        data.quantise_durations(x, rounding='floor')
    with pytest.raises(ValueError):
        data.quantise_durations(x, min_frames=3, max_frames=2)
    with pytest.raises(ValueError):
        data.quantise_durations(x, min_frames=-1)
    with pytest.raises(ValueError):
        data.quantise_durations(x, max_frames=2 ** 20 + 1)
    with pytest.raises(TypeError):
        data.quantise_durations(x, min_frames=1.5)
    for scale in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            data.quantise_durations(x, scale=scale)
    with pytest.raises(ValueError):
        data.quantise_durations(x, n_phones=np.array([3]))
    with pytest.raises(TypeError):
        data.quantise_durations(x.astype(np.int64))
    with pytest.raises(ValueError):
        data.quantise_durations(np.ones((2, 2, 2), dtype=np.float32))
    with pytest.raises(TypeError):
        data.quantise_durations(x, total=2.5)
    with pytest.raises(TypeError):
        data.quantise_durations(x, normaliser=data.MinMaxNormaliser('dur'))
    with pytest.raises(ValueError):
        data.quantise_durations(x, speaker_index='anna')
    with pytest.raises(ValueError):
        data.quantise_durations(x, normaliser=data.MeanVarianceNormaliser('dur').set_params({'mean': np.zeros(3), 'std_dev': np.ones(3)}))
    with pytest.raises(TypeError):
        data.quantise_durations([1.0, 2.0])
    import torch
    with pytest.raises(Exception):
        data.quantise_durations(torch.ones(2, 3))           # a CPU tensor: no CPU fallback for the device path
    from morgana_amd import models
    with pytest.raises(ValueError):
        models.DurationModel(rounding='floor')
    with pytest.raises(ValueError):
        models.DurationModel(n_states=0)
    with pytest.raises(KeyError):
        models.with_predicted_durations({}, {'dur': None}, {})
    model = models.DurationModel(n_states=5)
    assert model.layers[12].weight.shape == (5, 64) and sorted(model.normaliser_sources()) == ['dur', 'lab']
    assert model.fit_to('n_frames') is model and model._fit_key == 'n_frames' and model.fit_to(None)._fit_key is None
