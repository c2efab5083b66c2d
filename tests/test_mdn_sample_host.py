"""Host-side checks of the sampled mixture-density generation (no GPU): the float64 restatement the GPU tests hold the kernel to
(tests/mdn_sample_ref64.py) against an independent numpy formulation, a plain fp32 evaluation of the rule against its derived margin,
the share of undecided frames on the GPU tests' own inputs, the frequency test on the restatement alone (the GPU test's seed and
counter, Philox words from the library's host-only mg_philox4x32_10), the host checks of mg_mdn_sample_f32 and what the Python layers
refuse without a device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
import torch.nn as nn

import mdn_ref64
import mdn_sample_ref64 as ref
import sampling_ref64
from morgana_amd import _lib, losses, models, ops, utils


def _philox(counter, key):
    c, k, out = (ctypes.c_uint32 * 4)(*counter), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
    _lib.load().mg_philox4x32_10(c, k, out)
    return [int(v) for v in out]


def _uniforms(b, t):
    return ref.component_uniforms(b * t, ref.SEED, ops.MDN_COMPONENT_SITE, ref.CTR, _philox).reshape(b, t)


# --------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('k', [1, 2, 8, 64])
@pytest.mark.parametrize('temperature', ref.TEMPERATURES)
def test_restatement_equals_searchsorted_and_covers_an_fp32_evaluation(k, temperature):
    """Given the uniforms: the component is np.searchsorted's on the float64 cumulative sum (an independent formulation) on every
    decided frame, and a plain fp32 numpy evaluation of the documented rule differs from it on undecided frames only - and there
    stays among the components next to the boundary."""
    rng = np.random.RandomState(31 * k + int(8 * temperature))
    frames = 20000
    logits = (2.0 * rng.standard_normal((frames, k))).astype(np.float32)
    u = np.array([sampling_ref64.uniform(w) for w in rng.randint(0, 2 ** 32, size=frames, dtype=np.uint64)])
    # frames that sit ON a boundary, to the last fp32 digit: the margin is exercised, not only sampled
    if k > 1:
        cdf32 = np.cumsum(ref.weights(logits[:2000], temperature)[3], axis=-1)
        pick = rng.randint(0, k - 1, size=2000)
        near = np.float32(cdf32[np.arange(2000), pick])
        u[:2000] = np.clip(np.floor(near.astype(np.float64) * 2 ** 24) // 2 * 2 + 1, 1, 2 ** 24 - 1) * 2.0 ** -24   # an odd multiple of 2^-24
    out = ref.choose(logits, u, temperature)
    p = out['probability']
    scaled = np.cumsum(p, axis=-1)
    independent = np.minimum([np.searchsorted(scaled[i], u[i], side='right') for i in range(frames)], k - 1)
    decided = out['decided']
    assert np.array_equal(out['component'][decided], independent[decided])
    got32 = ref.fp32_choice(logits, u, temperature)
    differs = got32 != out['component']
    print('K=%d temperature=%g: %d of %d frames undecided, the fp32 evaluation differs on %d' % (k, temperature, (~decided).sum(), frames,
                                                                                                 differs.sum()))
    assert not np.any(differs & decided)
    assert np.all((out['lowest'] <= got32) & (got32 <= out['highest']))
    assert np.all(np.take_along_axis(out['live'], got32[:, None], axis=-1))
    assert np.all(out['lowest'][decided] == out['component'][decided]) and np.all(out['highest'][decided] == out['component'][decided])
    if k == 1:
        assert decided.all() and np.all(out['component'] == 0)
    else:
        assert 0 < (~decided).sum() and (~decided[2000:]).mean() <= ref.UNDECIDED_CAP
    # the margin's size: a small multiple of (K + 8) U, never a tolerance
    assert np.all(out['delta'] <= 2.2 * (k + 8) * ref.U) and np.all(out['delta'] >= (2 * (k - 1) + 9) * ref.U)


def test_restatement_edge_semantics():
    k = 4
    logits = np.array([[0.0, -np.inf, 1.0, -np.inf], [-np.inf] * 4, [-np.inf, -np.inf, 3.0, -np.inf], [1.0, 1.0, 1.0, 1.0]], dtype=np.float32)
    top = 1.0 - 2.0 ** -24
    for u in (2.0 ** -24, 0.25, 0.5, top):
        out = ref.choose(logits, np.full(4, u))
        assert out['component'][0] in (0, 2) and out['component'][2] == 2       # a -inf logit is never drawn
        assert out['component'][1] == 0 and out['broken'][1] and out['decided'][1]   # every logit -inf: mg_mdn_select_f32's component
        assert out['component'][3] == int(u * 4)
    assert ref.choose(logits, np.full(4, top))['component'][0] == 2
    # no k with u < C_k cannot happen in float64 (C_{K-1} = 1 > u): the fallback is the last LIVE component, reached through lowest / highest
    out = ref.choose(logits, np.full(4, top))
    assert out['highest'][0] == 2 and out['highest'][2] == 2
    # temperature: towards the mode below 1, towards uniform above
    cold, warm = ref.weights(logits[0], 0.5)[3], ref.weights(logits[0], 2.0)[3]
    assert cold[2] > ref.weights(logits[0])[3][2] > warm[2] > 0.5 and cold[1] == warm[1] == 0.0
    assert ref.inv_temperature(0.5) == 2.0 and ref.inv_temperature(2.0) == 0.5 and ref.inv_temperature(3.0) == float(np.float32(1.0 / 3.0))
    # pad frames: 0, 0 and 1, decided, not read
    pred, seq_len = ref.case(8, 3)
    dirty = pred.copy()
    b, t, _ = pred.shape
    mask = np.arange(t)[None, :] < seq_len[:, None]
    dirty[~mask] = np.nan
    u = np.full((b, t), 0.3)
    noise = np.ones((b, t, 3))
    clean_out, dirty_out = (ref.sample(x, seq_len, 8, 3, u, noise, noise_scale=1.0) for x in (pred, dirty))
    for key in ('component', 'mean', 'variance', 'mean_bound'):
        assert np.array_equal(clean_out[key], dirty_out[key]), key
    assert np.all(clean_out['component'][~mask] == 0) and np.all(clean_out['mean'][~mask] == 0.0) and np.all(clean_out['variance'][~mask] == 1.0)
    # the moments: mu + noise_scale exp(max(s, floor)) g and exp(2 max(s, floor)) of the chosen component
    _, mu, s = mdn_ref64.split(pred.astype(np.float64), 8, 3)
    floored = ref.sample(pred, seq_len, 8, 3, u, noise, min_log_std=-0.5, noise_scale=0.5)
    pick = floored['component'][:, :, None, None]
    sd = np.maximum(np.take_along_axis(s, pick, axis=2)[:, :, 0], -0.5)
    want = np.take_along_axis(mu, pick, axis=2)[:, :, 0] + 0.5 * np.exp(sd)
    assert np.array_equal(floored['mean'][mask], want[mask]) and np.array_equal(floored['variance'][mask], np.exp(2 * sd)[mask])
    assert np.all(floored['mean_bound'][mask] > 0) and np.all(floored['mean_bound'][mask] <= 2e-6 * (np.abs(want[mask]) + np.exp(sd[mask])))
    plain = ref.sample(pred, seq_len, 8, 3, u)
    assert np.all(plain['mean_bound'] == 0.0) and np.array_equal(plain['mean'][mask], np.take_along_axis(mu, plain['component'][:, :, None, None], axis=2)[:, :, 0][mask])
    with pytest.raises(ValueError, match='needs the noise'):
        ref.sample(pred, seq_len, 8, 3, u, noise_scale=1.0)


@pytest.mark.parametrize('k, d', sorted(ref.CASES))
def test_gpu_inputs_keep_their_undecided_share_under_the_cap(k, d):
    """The GPU tests' own inputs, uniforms and temperatures: at most 1 % of the valid frames are undecided (K = 64: at least 2000
    valid frames, so that the cap is a statement about the margin and not about one unlucky frame)."""
    pred, seq_len = ref.case(k, d)
    b, t, _ = pred.shape
    u = _uniforms(b, t)
    valid = int(np.clip(seq_len, 0, t).sum())
    assert 3 <= b <= 4 and t <= 640 and t % 16 != 0 and (k != 64 or valid >= 2000)
    for temperature in ref.TEMPERATURES:
        out = ref.sample(pred, seq_len, k, d, u, temperature=temperature)
        undecided = int((~out['decided'] & out['mask']).sum())
        print('K=%d D=%d temperature=%g: %d of %d valid frames undecided' % (k, d, temperature, undecided, valid))
        assert undecided <= ref.UNDECIDED_CAP * valid
        assert np.array_equal(ref.fp32_choice(pred[:, :, :k], u, temperature)[out['decided'] & out['mask']], out['component'][out['decided'] & out['mask']])
        if k > 1 and valid > 50:
            assert len(np.unique(out['component'][out['mask']])) > 1


def test_cases_cover_every_kernel_path():
    widths = sorted(d for _, d in ref.CASES)
    assert ref.ELEMENT_D in widths and ref.ELEMENT_D + 1 in widths                  # noise one element | one Philox block per lane
    assert any(d > ref.ELEMENT_D and d % 4 != 0 for d in widths)                    # blocks that straddle rows, in the block form
    assert any(d <= ref.ELEMENT_D and d % 4 != 0 for d in widths)                   # ... and in the element form
    assert max(k for k, _ in ref.CASES) == mdn_ref64.MAX_COMPONENTS and max(k * d for k, d in ref.CASES) == mdn_ref64.MAX_ROW
    assert min(ref.CASES) == (1, 1)


@pytest.mark.parametrize('k', [8, 64])
def test_restatement_passes_the_frequency_test(k):
    """16384 frames that share one logit vector, the GPU test's seed and counter: every component's share within five binomial
    standard deviations (+ one frame) of its float64 probability."""
    pred, p = ref.frequency_case(k)
    b, t, _ = pred.shape
    n = b * t
    assert n == 16384 and abs(p.sum() - 1.0) < 1e-12
    out = ref.choose(pred[:, :, :k], _uniforms(b, t))
    share = np.bincount(out['component'].ravel(), minlength=k) / n
    worst = np.abs(share - p) / ref.frequency_bound(p, n)
    print('K=%d: worst |f - p| / bound %.3f, %d undecided' % (k, worst.max(), (~out['decided']).sum()))
    assert np.all(worst <= 1.0)
    # an undecided frame moves a share by 1 / N at most: the test does not hinge on them
    assert (~out['decided']).sum() <= ref.UNDECIDED_CAP * n


def test_uniforms_follow_the_documented_word_mapping():
    u = ref.component_uniforms(9, ref.SEED, ops.MDN_COMPONENT_SITE, ref.CTR, _philox)
    for r in (0, 3, 4, 8):
        block = _philox([r // 4, 0, ref.CTR & 0xFFFFFFFF, (ops.MDN_COMPONENT_SITE ^ (ref.CTR >> 32)) & 0xFFFFFFFF],
                        [ref.SEED & 0xFFFFFFFF, ref.SEED >> 32])
        assert u[r] == ((block[r % 4] >> 8) | 1) * 2.0 ** -24 and 0.0 < u[r] < 1.0
    assert len({ops.SAMPLE_SITE, ops.SPHERE_SITE, ops.ELLIPSOID_SITE, ops.MDN_COMPONENT_SITE, ops.MDN_NOISE_SITE}) == 5


# ------------------------------------------------------------------------------------------------------------ the C ABI, host side
def test_mdn_sample_entry_point_validates_its_arguments_without_a_gpu():
    lib = _lib.load()

    def call(pred=16, ldp=56, col0=0, b=2, t=3, k=8, d=3, inv=1.0, noise=0.0, site_c=1, site_n=2, component=16, mean=16, variance=16):
        return lib.mg_mdn_sample_f32(pred, ldp, col0, None, b, t, k, d, 0.0, 0, inv, noise, 7, site_c, site_n, None, component, mean,
                                     variance, None)

    assert call(k=65, d=1, ldp=65 * 3) == -1 and 'cap of 64' in _lib.last_error()
    assert call(k=1, d=16385, ldp=2 * 16385 + 1) == -1 and 'cap of 16384' in _lib.last_error()
    assert call(k=0) == -1 and 'mg_mdn_sample_f32' in _lib.last_error()
    assert call(pred=None) == -1 and 'NULL' in _lib.last_error()
    assert call(mean=None) == -1 and call(variance=None) == -1 and call(component=None) == -1
    assert call(ldp=55) == -1 and 'ldp=55' in _lib.last_error()
    assert call(ldp=58, col0=3) == -1 and call(col0=-1) == -1 and call(t=0) == -1 and call(b=0) == -1 and call(b=65536) == -1
    assert call(inv=0.0) == -1 and 'inv_temperature' in _lib.last_error()
    assert call(inv=-1.0) == -1 and call(inv=float('inf')) == -1 and call(inv=float('nan')) == -1
    assert call(noise=-0.5) == -1 and 'noise_scale' in _lib.last_error()
    assert call(noise=float('inf')) == -1 and call(noise=float('nan')) == -1
    assert call(site_c=5, site_n=5) == -1 and 'site' in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(call(k=0), 'mg_mdn_sample_f32')
    assert _lib.SIGNATURES['mg_mdn_sample_f32'][1][10:15] == [ctypes.c_float, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]


# ------------------------------------------------------------------------------------------------------------------ host layers
def test_losses_mdn_sample_refusals_that_need_no_device():
    x = torch.zeros(2, 5, 28)
    assert list(inspect.signature(losses.mdn_sample).parameters) == ['predictions', 'n_components', 'dim', 'seq_len', 'min_log_std',
                                                                     'temperature', 'noise_scale']
    assert list(inspect.signature(ops.mdn_sample).parameters) == ['pred', 'seq_len', 'n_components', 'dim', 'seed', 'used', 'min_log_std',
                                                                  'temperature', 'noise_scale', 'col0']
    with pytest.raises(ValueError, match='mdn_select'):
        losses.mdn_sample(x, 4, 3, temperature=0)
    with pytest.raises(ValueError, match='mdn_select'):
        losses.mdn_sample(x, 4, 3, temperature=0.0)
    for bad in (-1.0, float('inf'), float('nan'), None, '1', torch.ones(()), True):
        with pytest.raises(ValueError, match='temperature'):
            losses.mdn_sample(x, 4, 3, temperature=bad)
        with pytest.raises(ValueError, match='temperature'):
            ops.mdn_sample(x, None, 4, 3, 1, None, temperature=bad)
    for bad in (-1e-3, float('inf'), float('nan'), None, torch.zeros(())):
        with pytest.raises(ValueError, match='noise_scale'):
            losses.mdn_sample(x, 4, 3, noise_scale=bad)
    with pytest.raises(ValueError, match='temperature'):
        losses.mdn_sample(x, 4, 3, temperature=1e-60)                              # 1 / temperature is no finite float32
    with pytest.raises(ValueError, match=r'4 \* \(1 \+ 2 \* 3\) = 28'):
        losses.mdn_sample(torch.zeros(2, 5, 27), 4, 3)
    with pytest.raises(TypeError, match='float32'):
        losses.mdn_sample(torch.zeros(2, 5, 28, dtype=torch.float64), 4, 3)
    with pytest.raises(_lib.MorganaHipError, match='no CPU fallback'):             # the right arguments: refused for the device only
        losses.mdn_sample(x, 4, 3, temperature=0.7, noise_scale=1)
    assert 'not provided' not in losses.mdn_select.__doc__ and 'mdn_sample' in losses.mdn_select.__doc__


def test_sample_mixtures_sets_one_attribute_and_refuses_models_without_a_mixture():
    mixture = models.GRUF0Model(n_components=4)
    assert mixture._mixture_sampling is None                                        # the default: select
    assert mixture.sample_mixtures() is mixture and mixture._mixture_sampling == (1.0, 0.0)
    assert mixture.sample_mixtures(temperature=0.5, noise_scale=2)._mixture_sampling == (0.5, 2.0)
    assert mixture.select_mixtures() is mixture and mixture._mixture_sampling is None
    assert '_mixture_sampling' not in mixture.state_dict() and sorted(mixture.state_dict()) == sorted(models.GRUF0Model().state_dict())
    with pytest.raises(ValueError, match='mdn_select'):
        mixture.sample_mixtures(temperature=0)
    with pytest.raises(ValueError, match='noise_scale'):
        mixture.sample_mixtures(noise_scale=-1)
    assert mixture._mixture_sampling is None                                        # a refused call changes nothing
    for plain in (models.GRUF0Model(), models.GRUF0Model(predict_variance=True), models.LSTMAcousticModel(num_layers=1), models.VAEF0Model()):
        with pytest.raises(ValueError, match="no 'mdn' stream"):
            plain.sample_mixtures()
        assert plain.select_mixtures() is plain
    streams = [models.Stream('lf0', 3, 'mdn', n_components=4), models.Stream('vuv', 1, 'sigmoid_bce')]
    layers = utils.SequentialWithRecurrent(nn.Linear(609, 16), nn.Sigmoid(), nn.Linear(16, 29), precision='fp32')
    assert models.StreamModel(layers, streams).sample_mixtures(2.0)._mixture_sampling == (2.0, 0.0)
