"""Generation under a global-variance prior on the device (run with ``-m gpu`` on an MI355X): mg_mlpg_gv_f32 against the dense float64
restatement of tests/mlpg_gv_ref64.py (whose cases and bounds these are) - the output, the stationarity of F at it, the multiplier
and the fallback flags - then gv_weight = 0, determinism, the frames it must not read, graph replay, viz.synthesis.MLPG_GV, the
model switch generate_with_gv and the statistics of data.fit_global_variance.

Worst ratios measured on an MI355X over every case below (the bounds are the issue's): see DESIGN.md section 4.22."""
import functools
import os

import numpy as np
import pytest
import torch

import mlpg_gv_ref64 as ref
from morgana_amd import data, losses, models, ops, synthetic, viz

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CASE_IDS = ['-'.join(str(part) for part in key) for key in ref.CASE_KEYS]


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)         # a copy: the shared cases are read-only


def _call(key, means=None, **kwargs):
    own, variances, gv_mean, gv_variance, windows, padding, seq_len = ref.case(*key)[:7]
    return ops.mlpg_gv(dev(own if means is None else means), dev(variances), dev(gv_mean), dev(gv_variance), windows,
                       padding_size=padding, seq_len=dev(seq_len), **kwargs)


@functools.lru_cache(maxsize=None)
def _run64(key):
    """(trajectory f64, info) of one case as host arrays: one launch shared by the checks of the float64 output."""
    out, info = _call(key, out_dtype=torch.float64, want_info=True)
    assert out.dtype == torch.float64 and info.dtype == torch.float64 and tuple(info.shape) == (ref.BSZ, ref.DIM, 4)
    return out.cpu().numpy(), info.cpu().numpy()


def _scale(want):
    return np.abs(want).max(axis=1, keepdims=True)        # max |x_ref| of each system (b, d)


# ------------------------------------------------------------------------------------------------ 1. the float64 output
@pytest.mark.parametrize('key', ref.CASE_KEYS, ids=CASE_IDS)
def test_f64_output_equals_the_float64_reference(key):
    want = ref.case(*key)[7]
    got, _ = _run64(key)
    assert got.shape == want.shape and np.isfinite(got).all()
    limit = ref.X_FLOOR * _scale(want)
    ratio = (np.abs(got - want) / np.where(limit > 0, limit, 1.0))[np.broadcast_to(limit > 0, want.shape)]
    print('%s: worst |x - x_ref| / (1e-9 max |x_ref|) = %.3e' % (key, ratio.max()))
    assert (np.abs(got - want) <= limit).all()


@pytest.mark.parametrize('key', ref.CASE_KEYS, ids=CASE_IDS)
def test_f64_output_is_a_stationary_point(key):
    """grad F recomputed on the host from the output rows (the padding rows, which the prior does not see, completed by their own
    block of P x = rhs): within 1e-9 of the gradient at MLPG's solution, per system that did not fall back."""
    info_ref, systems = ref.case(*key)[8:10]
    got, info = _run64(key)
    worst = 0.0
    for (b, d), system in systems.items():
        if info_ref[b, d, 3]:
            continue
        x = system.complete(got[b, :system.length, d])
        at_x, at_start = np.abs(system.gradient(x)).max(), np.abs(system.gradient(system.x0)).max()
        worst = max(worst, at_x / at_start)
        assert at_x <= ref.GRAD_RATIO * at_start, (b, d, at_x, at_start)
    print('%s: worst |grad F(x)| / |grad F(x0)| = %.3e' % (key, worst))


@pytest.mark.parametrize('key', ref.CASE_KEYS, ids=CASE_IDS)
def test_info_kappa_flags_and_evaluations(key):
    info_ref = ref.case(*key)[8]
    _, info = _run64(key)
    flags = info[:, :, 3]
    assert np.array_equal(flags, info_ref[:, :, 3])
    assert {b for b in range(ref.BSZ) if flags[b].any()} == {4, ref.DEGENERATE}            # the one-frame item and the all-zero one
    ok = flags == 0
    kappa, kappa_ref = info[:, :, 0][ok], info_ref[:, :, 0][ok]
    print('%s: worst |kappa - kappa_ref| / |kappa_ref| = %.3e (2^-36 = %.3e), evaluations %d .. %d' % (
        key, (np.abs(kappa - kappa_ref) / np.abs(kappa_ref)).max(), ref.KAPPA_REL, info[:, :, 2][ok].min(), info[:, :, 2][ok].max()))
    assert (np.abs(kappa - kappa_ref) <= ref.KAPPA_REL * np.abs(kappa_ref)).all()
    h_abs, used = info[:, :, 1][ok], info[:, :, 2][ok]
    assert (h_abs <= ref.H_RULE * (1.0 + np.abs(kappa))).all()
    assert (used <= 48).all() and (used >= 2).all()
    assert (info[4, :, :2] == 0).all()                                                     # one frame: nothing was searched


# ------------------------------------------------------------------------------------------------ 2. the float32 output
@pytest.mark.parametrize('key', ref.CASE_KEYS, ids=CASE_IDS)
def test_f32_output(key):
    want = ref.case(*key)[7]
    got = _call(key)
    assert got.dtype == torch.float32
    got = got.cpu().numpy().astype(np.float64)
    limit = ref.F32_ROUNDING * np.abs(want) + ref.X_FLOOR * _scale(want)
    assert np.isfinite(got).all() and (np.abs(got - want) <= limit).all()


# ------------------------------------------------------------------------------------------------ 3. no prior, fallbacks
@pytest.mark.parametrize('out_dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('key', [ref.CASE_KEYS[0], ref.CASE_KEYS[5], ref.CASE_KEYS[-1]], ids=[CASE_IDS[0], CASE_IDS[5], CASE_IDS[-1]])
def test_weight_zero_is_mlpg_bit_for_bit(key, out_dtype):
    means, variances, _, _, windows, padding, seq_len = ref.case(*key)[:7]
    plain = ops.mlpg(dev(means), dev(variances), windows, padding_size=padding, seq_len=dev(seq_len), out_dtype=out_dtype)
    got, info = _call(key, gv_weight=0., out_dtype=out_dtype, want_info=True)
    assert torch.equal(got, plain)
    assert np.array_equal(info.cpu().numpy(), np.broadcast_to(np.array([0., 0., 0., 1.]), (ref.BSZ, ref.DIM, 4)))


def test_fallback_items_are_the_mlpg_solution():
    key = ref.CASE_KEYS[0]
    means, variances, _, _, windows, padding, seq_len = ref.case(*key)[:7]
    plain = ops.mlpg(dev(means), dev(variances), windows, padding_size=padding, seq_len=dev(seq_len), out_dtype=torch.float64).cpu().numpy()
    got, _ = _run64(key)
    for b in (4, ref.DEGENERATE):
        assert (np.abs(got[b] - plain[b]) <= ref.X_FLOOR * np.abs(plain[b]).max()).all()
    assert not got[ref.DEGENERATE].any()
    assert np.abs(got[0] - plain[0]).max() > 1e-3 * np.abs(plain[0]).max()                  # and the prior moves the others


# ------------------------------------------------------------------------------------------------ 4. determinism, pad frames, graph
def test_two_calls_give_equal_bits():
    for key in (ref.CASE_KEYS[0], ref.CASE_KEYS[-1]):
        first, info_first = _call(key, want_info=True)
        second, info_second = _call(key, want_info=True)
        assert torch.equal(first, second) and torch.equal(info_first, info_second)


@pytest.mark.parametrize('key', [ref.CASE_KEYS[0], ref.CASE_KEYS[6], ref.CASE_KEYS[-1]], ids=[CASE_IDS[0], CASE_IDS[6], CASE_IDS[-1]])
def test_frames_past_seq_len_are_not_read_and_come_back_zero(key):
    means, seq_len = ref.case(*key)[0], ref.case(*key)[6]
    past = np.arange(means.shape[1])[None, :] >= seq_len[:, None]
    assert past.any()
    poisoned = means.copy()
    poisoned[past] = np.nan
    want, got = _call(key), _call(key, means=poisoned)
    assert torch.equal(got, want)                         # NaN != NaN: equal bits also means no NaN came through
    assert not got.cpu().numpy()[past].any()


def test_graph_replay_equals_eager():
    key = ref.CASE_KEYS[1]
    means, variances, gv_mean, gv_variance, windows, padding, seq_len = (
        dev(v) if isinstance(v, np.ndarray) else v for v in ref.case(*key)[:7])
    eager, eager_info = ops.mlpg_gv(means, variances, gv_mean, gv_variance, windows, padding_size=padding, seq_len=seq_len, want_info=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # warm-up on the capture's stream
        ops.mlpg_gv(means, variances, gv_mean, gv_variance, windows, padding_size=padding, seq_len=seq_len, want_info=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, info = ops.mlpg_gv(means, variances, gv_mean, gv_variance, windows, padding_size=padding, seq_len=seq_len, want_info=True)
    out.fill_(7.0)
    info.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(info, eager_info)


# ------------------------------------------------------------------------------------------------ 5. the reference-shaped entry point
def test_viz_synthesis_mlpg_gv_conventions():
    key = ref.CASE_KEYS[0]
    means, variances, gv_mean, gv_variance, windows, padding, seq_len, want = ref.case(*key)[:8]
    as_array = viz.synthesis.MLPG_GV(means, variances, gv_mean, gv_variance, padding_size=padding, seq_len=seq_len)
    assert isinstance(as_array, np.ndarray) and as_array.dtype == np.float64
    assert (np.abs(as_array - want) <= ref.X_FLOOR * _scale(want)).all()
    as_tensor = viz.synthesis.MLPG_GV(dev(means), dev(variances), gv_mean, gv_variance, padding_size=padding, seq_len=seq_len)
    assert isinstance(as_tensor, torch.Tensor) and as_tensor.dtype == torch.float32 and torch.equal(as_tensor, _call(key))
    single = viz.synthesis.MLPG_GV(means[0], variances, gv_mean, gv_variance, padding_size=padding)
    assert single.shape == (ref.T, ref.DIM)
    assert (np.abs(single - want[0]) <= ref.X_FLOOR * np.abs(want[0]).max(axis=0, keepdims=True)).all()
    with pytest.raises(ValueError, match='gv_variance'):
        viz.synthesis.MLPG_GV(means, variances, gv_mean, np.zeros_like(gv_variance), padding_size=padding)
    with pytest.raises(ValueError, match='gv_variance'):
        ops.mlpg_gv(dev(means), dev(variances), gv_mean, -gv_variance, windows, padding_size=padding)
    with pytest.raises(ValueError, match='max_iter'):
        _call(key, max_iter=2)


# ------------------------------------------------------------------------------------------------ 6. statistics and the model
@functools.lru_cache(maxsize=None)
def _batch_np():
    return synthetic.make_acoustic_batch(6, (30, 120), streams=(('lf0', 3, 'mse'),), seed=37, with_raw=True)


def _utterances():
    feats = _batch_np()
    return [{'name': 'utt%d' % b, 'lf0': feats['lf0'][b, :int(n)]} for b, n in enumerate(np.asarray(feats['n_frames']).reshape(-1))]


def test_fit_global_variance_files_and_values(tmp_path):
    utterances = _utterances()
    fitted = data.fit_global_variance(utterances, ['lf0'], device=DEV, out_dir='norm', data_root=str(tmp_path))
    assert sorted(fitted) == ['lf0_gv'] and os.path.exists(str(tmp_path / 'norm' / 'lf0_gv_mvn.json'))
    loaded = data.MeanVarianceNormaliser('lf0_gv')
    loaded.load_params('norm', data_root=str(tmp_path))
    per_utterance = np.stack([np.asarray(u['lf0'], np.float64).var(axis=0) for u in utterances])
    for name, want in (('mean', per_utterance.mean(axis=0)), ('std_dev', per_utterance.std(axis=0))):
        assert loaded.params[name].dtype == np.float32
        assert np.array_equal(loaded.params[name], fitted['lf0_gv'].params[name])            # bit for bit through the file
        assert (np.abs(loaded.params[name] - want) <= 1e-6 * np.abs(want)).all(), name


def _model():
    """The shipped F0 model on the synthetic weights, its last Linear times 100: with the weights as drawn the trajectory barely moves
    (variance 1e-6 against the corpus' 7.5e-2), the root then sits where A is all but singular, h is at its noise floor around the
    1e-6 rule and a third of the utterances take the fallback - which is not what this test is about."""
    model = models.GRUF0Model(precision='fp32').to(DEV)
    own = model.state_dict()
    for key, value in synthetic.gru_f0_state().items():
        own[key].copy_(torch.from_numpy(value))
    with torch.no_grad():
        model.layers[12].weight.mul_(100.)
    synthetic.acoustic_normalisers(model, device=DEV)
    model.mode = 'train'
    return model


def test_model_generates_with_and_without_gv():
    default, model = _model(), _model()
    batch = data.to_device(dict(_batch_np()), DEV, normalisers=model.normalisers)
    n_frames = batch['n_frames'].reshape(-1)
    assert 'lf0_gv' not in model.normaliser_sources()
    assert model.generate_with_gv() is model
    assert isinstance(model.normaliser_sources()['lf0_gv'], data.MeanVarianceNormaliser)
    # train() mode is untouched while the switch is on: the first step of either model, bit for bit
    loss_default, out_default = default(batch)
    loss_on, out_on = model(batch)
    assert torch.equal(loss_on, loss_default) and torch.equal(out_on['lf0'], out_default['lf0'])
    default.eval()
    model.eval()
    with torch.no_grad():
        plain = default.predict(batch)['lf0']
        with pytest.raises(KeyError, match='lf0_gv'):
            model.predict(batch)
        model.normalisers['lf0_gv'] = data.fit_global_variance(_utterances(), 'lf0', device=DEV)['lf0_gv']
        with_gv = model.predict(batch)['lf0']
        mu_v = model.normalisers['lf0_gv'].params_torch['mean'].to(DEV)
        gap_plain = (losses.global_variance(plain, n_frames) - mu_v).abs()
        gap_gv = (losses.global_variance(with_gv, n_frames) - mu_v).abs()
        print('|v - mu_v| per utterance: MLPG %s, under the prior %s' % (gap_plain.reshape(-1).tolist(), gap_gv.reshape(-1).tolist()))
        assert (gap_gv < gap_plain).all()
        assert model.generate_without_gv() is model and torch.equal(model.predict(batch)['lf0'], plain)
    assert 'lf0_gv' not in model.normaliser_sources()


def test_per_speaker_statistics_and_generation(tmp_path):
    """``speaker_id_list``: one row of statistics per speaker, written and read back as the speaker-dependent normaliser does, and a
    model built with a speaker list generates every utterance under the row of its own speaker (``features['speaker_index']``)."""
    names = synthetic.speaker_names(2)
    (tmp_path / 'speakers.scp').write_text('\n'.join(names) + '\n')
    speakers = [names[b % 2] for b in range(6)]
    utterances = [dict(u, speaker_id=spk) for u, spk in zip(_utterances(), speakers)]
    prior = data.fit_global_variance(utterances, ['lf0'], device=DEV, out_dir='norm', data_root=str(tmp_path),
                                     speaker_id_list='speakers.scp')['lf0_gv']
    assert isinstance(prior, data.SpeakerDependentMeanVarianceNormaliser) and prior.speaker_ids == names
    loaded = data.SpeakerDependentMeanVarianceNormaliser('lf0_gv', 'speakers.scp')
    loaded.load_params('norm', data_root=str(tmp_path))
    for spk in names:
        assert os.path.exists(str(tmp_path / 'norm' / spk / 'lf0_gv_mvn.json'))
        own = np.stack([np.asarray(u['lf0'], np.float64).var(axis=0) for u in utterances if u['speaker_id'] == spk])
        for key, want in (('mean', own.mean(axis=0)), ('std_dev', own.std(axis=0))):
            assert np.array_equal(loaded.params[spk][key], prior.params[spk][key])
            assert (np.abs(prior.params[spk][key] - want) <= 1e-6 * np.abs(want)).all(), (spk, key)

    model = models.GRUF0Model(precision='fp32', speaker_id_list='speakers.scp').to(DEV)
    own = model.state_dict()
    for key, value in synthetic.gru_f0_state().items():
        own[key].copy_(torch.from_numpy(value))
    with torch.no_grad():
        model.layers[12].weight.mul_(100.)               # see _model
    synthetic.speaker_acoustic_normalisers(model, n_speakers=2, device=DEV)
    model.mode = 'train'
    assert isinstance(model.generate_with_gv().normaliser_sources()['lf0_gv'], data.SpeakerDependentMeanVarianceNormaliser)
    model.normalisers['lf0_gv'] = prior
    feats = dict(_batch_np())
    feats['speaker_id'] = speakers
    batch = data.to_device(feats, DEV, normalisers=model.normalisers)
    index, n_frames = batch[data.SPEAKER_INDEX_KEY], batch['n_frames'].reshape(-1)
    assert index.cpu().tolist() == [b % 2 for b in range(6)]
    model.eval()
    with torch.no_grad():
        out = model.predict(batch)
        normaliser = model.normalisers['lf0']
        deltas = normaliser.denormalise(out['normalised_lf0_deltas'], index, deltas=True)
        std_dev = ops.item_rows(normaliser.tables(DEV, deltas=True)[1], index.to(torch.int32))
        gv_mean, gv_std = (ops.item_rows(table, index.to(torch.int32)) for table in prior.tables(DEV))
        by_hand = ops.mlpg_gv(deltas, std_dev ** 2, gv_mean, gv_std ** 2, viz.synthesis.DEFAULT_WINDOWS, padding_size=100, seq_len=n_frames)
        assert torch.equal(out['lf0'], by_hand)
        plain = model.generate_without_gv().predict(batch)['lf0']
        gap_plain = (losses.global_variance(plain, n_frames) - gv_mean).abs()
        gap_gv = (losses.global_variance(out['lf0'], n_frames) - gv_mean).abs()
        assert (gap_gv < gap_plain).all()
