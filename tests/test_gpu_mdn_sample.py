"""losses.mdn_sample / ops.mdn_sample on the device (csrc/mdn.hip, mg_mdn_sample_f32): the draw against the float64 restatement of
its Philox mapping, choice rule and moments (tests/mdn_sample_ref64.py: the component on every decided frame, a neighbour of the
boundary on the others, mean and variance inside the derived fp32 bounds), the exact temperature identities, the component
frequencies, the edge cases, column slices, the counter scheme with graph replay, the caps, and the mixture-density streams of
models.StreamModel in eval() and train() mode."""
import ctypes

import numpy as np
import pytest
import torch

import mdn_ref64
import mdn_sample_ref64 as ref
import parity_report
import sampling_ref64
from morgana_amd import _lib, data, losses, models, ops, optim, synthetic, viz

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SEED, CTR = ref.SEED, ref.CTR
_DRAWS = {}


def _counter(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def _philox(counter, key):
    c, k, out = (ctypes.c_uint32 * 4)(*counter), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
    _lib.load().mg_philox4x32_10(c, k, out)
    return [int(v) for v in out]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _draws(k, d):
    """The case's input, uniforms and float64 noise at (SEED, CTR), computed once and shared (never modified)."""
    if (k, d) not in _DRAWS:
        pred, seq_len = ref.case(k, d)
        b, t, _ = pred.shape
        u = ref.component_uniforms(b * t, SEED, ops.MDN_COMPONENT_SITE, CTR, _philox).reshape(b, t)
        noise = sampling_ref64.normal_noise(b * t, d, SEED, ops.MDN_NOISE_SITE, CTR, _philox).reshape(b, t, d)
        _DRAWS[(k, d)] = (pred, seq_len, u, noise)
    return _DRAWS[(k, d)]


def _sample(pred, seq_len, k, d, **kwargs):
    """ops.mdn_sample at (SEED, CTR) on numpy or device inputs -> three numpy arrays."""
    x = pred if torch.is_tensor(pred) else _dev(pred)
    n = seq_len if seq_len is None or torch.is_tensor(seq_len) else _dev(seq_len)
    return tuple(v.cpu().numpy() for v in ops.mdn_sample(x, n, k, d, SEED, _counter(CTR), **kwargs))


# ------------------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize('temperature', ref.TEMPERATURES)
@pytest.mark.parametrize('k, d', sorted(ref.CASES))
def test_against_the_restatement(k, d, temperature):
    pred, seq_len, u, noise = _draws(k, d)
    x, n = _dev(pred), _dev(seq_len)
    for noise_scale in (0.0, 1.0):
        want = ref.sample(pred, seq_len, k, d, u, noise, temperature=temperature, noise_scale=noise_scale)
        mask, decided = want['mask'], want['decided']
        component, mean, variance = _sample(x, n, k, d, temperature=temperature, noise_scale=noise_scale)
        assert component.dtype == np.int64 and component.shape == pred.shape[:2] and mean.shape == variance.shape == pred.shape[:2] + (d,)
        undecided = int((~decided & mask).sum())
        assert undecided <= ref.UNDECIDED_CAP * mask.sum(), (undecided, int(mask.sum()))
        assert np.array_equal(component[decided], want['component'][decided])          # pad frames are decided: 0
        assert np.all((want['lowest'] <= component) & (component <= want['highest']))  # undecided: next to the boundary
        assert np.all(np.take_along_axis(want['live'], component[:, :, None], axis=2)[mask])
        if k == 1:
            assert np.all(component == 0)
        mean_w, mean_b, var_w, var_b = want['moments'](component)
        mean_err, var_err = np.abs(mean.astype(np.float64) - mean_w), np.abs(variance.astype(np.float64) - var_w)
        if noise_scale == 0.0:
            assert np.array_equal(mean.astype(np.float64), mean_w)                     # exact copies of the chosen component's mu
        else:
            worst = float((mean_err / np.maximum(mean_b, 1e-300))[mask].max())
            parity_report.note(worst, 'K=%d D=%d T=%g: mean err / derived bound' % (k, d, temperature), bound=1.0)
            print('K=%d D=%d temperature=%g: noisy mean at %.3f of its bound' % (k, d, temperature, worst))
            assert np.all(mean_err <= mean_b), worst
        worst_v = float((var_err / np.maximum(var_b, 1e-300))[mask].max())
        parity_report.note(worst_v, 'K=%d D=%d T=%g: variance err / derived bound' % (k, d, temperature), bound=1.0)
        print('K=%d D=%d temperature=%g noise_scale=%g: %d undecided of %d, %d differ from float64, variance at %.3f of its bound'
              % (k, d, temperature, noise_scale, undecided, int(mask.sum()), int((component != want['component']).sum()), worst_v))
        assert np.all(var_err <= var_b), worst_v
        assert np.all(component[~mask] == 0) and np.all(mean[~mask] == 0.0) and np.all(variance[~mask] == 1.0)


def test_noise_moves_the_mean_by_its_standard_deviation():
    """noise_scale = 1 is a draw from the chosen Gaussian: (mean - mu) / sigma over every element of the largest case is N(0, 1)."""
    k, d = 64, 3
    pred, seq_len, u, noise = _draws(k, d)
    component, mean, variance = _sample(pred, seq_len, k, d, noise_scale=1.0)
    _, plain, _ = _sample(pred, seq_len, k, d)
    mask = np.arange(pred.shape[1])[None, :] < seq_len[:, None]
    z = ((mean.astype(np.float64) - plain) / np.sqrt(variance.astype(np.float64)))[mask].ravel()
    n = z.size
    assert n >= 6000 and abs(z.mean()) <= 5 / np.sqrt(n) and abs((z * z).mean() - 1.0) <= 5 * np.sqrt(2.0 / n)
    # another scale: the same noise, half the step - inside the restatement's bound at noise_scale = 0.5
    half = _sample(pred, seq_len, k, d, noise_scale=0.5)
    mean_w, mean_b, _, _ = ref.sample(pred, seq_len, k, d, u, noise, noise_scale=0.5)['moments'](half[0])
    assert np.array_equal(half[0], component) and np.all(np.abs(half[1].astype(np.float64) - mean_w) <= mean_b)


# --------------------------------------------------------------------------------------------------------------- 2. temperature
@pytest.mark.parametrize('k, d', [(8, 3), (64, 3)])
@pytest.mark.parametrize('temperature', [0.5, 2.0])
def test_temperature_is_a_scaling_of_the_logits(k, d, temperature):
    """1 / temperature is a power of two: multiplying the logits by it is exact in fp32, and so is (a - max a) * inv_temperature =
    a' - max a'.  Same seed and counter: the same components."""
    pred, seq_len, u, _ = _draws(k, d)
    scaled = pred.copy()
    scaled[:, :, :k] *= np.float32(1.0 / temperature)
    tempered = _sample(pred, seq_len, k, d, temperature=temperature)
    plain = _sample(scaled, seq_len, k, d, temperature=1.0)
    decided = ref.sample(pred, seq_len, k, d, u, temperature=temperature)['decided']
    assert np.array_equal(tempered[0][decided], plain[0][decided])
    assert np.array_equal(tempered[0], plain[0]) and np.array_equal(tempered[1], plain[1])     # in fact the same arithmetic: every frame
    other = _sample(pred, seq_len, k, d, temperature=1.0)
    assert not np.array_equal(other[0], tempered[0])


# --------------------------------------------------------------------------------------------------------------- 3. frequencies
@pytest.mark.parametrize('k', [8, 64])
def test_component_frequencies(k):
    pred, p = ref.frequency_case(k)
    b, t, _ = pred.shape
    n = b * t
    component, mean, _ = _sample(pred, None, k, 1)
    assert np.array_equal(mean[:, :, 0], component.astype(np.float32))                # the means of this input ARE the component indices
    share = np.bincount(component.ravel(), minlength=k) / n
    worst = np.abs(share - p) / ref.frequency_bound(p, n)
    print('K=%d: worst |f - p| / (5 sigma + 1 / N) = %.3f' % (k, worst.max()))
    parity_report.note(float(worst.max()), 'K=%d: |f - p| / (5 sigma + 1 / N)' % k, bound=1.0)
    assert component.min() >= 0 and component.max() < k and np.all(worst <= 1.0)


# ---------------------------------------------------------------------------------------------------------------- 4. edge cases
def test_a_minus_inf_logit_is_never_drawn():
    k, d, b, t = 8, 3, 8, 512                                                          # 4096 frames
    rng = np.random.RandomState(5)
    pred = rng.standard_normal((b, t, mdn_ref64.width(k, d))).astype(np.float32)
    others = np.delete(pred[:, :, :k].astype(np.float64), 3, axis=2)
    pred[:, :, 3] = np.log(np.exp(others).sum(axis=2)).astype(np.float32)              # component 3 holds half the mass of every frame
    with_it = _sample(pred, None, k, d)[0]
    assert 0.45 < (with_it == 3).mean() < 0.55
    pred[:, :, 3] = -np.inf
    for temperature in (0.5, 1.0, 2.0):
        component = _sample(pred, None, k, d, temperature=temperature)[0]
        assert not np.any(component == 3) and len(np.unique(component)) == k - 1
    pred[:, :, 4:k] = -np.inf                                                         # the LAST live component is 2: the fallback's range
    component = _sample(pred, None, k, d)[0]
    assert set(np.unique(component)) == {0, 1, 2}


def test_all_logits_minus_inf_give_the_selected_component():
    k, d = 8, 3
    pred, seq_len, _, _ = _draws(k, d)
    gone = pred.copy()
    gone[0, 5, :k] = -np.inf
    gone[1, 30, :k] = -np.inf                                                          # a pad frame: not read
    x, n = _dev(gone), _dev(seq_len)
    clean = _sample(pred, seq_len, k, d, noise_scale=1.0)
    got = _sample(x, n, k, d, noise_scale=1.0)
    selected = ops.mdn_select(x, n, k, d)
    assert got[0][0, 5] == selected[0][0, 5].item() == 0
    assert np.array_equal(got[2][0, 5], selected[2][0, 5].cpu().numpy()) and np.isfinite(got[1]).all()
    keep = np.ones(pred.shape[:2], dtype=bool)
    keep[0, 5] = False
    for a, c in zip(got, clean):
        assert np.array_equal(a[keep], c[keep])


def test_pad_frames_are_not_read_and_hold_0_0_1():
    for k, d in ((8, 3), (4, 180)):
        pred, seq_len, _, _ = _draws(k, d)
        mask = np.arange(pred.shape[1])[None, :] < seq_len[:, None]
        dirty = pred.copy()
        dirty[~mask] = np.nan
        clean, got = _sample(pred, seq_len, k, d, noise_scale=1.0), _sample(dirty, seq_len, k, d, noise_scale=1.0)
        for a, c in zip(got, clean):
            assert np.array_equal(a, c)
        assert np.all(got[0][~mask] == 0) and np.all(got[1][~mask] == 0.0) and np.all(got[2][~mask] == 1.0)
        clamped = _sample(pred, np.array([99, 20, 1], dtype=np.int64), k, d, noise_scale=1.0)   # seq_len > T is clamped
        for a, c in zip(clamped, clean):
            assert np.array_equal(a, c)


@pytest.mark.parametrize('k, d', [(8, 3), (4, 180)])
def test_floor(k, d):
    pred, seq_len, u, noise = _draws(k, d)
    plain = _sample(pred, seq_len, k, d)
    floored = _sample(pred, seq_len, k, d, min_log_std=-0.5)
    want = ref.sample(pred, seq_len, k, d, u, noise, min_log_std=-0.5)
    mask = want['mask']
    assert np.array_equal(floored[0], plain[0]) and np.array_equal(floored[1], plain[1])      # the floor touches no choice and no mean
    _, _, var_w, var_b = want['moments'](floored[0])
    assert np.all(np.abs(floored[2].astype(np.float64) - var_w) <= var_b)
    assert floored[2][mask].min() >= np.float32(np.exp(-1.0)) * (1 - 1e-6) and plain[2][mask].min() < np.exp(-1.0)
    # with noise the step is noise_scale * exp(max(s, floor)) * g: inside the floored restatement's bound, different from the unfloored
    noisy = _sample(pred, seq_len, k, d, min_log_std=-0.5, noise_scale=1.0)
    want_n = ref.sample(pred, seq_len, k, d, u, noise, min_log_std=-0.5, noise_scale=1.0)
    mean_w, mean_b, _, _ = want_n['moments'](noisy[0])
    assert np.all(np.abs(noisy[1].astype(np.float64) - mean_w) <= mean_b)
    assert not np.array_equal(noisy[1], _sample(pred, seq_len, k, d, noise_scale=1.0)[1])
    selected = ops.mdn_select(_dev(pred), _dev(seq_len), k, d, min_log_std=-0.5)[2].cpu().numpy()
    same = floored[0] == ops.mdn_select(_dev(pred), _dev(seq_len), k, d)[0].cpu().numpy()
    assert np.array_equal(floored[2][same & mask], selected[same & mask])                      # mdn_select's arithmetic


# --------------------------------------------------------------------------------------------------------------------- 5. layout
@pytest.mark.parametrize('k, d', [(8, 3), (2, 65), (4, 180), (16, 1024)])
def test_column_slice_and_no_seq_len(k, d):
    pred, seq_len, _, _ = _draws(k, d)
    b, t, w = pred.shape
    x, n = _dev(pred), _dev(seq_len)
    wide = torch.cat((torch.full((b, t, 7), 9.0, device=DEV), x, torch.full((b, t, 2), -9.0, device=DEV)), dim=2)
    view = wide[:, :, 7:7 + w]
    assert not view.is_contiguous()
    want = ops.mdn_sample(x, n, k, d, SEED, _counter(CTR), noise_scale=1.0)
    by_col0 = ops.mdn_sample(wide, n, k, d, SEED, _counter(CTR), noise_scale=1.0, col0=7)
    by_view = ops.mdn_sample(view, n, k, d, SEED, _counter(CTR), noise_scale=1.0)
    for got in (by_col0, by_view):
        assert all(torch.equal(g, a) for g, a in zip(got, want))
    assert torch.equal(wide[:, :, 7:7 + w], x)                                          # the prediction itself is only read
    # through losses.mdn_sample on the view: the draw of the device counter, made explicit
    state = ops.dropout_state(DEV)
    before = int(state.item())
    through = losses.mdn_sample(view, k, d, seq_len=n, noise_scale=1.0)
    again = ops.mdn_sample(x, n, k, d, ops.dropout_seed(), _counter(before), noise_scale=1.0)
    assert int(state.item()) == before + 1 and all(torch.equal(g, a) for g, a in zip(through, again))
    assert not through[1].requires_grad and not through[2].requires_grad
    # seq_len=None: every frame is drawn, and a frame's draw does not depend on seq_len
    full = ops.mdn_sample(x, None, k, d, SEED, _counter(CTR), noise_scale=1.0)
    valid = torch.arange(t, device=DEV)[None, :] < n[:, None]
    for g, a in zip(full, want):
        assert torch.equal(g[valid], a[valid])
    assert not torch.all(full[2][~valid] == 1.0)
    lengths = ops.mdn_sample(x, torch.full((b,), t, dtype=torch.int64, device=DEV), k, d, SEED, _counter(CTR), noise_scale=1.0)
    assert all(torch.equal(g, a) for g, a in zip(full, lengths))


# ------------------------------------------------------------------------------------------------------------ 6. counter scheme
def test_counters_sites_and_seed(monkeypatch):
    k, d = 8, 3
    pred, seq_len, _, _ = _draws(k, d)
    x, n = _dev(pred), _dev(seq_len)

    def draw(seed=SEED, ctr=CTR, **kwargs):
        return ops.mdn_sample(x, n, k, d, seed, _counter(ctr), **kwargs)

    a = draw(noise_scale=1.0)
    assert all(torch.equal(g, w) for g, w in zip(a, draw(noise_scale=1.0)))            # the same (seed, used): the same bits
    for other in (draw(ctr=CTR + 1, noise_scale=1.0), draw(ctr=CTR + (1 << 32), noise_scale=1.0), draw(seed=SEED ^ 1, noise_scale=1.0),
                  draw(seed=SEED ^ (1 << 40), noise_scale=1.0)):
        assert not torch.equal(a[0], other[0]) and not torch.equal(a[1], other[1])
    # two sites, independent streams: the noise changes no component (and no variance), the component site no noise
    for noise_scale in (0.0, 0.5, 3.0):
        b_ = draw(noise_scale=noise_scale)
        assert torch.equal(a[0], b_[0]) and torch.equal(a[2], b_[2]) and (noise_scale == 0.0 or not torch.equal(a[1], b_[1]))
    assert len({ops.SAMPLE_SITE, ops.SPHERE_SITE, ops.ELLIPSOID_SITE, ops.MDN_COMPONENT_SITE, ops.MDN_NOISE_SITE}) == 5
    monkeypatch.setattr(ops, 'MDN_NOISE_SITE', ops.MDN_NOISE_SITE + 1)
    moved = draw(noise_scale=1.0)
    assert torch.equal(moved[0], a[0]) and not torch.equal(moved[1], a[1])
    monkeypatch.undo()
    monkeypatch.setattr(ops, 'MDN_COMPONENT_SITE', ops.MDN_COMPONENT_SITE + 1)
    moved = draw(noise_scale=1.0)
    assert not torch.equal(moved[0], a[0])
    monkeypatch.undo()
    # losses.mdn_sample: ONE draw of the device counter per call, new draws every call, torch.manual_seed makes a run repeatable
    state = ops.dropout_state(DEV)
    keep_seed = torch.initial_seed()
    try:
        runs = []
        for seed in (5, 5, 6):
            torch.manual_seed(seed)
            state.zero_()
            first = losses.mdn_sample(x, k, d, seq_len=n, noise_scale=1.0)
            second = losses.mdn_sample(x, k, d, seq_len=n, noise_scale=1.0)
            assert int(state.item()) == 2
            runs.append((first, second))
        assert all(torch.equal(g, w) for g, w in zip(runs[0][0], runs[1][0])) and all(torch.equal(g, w) for g, w in zip(runs[0][1], runs[1][1]))
        assert not torch.equal(runs[0][0][0], runs[2][0][0]) and not torch.equal(runs[0][0][1], runs[2][0][1])
        assert not torch.equal(runs[0][0][0], runs[0][1][0]) and not torch.equal(runs[0][0][1], runs[0][1][1])   # two calls differ
    finally:
        torch.manual_seed(keep_seed)


def test_graph_replay_draws_new_components():
    k, d = 8, 3
    pred, seq_len, _, _ = _draws(k, d)
    x, n = _dev(pred), _dev(seq_len)
    state = ops.dropout_state(DEV)
    losses.mdn_sample(x, k, d, seq_len=n, noise_scale=1.0)                             # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = losses.mdn_sample(x, k, d, seq_len=n, noise_scale=1.0)
    before = int(state.item())
    graph.replay()
    first = [v.clone() for v in out]
    graph.replay()
    second = [v.clone() for v in out]
    torch.cuda.synchronize()
    assert int(state.item()) == before + 2
    assert not torch.equal(first[0], second[0]) and not torch.equal(first[1], second[1])
    for replay, ctr in ((first, before), (second, before + 1)):                        # each replay IS the eager draw at its counter
        want = ops.mdn_sample(x, n, k, d, ops.dropout_seed(), _counter(ctr), noise_scale=1.0)
        assert all(torch.equal(g, w) for g, w in zip(replay, want))


# ----------------------------------------------------------------------------------------------------------------------- 7. caps
def test_caps_are_refused_before_any_launch():
    used = _counter(CTR)
    ops.dropout_state(DEV)
    calls = _lib.CALL_LOG = []
    try:
        with pytest.raises(_lib.MorganaHipError, match='cap of 64'):
            ops.mdn_sample(torch.zeros(1, 2, 65 * 3, device=DEV), None, 65, 1, SEED, used)
        with pytest.raises(_lib.MorganaHipError, match='cap of 16384'):
            ops.mdn_sample(torch.zeros(1, 2, 2 * 16385 + 1, device=DEV), None, 1, 16385, SEED, used)
        with pytest.raises(_lib.MorganaHipError, match='cap of 64'):
            losses.mdn_sample(torch.zeros(1, 2, 65 * 3, device=DEV), 65, 1)
        with pytest.raises(_lib.MorganaHipError, match='cap of 16384'):
            losses.mdn_sample(torch.zeros(1, 2, 2 * 16385 + 1, device=DEV), 1, 16385)
        with pytest.raises(ValueError, match='do not fit'):
            ops.mdn_sample(torch.zeros(1, 2, 30, device=DEV), None, 4, 3, SEED, used, col0=3)
        with pytest.raises(ValueError, match='do not fit'):
            ops.mdn_sample(torch.zeros(1, 2, 30, device=DEV), None, 4, 3, SEED, used, col0=-1)
        for temperature in (0, 0.0, -1.0, float('nan'), float('inf')):
            with pytest.raises(ValueError, match='temperature'):
                ops.mdn_sample(torch.zeros(1, 2, 28, device=DEV), None, 4, 3, SEED, used, temperature=temperature)
            with pytest.raises(ValueError, match='temperature'):
                losses.mdn_sample(torch.zeros(1, 2, 28, device=DEV), 4, 3, temperature=temperature)
        with pytest.raises(ValueError, match='mdn_select'):
            losses.mdn_sample(torch.zeros(1, 2, 28, device=DEV), 4, 3, temperature=0)
        with pytest.raises(ValueError, match='noise_scale'):
            losses.mdn_sample(torch.zeros(1, 2, 28, device=DEV), 4, 3, noise_scale=-1.0)
        assert calls == []                                                             # no entry point was reached, no counter drawn
    finally:
        _lib.CALL_LOG = None


# ---------------------------------------------------------------------------------------------------------------------- 8. model
K_MODEL, D_MODEL = 8, 3
STREAMS = (('lf0', D_MODEL, 'mse'), ('vuv', 1, 'sigmoid_bce'))


def _batch():
    return data.to_device(synthetic.make_acoustic_batch(2, (30, 40), streams=STREAMS, seed=71, with_raw=True), DEV)


def _f0_model(seed=11, mode='valid', **kwargs):
    torch.manual_seed(seed)
    model = models.GRUF0Model(n_components=K_MODEL, precision='fp32', **kwargs).to(DEV)
    synthetic.acoustic_normalisers(model, device=DEV)
    model.mode = mode
    model.metrics.reset_state(mode)
    return model


def test_model_predicts_a_new_trajectory_on_every_call():
    feats = _batch()
    n = feats['n_frames']
    model, twin = _f0_model().eval(), _f0_model().eval()
    assert model.sample_mixtures() is model
    with torch.no_grad():
        first, second, selected = model.predict(feats), model.predict(feats), twin.predict(feats)
    assert set(first) == set(selected) | {'lf0_component'} == {'lf0_mdn', 'lf0_component', 'normalised_lf0_deltas',
                                                                'normalised_lf0_deltas_variance', 'lf0'}
    for out in (first, second):
        assert tuple(out['lf0'].shape) == tuple(feats['lf0'].shape) and torch.isfinite(out['lf0']).all()
        assert out['lf0_component'].dtype == torch.int64 and tuple(out['lf0_component'].shape) == tuple(out['lf0'].shape[:2])
        assert 0 <= out['lf0_component'].min().item() and out['lf0_component'].max().item() < K_MODEL
        variance = out['normalised_lf0_deltas_variance']
        assert torch.isfinite(variance).all() and variance.min().item() > 0.0
        assert torch.equal(out['lf0_mdn'], selected['lf0_mdn'])                        # what the loss reads is untouched
        # the trajectory IS MLPG on the sampled mean under the sampled per-frame variances
        normaliser = model.normalisers['lf0']
        std_dev = normaliser.delta_params_torch['std_dev'].to(device=DEV, dtype=torch.float32)
        by_hand = ops.mlpg(normaliser.denormalise(out['normalised_lf0_deltas'], deltas=True), variance * std_dev ** 2,
                           viz.synthesis.DEFAULT_WINDOWS, padding_size=100, seq_len=n)
        assert torch.equal(out['lf0'], by_hand)
    assert not torch.equal(first['lf0_component'], second['lf0_component']) and not torch.equal(first['lf0'], second['lf0'])
    assert not torch.equal(first['lf0'], selected['lf0'])
    # temperature and noise reach the kernel: the draw of this call, restated through ops at the counter it used
    model.sample_mixtures(temperature=0.5, noise_scale=1.0)
    state = ops.dropout_state(DEV)
    before = int(state.item())
    with torch.no_grad():
        out = model.predict(feats)
    want = ops.mdn_sample(out['lf0_mdn'], n.reshape(-1), K_MODEL, D_MODEL, ops.dropout_seed(), _counter(before), temperature=0.5, noise_scale=1.0)
    assert int(state.item()) == before + 1
    assert torch.equal(out['lf0_component'], want[0]) and torch.equal(out['normalised_lf0_deltas'], want[1])
    # eval-mode forward: the loss reads <name>_mdn and is the twin's, the metrics read the sampled trajectory
    with torch.no_grad():
        loss, out = model(feats)
        loss_twin, _ = twin(feats)
    assert torch.equal(loss, loss_twin) and 'lf0_component' in out
    assert np.isfinite(model.metrics.results_as_json_dict('valid')['LF0_RMSE_Hz'])
    # select_mixtures: bit-equal to the untouched twin again
    model.select_mixtures()
    with torch.no_grad():
        back = model.predict(feats)
    assert set(back) == set(selected) and all(torch.equal(back[key], selected[key]) for key in selected)


def test_training_mode_ignores_the_setting():
    from morgana_amd import graphs
    feats = _batch()
    model, twin = _f0_model(mode='train'), _f0_model(mode='train')
    model.sample_mixtures(temperature=2.0, noise_scale=1.0)
    assert model.training and twin.training
    state = ops.dropout_state(DEV)
    before = int(state.item())
    loss, out = model(feats)
    loss_twin, out_twin = twin(feats)
    loss.backward()
    loss_twin.backward()
    assert int(state.item()) == before                                                 # nothing was drawn
    assert torch.equal(loss, loss_twin) and set(out) == set(out_twin)
    assert all(torch.equal(out[key], out_twin[key]) for key in out_twin)
    for (name, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p.grad, q.grad), name
    # a graphed training step: the same replays
    results = []
    for sampling in (True, False):
        fresh = _f0_model(mode='train')
        if sampling:
            fresh.sample_mixtures(temperature=2.0, noise_scale=1.0)
        opt = optim.Adam(fresh.parameters(), lr=0.01)
        step = graphs.GraphedTrainStep(fresh, opt, feats, warmup=2)
        results.append(([step().clone() for _ in range(3)], opt.flat_buffers()))
    for a, b in zip(results[0][0], results[1][0]):
        assert torch.equal(a, b)
    for key in ('param', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(results[0][1][key], results[1][1][key]), key


def test_models_without_a_mixture_stream_refuse():
    torch.manual_seed(3)
    plain = models.GRUF0Model(precision='fp32').to(DEV)
    with pytest.raises(ValueError, match="no 'mdn' stream"):
        plain.sample_mixtures()
    assert plain._mixture_sampling is None


def test_speaker_dependent_trajectory_takes_the_sampled_variances():
    feats = _batch()
    names, rows = synthetic.speaker_batch_ids(2, n_speakers=3, seed=5)
    feats['speaker_id'], feats[data.SPEAKER_INDEX_KEY] = names, torch.from_numpy(rows).to(DEV)
    torch.manual_seed(9)
    model = models.GRUF0Model(n_components=K_MODEL, speaker_id_list=synthetic.speaker_names(3), precision='fp32').to(DEV)
    synthetic.speaker_acoustic_normalisers(model, n_speakers=3, device=DEV)
    model.mode = 'valid'
    model.metrics.reset_state('valid')
    model.eval().sample_mixtures(noise_scale=1.0)
    with torch.no_grad():
        loss, outputs = model(feats)
        _, again = model(feats)
    assert np.isfinite(loss.item()) and not torch.equal(outputs['lf0'], again['lf0'])
    normaliser, n = model.normalisers['lf0'], feats['n_frames']
    mean, variance = outputs['normalised_lf0_deltas'], outputs['normalised_lf0_deltas_variance']
    index = normaliser.speaker_index(feats[data.SPEAKER_INDEX_KEY], DEV)
    std_dev = ops.item_rows(normaliser.tables(DEV, deltas=True)[1], index)
    by_hand = ops.mlpg(normaliser.denormalise(mean, feats[data.SPEAKER_INDEX_KEY], deltas=True), variance * (std_dev ** 2)[:, None, :],
                       viz.synthesis.DEFAULT_WINDOWS, padding_size=100, seq_len=n)
    assert torch.equal(outputs['lf0'], by_hand) and 'lf0_component' in outputs
