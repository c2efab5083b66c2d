"""Speaker-dependent normalisers on the device (run with ``-m gpu`` on an MI355X): the per-item kernels against the reference's
outputs (tests/golden/g17_speaker_normalisers.npz), against the shared kernel bit for bit, their gradient, the device loader, the
guard on the row index, MLPG's per-item variances, the shipped F0 model with per-speaker parameters and graph replay with speakers
that change from batch to batch."""
import os
import warnings

import numpy as np
import pytest
import torch

from morgana_amd import data, graphs, metrics, models, ops, optim, synthetic, viz
from morgana_amd import functional as F_hip

from test_speaker_normalisers_host import KINDS, TOL, _names, _normaliser

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
OP_KINDS = {'norm_mvn': ops.NORM_MVN, 'denorm_mvn': ops.DENORM_MVN, 'norm_minmax': ops.NORM_MINMAX, 'denorm_minmax': ops.DENORM_MINMAX}


def _close(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    print('%s: max abs difference %.3e' % (what, float(np.max(np.abs(got - want))) if got.size else 0.0))
    np.testing.assert_allclose(got, want, err_msg=what, **TOL)


@pytest.mark.parametrize('kind', ['mvn', 'minmax'])
@pytest.mark.parametrize('group', ['static', 'deltas'])
def test_device_path_equals_the_reference(golden, kind, group):
    g = golden('g17_speaker_normalisers.npz')
    normaliser, deltas, key = _normaliser(g, kind, device=DEV), group == 'deltas', '%s__%s__' % (kind, group)
    batch, single = _names(g, 'batch_speakers'), _names(g, 'single_speaker')[0]
    x = torch.from_numpy(g['x__' + group]).to(DEV)
    index = torch.tensor(normaliser.speaker_rows(batch), dtype=torch.int32, device=DEV)
    for who, label in ((batch, 'names'), (index, 'index'), (index.to(torch.int64), 'int64 index')):
        _close(normaliser.normalise(x, who, deltas=deltas), g[key + 'torch_norm'], '%s normalise by %s' % (key, label))
        _close(normaliser.denormalise(x, who, deltas=deltas), g[key + 'torch_denorm'], '%s denormalise by %s' % (key, label))
    x1 = torch.from_numpy(g['x_single__' + group]).to(DEV)
    got = normaliser.normalise(x1, single, deltas=deltas)
    assert tuple(got.shape) == tuple(x1.shape)
    _close(got, g[key + 'single_norm'], key + ' single sequence')
    with pytest.raises(KeyError):
        normaliser.normalise(x, ['p1', 'nobody', 'p2', 'p3'], deltas=deltas)
    with pytest.raises(ValueError):
        normaliser.normalise(x, batch[:2], deltas=deltas)


@pytest.mark.parametrize('kind', sorted(OP_KINDS))
@pytest.mark.parametrize('dim', [8, 7])                   # 8: the 16-byte path; 7: element by element
def test_one_speaker_is_bit_equal_to_the_shared_kernel(kind, dim):
    rng = np.random.RandomState(5 + dim)
    p0 = rng.standard_normal((3, dim)).astype(np.float32)
    p1 = (p0 + rng.uniform(0.2, 1.5, (3, dim))).astype(np.float32)
    p1[:, 2] = p0[:, 2] if 'minmax' in kind else 0.0      # a zero range / a zero standard deviation
    x = torch.from_numpy(rng.standard_normal((5, 1037, dim)).astype(np.float32) * 3).to(DEV)
    t0, t1 = torch.from_numpy(p0).to(DEV), torch.from_numpy(p1).to(DEV)
    for speaker in range(3):
        rows = torch.full((5,), speaker, dtype=torch.int32, device=DEV)
        got = ops.normalise_items(x, t0, t1, rows, OP_KINDS[kind])
        want = ops.normalise(x, t0[speaker].contiguous(), t1[speaker].contiguous(), OP_KINDS[kind])
        assert torch.equal(got, want), (kind, dim, speaker, float((got - want).abs().max()))
    # a view that is not 16-byte aligned takes the element path and gives the same bits
    if dim == 8:
        flat = torch.zeros(x.numel() + 1, dtype=torch.float32, device=DEV)
        shifted = flat[1:].view(x.shape)
        shifted.copy_(x)
        rows = torch.full((5,), 1, dtype=torch.int32, device=DEV)
        assert shifted.data_ptr() % 16 != 0
        assert torch.equal(ops.normalise_items(shifted, t0, t1, rows, OP_KINDS[kind]), ops.normalise_items(x, t0, t1, rows, OP_KINDS[kind]))


@pytest.mark.parametrize('kind', ['mvn', 'minmax'])
def test_gradient_equals_torch_autograd(golden, kind):
    g = golden('g17_speaker_normalisers.npz')
    normaliser = _normaliser(g, kind, device=DEV)
    batch = _names(g, 'batch_speakers')
    rows = normaliser.speaker_rows(batch)
    p0 = torch.from_numpy(g['%s__deltas__p0' % kind])[rows][:, None, :]
    p1 = torch.from_numpy(g['%s__deltas__p1' % kind])[rows][:, None, :]
    x_host = torch.from_numpy(g['x__deltas'])
    weight = torch.from_numpy(np.random.RandomState(9).standard_normal(x_host.shape).astype(np.float32))
    for inverse in (False, True):
        x_cpu = x_host.clone().requires_grad_(True)
        if kind == 'mvn':
            y_cpu = x_cpu * p1 + p0 if inverse else (x_cpu - p0) / (p1 + 1e-8)
        else:
            scale = p1 - p0
            scale = torch.where(scale.abs() <= 1e-8, torch.ones_like(scale), scale)
            y_cpu = x_cpu * scale + p0 if inverse else (x_cpu - p0) / scale
        (y_cpu * weight).sum().backward()
        x_dev = x_host.clone().to(DEV).requires_grad_(True)
        y_dev = (normaliser.denormalise if inverse else normaliser.normalise)(x_dev, batch, deltas=True)
        (y_dev * weight.to(DEV)).sum().backward()
        _close(y_dev, y_cpu.detach().numpy(), '%s inverse=%s forward' % (kind, inverse))
        _close(x_dev.grad, x_cpu.grad.numpy(), '%s inverse=%s gradient' % (kind, inverse))


def test_collate_to_device_equals_the_host_pipeline(golden, tmp_path):
    g = golden('g17_speaker_normalisers.npz')
    root, rng = str(tmp_path), np.random.RandomState(21)
    speakers = _names(g, 'speakers')
    normalisers = {'feat': _normaliser(g, 'mvn', device=DEV, use_deltas=False),
                   'other': _normaliser(g, 'minmax', device=DEV, use_deltas=False)}
    lengths, who = [13, 40, 7, 40, 1, 29], ['p3', 'p1', 'p1', 'p2', 'p3', 'p2']
    for name in ('feat', 'other', 'speaker_id', 'n_frames'):
        os.makedirs(os.path.join(root, 'train', name))
    for i, (n, speaker) in enumerate(zip(lengths, who)):
        for name in ('feat', 'other'):
            np.save(os.path.join(root, 'train', name, 'utt%d.npy' % i), (rng.standard_normal((n, 3)) * 2).astype(np.float32))
        for name, text in (('speaker_id', speaker), ('n_frames', str(n))):
            with open(os.path.join(root, 'train', name, 'utt%d.txt' % i), 'w') as f:
                f.write(text + '\n')
    with open(os.path.join(root, 'ids.scp'), 'w') as f:
        f.write('\n'.join('utt%d' % i for i in range(len(lengths))) + '\n')
    sources = {'feat': data.NumpyBinarySource('feat'), 'other': data.NumpyBinarySource('other'),
               'speaker_id': data.StringSource('speaker_id'), 'n_frames': data.TextSource('n_frames')}
    dataset = data.FilesDataset(sources, 'train', 'ids.scp', normalisers, data_root=root)
    want = data.to_device(data.collate_fn([dataset[i] for i in range(len(dataset))]), DEV, normalisers=normalisers)
    got = data.collate_to_device([dataset.raw(i) for i in range(len(dataset))], normalisers, DEV)
    assert got['speaker_id'] == want['speaker_id'] == who
    for batch in (got, want):
        index = batch['speaker_index']
        assert index.is_cuda and index.dtype == torch.int32 and index.tolist() == [speakers.index(s) for s in who]
    assert torch.equal(got['n_frames'], want['n_frames']) and got['n_frames_total'] == sum(lengths)
    for name in ('feat', 'other'):
        assert torch.equal(got[name], want[name])
        assert tuple(got['normalised_' + name].shape) == (len(lengths), max(lengths), 3)
        _close(got['normalised_' + name], want['normalised_' + name].cpu().numpy(), 'loader normalised_' + name)
    # the loader class end to end (two batches, the second one smaller)
    batches = list(data.DeviceBatches(dataset, 4, normalisers, DEV))
    assert [b['speaker_index'].tolist() for b in batches] == [[speakers.index(s) for s in who[:4]], [speakers.index(s) for s in who[4:]]]
    _close(batches[1]['normalised_feat'], want['normalised_feat'][4:, :29].cpu().numpy(), 'second batch')


def test_a_row_index_outside_the_tables_gives_nan_not_a_read(golden):
    """The kernels guard the index (nothing is provoked: no table element is addressed with it)."""
    g = golden('g17_speaker_normalisers.npz')
    normaliser = _normaliser(g, 'mvn', device=DEV)
    p0, p1 = normaliser.tables(DEV, deltas=True)
    n_speakers = p0.shape[0]
    x = torch.from_numpy(g['x__deltas']).to(DEV)
    good = torch.tensor([1, 0, 2, 1], dtype=torch.int32, device=DEV)
    bad = torch.tensor([1, n_speakers, 2, -1], dtype=torch.int32, device=DEV)
    for kind in OP_KINDS.values():
        t0, t1 = (p0, p1) if kind in (ops.NORM_MVN, ops.DENORM_MVN) else (p0, p0 + p1)
        want, got = ops.normalise_items(x, t0, t1, good, kind), ops.normalise_items(x, t0, t1, bad, kind)
        assert torch.isnan(got[1]).all() and torch.isnan(got[3]).all()
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
        assert torch.isnan(ops.normalise_items_backward(x, t0, t1, bad, kind)[3]).all()
    rows = ops.item_rows(p1, bad)
    assert torch.isnan(rows[1]).all() and torch.isnan(rows[3]).all() and torch.equal(rows[0], p1[1]) and torch.equal(rows[2], p1[2])
    # the loader's pass: NaN in the valid frames of that utterance, zeros in its pad frames, the others untouched
    lens = [5, 7, 3, 6]
    packed = torch.cat([x[i, :n] for i, n in enumerate(lens)]).contiguous()
    offsets = torch.tensor(np.concatenate(([0], np.cumsum(lens))), dtype=torch.int64, device=DEV)
    raw_w, norm_w = ops.pad_normalise_items(packed, offsets, 7, p0, p1, good, ops.NORM_MVN)
    raw_g, norm_g = ops.pad_normalise_items(packed, offsets, 7, p0, p1, bad, ops.NORM_MVN)
    assert torch.equal(raw_g, raw_w) and torch.equal(norm_g[0], norm_w[0]) and torch.equal(norm_g[2], norm_w[2])
    assert torch.isnan(norm_g[3, :6]).all() and (norm_g[3, 6:] == 0).all() and torch.isnan(norm_g[1]).all()
    # MLPG under that item's variances: its trajectory is NaN, the others' are not touched
    means = ops.normalise_items(x, p0, p1, good, ops.DENORM_MVN)
    seq_len = torch.tensor([7, 7, 5, 6], dtype=torch.int64, device=DEV)
    std = p1.clamp_min(0.1)                               # (the fixture's zero standard deviation is no variance to solve under)
    traj_w = ops.mlpg(means, ops.item_rows(std, good) ** 2, viz.synthesis.DEFAULT_WINDOWS, padding_size=3, seq_len=seq_len)
    traj_g = ops.mlpg(means, ops.item_rows(std, bad) ** 2, viz.synthesis.DEFAULT_WINDOWS, padding_size=3, seq_len=seq_len)
    assert torch.isnan(traj_g[1]).all() and torch.isnan(traj_g[3, :6]).all()
    assert torch.equal(traj_g[0], traj_w[0]) and torch.equal(traj_g[2], traj_w[2]) and not torch.isnan(traj_w).any()


@pytest.mark.parametrize('padding', [0, 100])
def test_mlpg_per_item_variances_equal_the_expanded_per_frame_form(padding):
    rng = np.random.RandomState(77)
    b, t, d = 6, 57, 5
    means = torch.from_numpy(rng.standard_normal((b, t, 3 * d)).astype(np.float32)).to(DEV)
    variances = torch.from_numpy(rng.uniform(0.05, 2.0, (b, 3 * d)).astype(np.float32)).to(DEV)
    seq_len = torch.tensor([57, 1, 30, 56, 2, 17], dtype=torch.int64, device=DEV)
    expanded = variances[:, None, :].expand(b, t, 3 * d).contiguous()
    for lengths in (seq_len, None):
        got = ops.mlpg(means, variances, viz.synthesis.DEFAULT_WINDOWS, padding_size=padding, seq_len=lengths)
        want = ops.mlpg(means, expanded, viz.synthesis.DEFAULT_WINDOWS, padding_size=padding, seq_len=lengths)
        assert torch.equal(got, want) and not torch.isnan(got).any()
    with pytest.raises(ValueError):
        ops.mlpg(means, variances[:4], viz.synthesis.DEFAULT_WINDOWS)
    # viz.synthesis.MLPG keeps the reference's meaning of 2-D variances: ONE sequence with per-frame variances
    one = viz.synthesis.MLPG(means[0], expanded[0], padding_size=padding)
    assert tuple(one.shape) == (t, d) and torch.equal(one, ops.mlpg(means[:1], expanded[:1], viz.synthesis.DEFAULT_WINDOWS, padding_size=padding)[0])


N_SPEAKERS = 5


def _speaker_batch(seed, b=8, frames=(60, 100), n_speakers=N_SPEAKERS):
    feats = synthetic.make_acoustic_batch(b, frames, streams=(('lf0', 3, 'mse'),), seed=seed, with_raw=True)
    feats['speaker_id'], _ = synthetic.speaker_batch_ids(b, n_speakers=n_speakers, seed=seed)
    return feats


def _speaker_model(cls=models.GRUF0Model, **kwargs):
    torch.manual_seed(3)
    model = cls(speaker_id_list='speakers.scp', **kwargs).to(DEV)
    own = model.state_dict()
    for key, value in synthetic.gru_f0_state().items():
        own[key].copy_(torch.from_numpy(value))
    synthetic.speaker_acoustic_normalisers(model, n_speakers=N_SPEAKERS, device=DEV)
    model.mode = 'train'
    return model


def test_gru_f0_model_with_per_speaker_parameters():
    """Loss, trajectory and LF0_RMSE_Hz of ``GRUF0Model(speaker_id_list=...)`` against a run in which the test denormalises the predicted
    deltas itself with per-frame expanded parameters and solves MLPG in the per-frame mode; fp32, 1e-4 relative (README 'Parity')."""
    model = _speaker_model(precision='fp32')
    feats = _speaker_batch(11)
    batch = data.to_device(feats, DEV, normalisers=model.normalisers)
    assert batch['speaker_index'].dtype == torch.int32 and batch['speaker_id'] == feats['speaker_id']
    loss, outputs = model(batch)
    got_metric = model.metrics.results_as_json_dict('train')['LF0_RMSE_Hz']

    plain = models.GRUF0Model(precision='fp32', generate=False).to(DEV)
    plain.load_state_dict(model.state_dict())
    plain.mode = 'train'
    want_loss, want_outputs = plain(batch)
    normaliser = model.normalisers['lf0']
    rows = torch.tensor(normaliser.speaker_rows(feats['speaker_id']), device=DEV)
    mean, std = normaliser.tables(DEV, deltas=True)
    t = want_outputs['normalised_lf0_deltas'].shape[1]
    mean_f, std_f = (p[rows][:, None, :].expand(-1, t, -1).contiguous() for p in (mean, std))
    deltas = want_outputs['normalised_lf0_deltas'].detach() * std_f + mean_f
    want_traj = viz.synthesis.MLPG(deltas, std_f ** 2, padding_size=100, seq_len=batch['n_frames'])
    metric = metrics.LF0Distortion()
    metric.accumulate(batch['lf0'], want_traj, batch['vuv'], batch['n_frames'])
    want_metric = metric.result_as_json()

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))

    print('loss %.8f / %.8f, trajectory rel %.3e, LF0_RMSE_Hz %.6f / %.6f' % (
        loss.item(), want_loss.item(), rel(outputs['lf0'], want_traj), got_metric, want_metric))
    assert abs(loss.item() - want_loss.item()) <= 1e-4 * abs(want_loss.item())
    assert rel(outputs['lf0'], want_traj) <= 1e-4
    assert want_metric > 0 and abs(got_metric - want_metric) <= 1e-4 * want_metric
    # speakers matter: the same prediction under speaker 0's parameters for everybody is another trajectory
    other = dict(batch)
    other['speaker_index'] = torch.zeros_like(batch['speaker_index'])
    assert rel(model.predict(other)['lf0'], want_traj) > 1e-3
    del other['speaker_index']
    with pytest.raises(KeyError, match='speaker_index'):
        model.predict(other)


class NamesInsideTheStep(models.GRUF0Model):
    """Hands the NAMES to the normaliser inside the step: what a model written against the reference does."""

    def _with_trajectories(self, outputs, n_frames, speaker_index=None):
        names = self._current_names
        index = None if speaker_index is None else self.normalisers['lf0'].speaker_index(names, speaker_index.device)
        return super()._with_trajectories(outputs, n_frames, index)

    def forward(self, features):
        self._current_names = features['speaker_id']
        return super().forward(features)


@pytest.mark.parametrize('names_inside', [False, True])
def test_graphed_steps_follow_the_speakers_of_every_batch(names_inside):
    """Six batches of ONE shape whose speakers differ: the replayed steps must read each batch's own ``speaker_index`` (a stale index
    would change the trajectories and the metric, not the loss, so the trajectories are compared too).  A model that resolves names
    inside the step cannot be captured: one warning, ordinary launches, the same numbers."""
    cls = NamesInsideTheStep if names_inside else models.GRUF0Model
    feats = [_speaker_batch(100 + i, b=8, frames=80) for i in range(6)]
    assert len({tuple(f['speaker_id']) for f in feats}) == len(feats)

    def run(graphed):
        model = _speaker_model(cls, precision='bf16')
        opt = optim.Adam(model.parameters(), lr=0.01, fused_loop=True)
        batches = [data.to_device(f, DEV, normalisers=model.normalisers) for f in feats]
        losses, trajectories = [], []
        cache = graphs.GraphedStepCache(model, opt) if graphed else None

        def one(batch):
            # (nothing of a step may stay referenced when the next one is captured: an autograd graph kept alive by its loss has its
            # gradient accumulation on the stream of the step that built it, which a capture must not touch)
            if graphed:
                loss, outputs = cache.step(batch)
            else:
                opt.zero_grad()
                loss, outputs = model(batch)
                F_hip.backward(loss)
                opt.step()
            return loss.detach().clone(), outputs['lf0'].detach().clone()

        for batch in batches:
            loss, trajectory = one(batch)
            losses.append(loss)
            trajectories.append(trajectory)
        if graphed:
            cache.flush()
        metric = model.metrics.results_as_json_dict('train')['LF0_RMSE_Hz']
        return torch.stack(losses).tolist(), trajectories, [p.detach().clone() for p in model.parameters()], metric, cache

    want = run(False)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        got = run(True)
    refused = [w for w in caught if 'cannot be captured' in str(w.message)]
    stats = got[4].stats()
    if names_inside:
        assert len(refused) == 1 and 'speaker_index' in str(refused[0].message), [str(w.message) for w in caught]
        assert stats['replayed'] == 0 and stats['eager'] == len(feats), stats
    else:
        assert not refused, [str(w.message) for w in refused]
        assert got[4].replayed_steps > 0 and stats['replayed'] >= 4, stats
    assert got[0] == want[0]
    for i, (a, b) in enumerate(zip(got[1], want[1])):
        assert torch.equal(a, b), 'trajectories of batch %d differ' % i
    for a, b in zip(got[2], want[2]):
        assert torch.equal(a, b)
    assert got[3] == want[3]
