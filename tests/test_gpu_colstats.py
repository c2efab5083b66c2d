"""K22 on the device: ops.column_stats / data.ColumnStats / data.fit_normalisers against tests/colstats_ref64.py.  Every expectation and
every bound comes from that helper (derived there from the algorithm, not from what the kernel returns)."""
import functools
import os

import numpy as np
import pytest
import torch

import colstats_ref64 as ref
from morgana_amd import data, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ONE_ROUNDING = 2.0 ** -23
GUARD = np.float32(7.5e33)
CONSTANTS = (np.float32(0.1), np.float32(2.0 ** 20 + 0.125), np.float32(-3e-30))
# A zero-length item, one frame, the edges of a wave, an item over several workgroups and merge levels.  The last length: an item
# is cut into one chunk per 16 steps and a step of a narrow feature is 1024 elements whatever D (1024 frames at D = 1, 340 at
# D = 3, 204 at D = 5), so 5000 frames of those are ONE workgroup; 40000 make 3 (D = 1), 8 (D = 3) and 13 (D = 5).  From D = 64 on
# 5000 frames are 20 workgroups and more.
LENGTHS = (0, 1, 63, 64, 65, 257)


def _long(width):
    return 40000 if width <= 5 else 5000


@functools.lru_cache(maxsize=None)
def _case(width, constant_only=False, adversarial=False):
    """(items, constant columns {column: value}) - items float32 (len, width); computed once and never written to."""
    rng = np.random.RandomState(100 + width)
    lengths = LENGTHS + (_long(width),)
    total = sum(lengths)
    centre, scale = rng.uniform(-5, 5, size=width), rng.uniform(0.5, 2.0, size=width)
    rows = (rng.randn(total, width) * scale + centre).astype(np.float32)
    constants = {}
    if constant_only:
        constants = {c: CONSTANTS[c % 3] for c in range(width)}
    elif width >= 3:
        constants = {0: CONSTANTS[0], width - 1: CONSTANTS[1]}
        if width >= 5:
            constants[2] = CONSTANTS[2]
            rows[:, 3] = rng.randint(0, 2, size=total)    # a binary label column
    for c, value in constants.items():
        rows[:, c] = value
    if adversarial:
        rows[:, 1] = ref.adversarial_column(total, seed=7)
    bounds = np.cumsum((0,) + lengths)
    items = tuple(rows[lo:hi] for lo, hi in zip(bounds[:-1], bounds[1:]))
    for x in items:
        x.setflags(write=False)
    return items, constants


@functools.lru_cache(maxsize=None)
def _want(width, constant_only=False, adversarial=False):
    return ref.two_pass(list(_case(width, constant_only, adversarial)[0]))


def _packed(items, lead=3, tail=5):
    """(whole allocation, packed view (N, D) starting `lead` floats in, offsets, longest item)"""
    width = items[0].shape[1]
    flat = np.concatenate([x.reshape(-1) for x in items])
    whole = np.full(lead + flat.size + tail, GUARD, dtype=np.float32)
    whole[lead:lead + flat.size] = flat
    dev = torch.from_numpy(whole).to(DEV)
    offsets = torch.from_numpy(np.cumsum([0] + [len(x) for x in items]).astype(np.int64)).to(DEV)
    return dev, dev[lead:lead + flat.size].view(-1, width), offsets, max(len(x) for x in items)


def _padded(items, lead=1, slack=3, fill_last=False):
    """(whole allocation, padded view (B, T, D), lengths, T): NaN past every item's length, T ``slack`` above the longest item.
    ``fill_last``: the (longest, last) item's rows up to T hold real values - for a seq_len above T, which the kernel clamps to T."""
    width = items[0].shape[1]
    t = max(len(x) for x in items) + slack
    body = np.full((len(items), t, width), np.nan, dtype=np.float32)
    for i, x in enumerate(items):
        body[i, :len(x)] = x
    lens = [len(x) for x in items]
    if fill_last:
        body[-1, lens[-1]:] = items[-1][:t - lens[-1]]
    whole = np.full(lead + body.size + 5, GUARD, dtype=np.float32)
    whole[lead:lead + body.size] = body.reshape(-1)
    dev = torch.from_numpy(whole).to(DEV)
    return dev, dev[lead:lead + body.size].view(len(items), t, width), lens, t


def _guards_untouched(whole, lead, used):
    host = whole.cpu().numpy()
    return np.all(host[:lead] == GUARD) and np.all(host[lead + used:] == GUARD)


def _check(got, want, all_items, constants=None, n_batches=1, caps=True, skip_columns=(), label=''):
    """count / min / max bit-equal; mean and var inside the derived bounds (and the bounds under the issue's caps); constant columns
    exact.  Prints each figure before it asserts."""
    np.testing.assert_array_equal(got['count'], want['count'])
    seen = want['count'] > 0
    keep = np.ones(want['count'].shape[1], dtype=bool)
    keep[list(skip_columns)] = False
    np.testing.assert_array_equal(got['mmin'][:, keep], want['mmin'][:, keep])
    np.testing.assert_array_equal(got['mmax'][:, keep], want['mmax'][:, keep])
    bound_mean, bound_var = ref.bounds(all_items, want['count'], n_batches)
    largest = np.nanmax(np.abs(np.concatenate([x for x in all_items if len(x)])), axis=0)
    constant = np.zeros_like(keep)
    constant[list(constants or ())] = True
    live = seen & keep & ~constant
    err_mean, err_var = np.abs(got['mean'] - want['mean']), np.abs(got['var'] - want['var'])
    with np.errstate(all='ignore'):
        ratios = (err_mean / bound_mean, err_var / bound_var, bound_var / want['var'], bound_mean / largest)
    print('%s: worst |mean err| / bound %.3g, |var err| / bound %.3g, bound_var / var %.3g, bound_mean / max|x| %.3g (2^-40 = %.3g)' % (
        (label,) + tuple(np.max(r[live], initial=0.0) for r in ratios) + (ref.CAP_MEAN,)))
    assert np.all(err_mean[live] <= bound_mean[live])
    assert np.all(err_var[live] <= bound_var[live])
    if caps:
        assert np.all(bound_mean[live] <= (ref.CAP_MEAN * np.broadcast_to(largest, live.shape))[live])
        assert np.all(bound_var[live] <= ref.CAP_VAR * want['var'][live])
    for c, value in (constants or {}).items():
        rows = seen[:, c]
        assert np.all(got['var'][rows, c] == 0.0) and np.all(got['mean'][rows, c] == float(value)), (c, got['mean'][:, c], got['var'][:, c])


SWEEP = [(1, False), (1, True), (3, False), (5, False), (64, False), (187, False), (609, False)]


@pytest.mark.parametrize('layout', ['packed', 'padded'])
@pytest.mark.parametrize('width, constant_only', SWEEP, ids=['1', '1const', '3', '5', '64', '187', '609'])
def test_sweep(width, constant_only, layout):
    items, constants = _case(width, constant_only)
    want = _want(width, constant_only)
    states = []
    for _ in range(2):
        stats = data.ColumnStats(width, device=DEV)
        if layout == 'packed':
            whole, view, offsets, longest = _packed(items)
            stats.update_packed(view, offsets, max_rows=longest)
            lead, used = 3, view.numel()
        else:
            whole, view, lens, t = _padded(items, fill_last=True)
            seq_len = torch.tensor(lens[:-1] + [t + 9], dtype=torch.int64, device=DEV)
            stats.update_padded(view, seq_len)
            lead, used = 1, view.numel()
        torch.cuda.synchronize()
        assert _guards_untouched(whole, lead, used)
        states.append(stats.state.clone())
    assert torch.equal(states[0].view(torch.int64), states[1].view(torch.int64)), 'two calls from the same state differ in their bits'
    if layout == 'padded':                                # the clamped last item really has T frames
        slack = t - lens[-1]
        items = items[:-1] + (np.concatenate([items[-1], items[-1][:slack]]),)
        want = ref.two_pass(list(items))
    _check(stats.result(), want, items, constants, label='D=%d %s' % (width, layout))


@pytest.mark.parametrize('width', [1, 3, 64])
@pytest.mark.parametrize('lead', [0, 1, 2, 3])
def test_every_alignment_of_the_first_element(width, lead):
    rng = np.random.RandomState(width * 4 + lead)
    items = [(rng.randn(n, width) + 2.0).astype(np.float32) for n in (2, 0, 1, 1500, 63, 7)]
    whole, view, offsets, longest = _packed(items, lead=lead)
    stats = data.ColumnStats(width, device=DEV).update_packed(view, offsets, max_rows=longest)
    torch.cuda.synchronize()
    assert _guards_untouched(whole, lead, view.numel())
    _check(stats.result(), ref.two_pass(items), items, label='D=%d lead=%d' % (width, lead))
    single = data.ColumnStats(width, device=DEV).update_packed(view, offsets)      # one chunk per item: the default without max_rows
    _check(single.result(), ref.two_pass(items), items, label='D=%d lead=%d, one chunk' % (width, lead))


def test_row_stride_above_the_width_takes_the_scalar_path():
    """ld > D: rows are not back to back.  ops.column_stats takes contiguous tensors only, so this goes through the C ABI."""
    from morgana_amd import _lib
    rng = np.random.RandomState(11)
    width, ld, lens = 5, 8, (3, 0, 700)
    wide = np.full((sum(lens), ld), np.nan, dtype=np.float32)
    wide[:, :width] = (rng.randn(sum(lens), width) * 2 - 1).astype(np.float32)
    dev = torch.from_numpy(wide).to(DEV)
    offsets = torch.from_numpy(np.cumsum((0,) + lens).astype(np.int64)).to(DEV)
    stats = data.ColumnStats(width, device=DEV)
    lib = _lib.load()
    need = lib.mg_column_stats_workspace_bytes(len(lens), max(lens), width)
    buf = torch.empty(need, dtype=torch.uint8, device=DEV)
    _lib.check(lib.mg_column_stats_f32(dev.data_ptr(), ld, width, len(lens), 0, offsets.data_ptr(), None, None, 1, stats.state.data_ptr(),
                                       buf.data_ptr(), need, None), 'mg_column_stats_f32')
    torch.cuda.synchronize()
    bounds = np.cumsum((0,) + lens)
    items = [wide[lo:hi, :width].copy() for lo, hi in zip(bounds[:-1], bounds[1:])]
    _check(stats.result(), ref.two_pass(items), items, label='ld=8 D=5')


def test_adversarial_column():
    items, constants = _case(5, adversarial=True)
    want = _want(5, adversarial=True)
    column = np.concatenate([x[:, 1] for x in items])
    mean, var = ref.exact(column[:2113])                   # the reference once more against exact arithmetic, on this very column
    assert abs(ref.two_pass([column[:2113].reshape(-1, 1)])['var'][0, 0] - float(var)) <= 1e-13 * float(var)
    for layout in ('packed', 'padded'):
        stats = data.ColumnStats(5, device=DEV)
        if layout == 'packed':
            whole, view, offsets, longest = _packed(items)
            stats.update_packed(view, offsets, max_rows=longest)
        else:
            whole, view, lens, t = _padded(items)
            stats.update_padded(view, torch.tensor(lens, dtype=torch.int64, device=DEV))
        got = stats.result()
        print('2^20 + k/8 column, %s: var %.17g (float64 %.17g), relative %.3g' % (
            layout, got['var'][0, 1], want['var'][0, 1], abs(got['var'][0, 1] - want['var'][0, 1]) / want['var'][0, 1]))
        assert abs(got['var'][0, 1] - want['var'][0, 1]) <= ref.CAP_VAR * want['var'][0, 1]
        _check(got, want, items, constants, label='adversarial ' + layout)


def test_accumulation_over_batches_and_layouts():
    items, constants = _case(5)
    want = _want(5)
    results = {}
    for name, splits in (('one batch', [items]), ('three batches', [items[:3], items[3:5], items[5:]]),
                         ('one item per batch', [items[i:i + 1] for i in range(len(items))])):
        for layout in ('packed', 'padded'):
            stats = data.ColumnStats(5, device=DEV)
            for part in splits:
                if layout == 'packed':
                    _, view, offsets, longest = _packed(part)
                    stats.update_packed(view, offsets, max_rows=longest)
                else:
                    _, view, lens, _ = _padded(part, slack=0)
                    stats.update_padded(view, torch.tensor(lens, dtype=torch.int64, device=DEV))
            results[name, layout] = stats.result()
            _check(results[name, layout], want, items, constants, n_batches=len(splits), caps=False, label='%s, %s' % (name, layout))
    bound_mean, bound_var = ref.bounds(items, want['count'], n_batches=len(items))
    for name in ('one batch', 'three batches', 'one item per batch'):
        a, b = results[name, 'packed'], results[name, 'padded']
        assert np.all(np.abs(a['mean'] - b['mean']) <= 2 * bound_mean) and np.all(np.abs(a['var'] - b['var']) <= 2 * bound_var)


def test_groups_and_out_of_range_rows():
    rng = np.random.RandomState(21)
    lens = (40, 0, 300, 1, 65, 2000, 64, 129)
    rows = [0, 2, 2, 0, 7, 0, -1, 2]                      # speaker 1 is absent; items 4 and 6 name no speaker
    shift = {0: 0.0, 2: 4.0, 7: -6.0, -1: 8.0}
    items = [(rng.randn(n, 5) * 1.5 + shift[r]).astype(np.float32) for n, r in zip(lens, rows)]
    want = ref.two_pass(items, rows, groups=3)
    assert want['count'][1, 0] == 0 and want['count'][0, 0] == 2041 and want['count'][2, 0] == 429
    item_row = torch.tensor(rows, dtype=torch.int32, device=DEV)
    for layout in ('packed', 'padded'):
        stats = data.ColumnStats(5, groups=3, device=DEV)
        if layout == 'packed':
            _, view, offsets, longest = _packed(items)
            stats.update_packed(view, offsets, item_row, max_rows=longest)
        else:
            _, view, seq, _ = _padded(items, slack=0)
            stats.update_padded(view, torch.tensor(seq, dtype=torch.int64, device=DEV), item_row)
        got = stats.result()
        assert np.all(got['count'][1] == 0) and np.isnan(got['mean'][1]).all()
        _check(got, want, items, label='groups, ' + layout)
    # the same without the two items that name no speaker: nothing else moves beyond the bounds
    kept = [i for i, r in enumerate(rows) if 0 <= r < 3]
    _, view, offsets, longest = _packed([items[i] for i in kept])
    alone = data.ColumnStats(5, groups=3, device=DEV).update_packed(
        view, offsets, torch.tensor([rows[i] for i in kept], dtype=torch.int32, device=DEV), max_rows=longest).result()
    _check(alone, want, items, label='groups without the out-of-range items')
    with pytest.raises(ValueError, match='item_row'):
        ops.column_stats(stats.state, view, offsets=offsets)


def test_a_nan_poisons_its_column_only():
    items, constants = _case(5)
    items = [x.copy() for x in items]
    items[5][100, 1] = np.nan
    want = ref.two_pass(items)
    for layout in ('packed', 'padded'):
        stats = data.ColumnStats(5, device=DEV)
        if layout == 'packed':
            _, view, offsets, longest = _packed(items)
            stats.update_packed(view, offsets, max_rows=longest)
        else:
            _, view, lens, _ = _padded(items, slack=0)
            stats.update_padded(view, torch.tensor(lens, dtype=torch.int64, device=DEV))
        got = stats.result()
        assert np.isnan(got['mean'][0, 1]) and np.isnan(got['var'][0, 1])
        _check(got, want, items, constants, skip_columns=(1,), label='NaN, ' + layout)
        clean = [x for i, x in enumerate(items) if i != 5] + [np.delete(items[5], 100, axis=0)]
        assert got['mmin'][0, 1] == np.concatenate(clean)[:, 1].min()       # min / max skip the NaN


# ---------------------------------------------------------------------------------------------------------------- end to end
SPEAKERS = ('anna', 'bert')


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    """9 utterances of 40-120 frames, two speakers: lf0 (+ deltas), phone-level lab with constant and binary columns, integer dur."""
    root = tmp_path_factory.mktemp('corpus')
    rng = np.random.RandomState(42)
    names = ['utt%02d' % i for i in range(9)]
    utterances = []
    for i, name in enumerate(names):
        frames, speaker = int(rng.randint(40, 121)), SPEAKERS[i % 2]
        phones = frames // 5
        lab = np.zeros((phones, 12), dtype=np.float32)
        lab[:, 1] = 1.0                                    # columns 0 and 1 constant
        lab[:, 2:8] = rng.randint(0, 2, size=(phones, 6))
        lab[:, 8:] = rng.uniform(0.0, 1.0, size=(phones, 4)).astype(np.float32)
        feats = {'lf0': (rng.randn(frames, 1) * 0.3 + (5.0 if speaker == 'anna' else 4.4)).astype(np.float32),
                 'lf0_deltas': (rng.randn(frames, 3) * 0.1).astype(np.float32),
                 'lab': lab, 'dur': rng.randint(1, 11, size=(phones, 1)).astype(np.int64)}
        for key, value in feats.items():
            os.makedirs(root / 'train' / key, exist_ok=True)
            np.save(root / 'train' / key / (name + '.npy'), value)
        os.makedirs(root / 'train' / 'speaker_id', exist_ok=True)
        (root / 'train' / 'speaker_id' / (name + '.txt')).write_text(speaker + '\n')
        utterances.append(dict(feats, name=name, speaker_id=speaker))
    (root / 'train_ids.scp').write_text('\n'.join(names) + '\n')
    (root / 'speakers.txt').write_text('\n'.join(SPEAKERS) + '\n')
    (root / 'speakers_plus_one.txt').write_text('\n'.join(SPEAKERS + ('carl',)) + '\n')
    return root, utterances


def _sources():
    return {'lf0': data.NumpyBinarySource('lf0', use_deltas=True), 'lab': data.NumpyBinarySource('lab'),
            'dur': data.NumpyBinarySource('dur'), 'speaker_id': data.StringSource('speaker_id')}


def _normalisers(root, by_speaker, speaker_list='speakers.txt'):
    if by_speaker:
        path = str(root / speaker_list)
        return {'lf0': data.SpeakerDependentMeanVarianceNormaliser('lf0', path, use_deltas=True),
                'lab': data.SpeakerDependentMinMaxNormaliser('lab', path), 'dur': data.MeanVarianceNormaliser('dur')}
    return {'lf0': data.MeanVarianceNormaliser('lf0', use_deltas=True), 'lab': data.MinMaxNormaliser('lab'),
            'dur': data.MeanVarianceNormaliser('dur')}


def _reference_params(utterances, key, kind, speaker=None):
    rows = [np.asarray(u[key], dtype=np.float32) for u in utterances if speaker is None or u['speaker_id'] == speaker]
    want = ref.two_pass(rows)
    if kind == 'mvn':
        return {'mean': want['mean'][0], 'std_dev': np.sqrt(want['var'][0])}
    return {'mmin': want['mmin'][0], 'mmax': want['mmax'][0]}


def _within_one_rounding(got, want64):
    want32 = want64.astype(np.float32)
    assert got.dtype == np.float32
    assert np.all(np.abs(got.astype(np.float64) - want32.astype(np.float64)) <= ONE_ROUNDING * np.abs(want64)), (got, want32)


@pytest.mark.parametrize('by_speaker', [False, True], ids=['shared', 'per_speaker'])
def test_fit_normalisers_end_to_end(corpus, by_speaker):
    root, utterances = corpus
    out_dir = 'norm_per_speaker' if by_speaker else 'norm_shared'
    normalisers = _normalisers(root, by_speaker)
    dataset = data.FilesDataset(_sources(), 'train', 'train_ids.scp', normalisers, data_root=str(root))
    results = data.fit_normalisers(dataset, normalisers, device=DEV, batch_size=4, out_dir=out_dir, data_root=str(root))
    assert sorted(results) == ['dur', 'lab', 'lf0', 'lf0_deltas']
    assert results['lf0']['count'].sum() == sum(len(u['lf0']) for u in utterances)
    written = sorted(os.path.relpath(os.path.join(d, f), root / out_dir) for d, _, fs in os.walk(root / out_dir) for f in fs)
    if by_speaker:
        assert written == sorted(['dur_mvn.json'] + [os.path.join(s, f) for s in SPEAKERS
                                                     for f in ('lf0_mvn.json', 'lf0_deltas_mvn.json', 'lab_minmax.json')])
    else:
        assert written == ['dur_mvn.json', 'lab_minmax.json', 'lf0_deltas_mvn.json', 'lf0_mvn.json']

    fresh = data.Normalisers(_normalisers(root, by_speaker), out_dir, data_root=str(root))
    expected = _normalisers(root, by_speaker)
    kinds = {'lf0': 'mvn', 'lab': 'minmax', 'dur': 'mvn'}
    for name, kind in kinds.items():
        if by_speaker and name != 'dur':
            own = {s: _reference_params(utterances, name, kind, s) for s in SPEAKERS}
            deltas = {s: _reference_params(utterances, 'lf0_deltas', kind, s) for s in SPEAKERS} if name == 'lf0' else None
            for s in SPEAKERS:
                for p, value in own[s].items():
                    _within_one_rounding(fresh[name].params[s][p], value)
                    np.testing.assert_array_equal(fresh[name].params[s][p], normalisers[name].params[s][p])
                if deltas:
                    for p, value in deltas[s].items():
                        _within_one_rounding(fresh[name].delta_params[s][p], value)
        else:
            own = _reference_params(utterances, name, kind)
            deltas = _reference_params(utterances, 'lf0_deltas', kind) if name == 'lf0' else None
            for p, value in own.items():
                _within_one_rounding(fresh[name].params[p], value)
                np.testing.assert_array_equal(fresh[name].params[p], normalisers[name].params[p])
            if deltas:
                for p, value in deltas.items():
                    _within_one_rounding(fresh[name].delta_params[p], value)
        expected[name].set_params(own, deltas)

    raw = [dataset.raw(i) for i in range(len(dataset))]
    got = data.collate_to_device(raw, fresh, DEV)
    want = data.collate_to_device(raw, expected, DEV)
    lens = {'lf0': [len(u['lf0']) for u in raw], 'lab': [len(u['lab']) for u in raw], 'dur': [len(u['dur']) for u in raw]}
    for name in ('normalised_lf0', 'normalised_lab', 'normalised_dur'):
        np.testing.assert_allclose(got[name].cpu().numpy(), want[name].cpu().numpy(), rtol=1e-4, atol=1e-6)
    groups = [[i for i, u in enumerate(raw) if u['speaker_id'] == s] for s in SPEAKERS] if by_speaker else [list(range(len(raw)))]

    def valid(name, feature, members):
        out = got[name].cpu().numpy().astype(np.float64)
        return np.concatenate([out[i, :lens[feature][i]] for i in members])

    for members in groups:
        rows = valid('normalised_lf0', 'lf0', members)
        print('normalised_lf0: |mean| %.3g, |std - 1| %.3g' % (np.abs(rows.mean(axis=0)).max(), np.abs(rows.std(axis=0) - 1).max()))
        assert np.all(np.abs(rows.mean(axis=0)) <= 1e-4) and np.all(np.abs(rows.std(axis=0) - 1.0) <= 1e-4)
        rows = valid('normalised_lab', 'lab', members)
        source = np.concatenate([raw[i]['lab'] for i in members])
        moving = source.min(axis=0) != source.max(axis=0)
        assert moving.sum() == 10
        assert np.all(rows.min(axis=0)[moving] == 0.0) and np.all(rows.max(axis=0)[moving] == 1.0)
        assert np.all(rows[:, ~moving] == 0.0)
    rows = valid('normalised_dur', 'dur', list(range(len(raw))))
    assert np.all(np.abs(rows.mean(axis=0)) <= 1e-4) and np.all(np.abs(rows.std(axis=0) - 1.0) <= 1e-4)


def test_fit_normalisers_refuses_an_absent_speaker_and_a_nan(corpus):
    root, utterances = corpus
    normalisers = _normalisers(root, True, speaker_list='speakers_plus_one.txt')
    dataset = data.FilesDataset(_sources(), 'train', 'train_ids.scp', normalisers, data_root=str(root))
    with pytest.raises(ValueError, match='carl'):
        data.fit_normalisers(dataset, normalisers, device=DEV, out_dir='norm_absent', data_root=str(root))
    assert not os.path.exists(root / 'norm_absent')
    assert normalisers['lf0'].params == {} and normalisers['dur'].params is None
    poisoned = [dict(u) for u in utterances]
    poisoned[3]['lf0_deltas'] = poisoned[3]['lf0_deltas'].copy()
    poisoned[3]['lf0_deltas'][7, 2] = np.nan
    shared = _normalisers(root, False)
    with pytest.raises(ValueError, match=r"'lf0_deltas' is not finite in columns \[2\]"):
        data.fit_normalisers(poisoned, shared, device=DEV, out_dir='norm_nan', data_root=str(root))
    assert not os.path.exists(root / 'norm_nan') and shared['lf0'].params is None
