"""K30 on the device: mg_frame_counters_f32 / ops.frame_counters / data.frame_counters and the loaders that use them, bit for bit
against tests/counters_ref.py (python integers and Fractions rounded to float32 from the exact rational) over whole padded outputs."""
import functools
import os

import numpy as np
import pytest
import torch

import counters_ref as ref
from morgana_amd import _lib, data, models, ops, optim

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = np.float32(7.5e33)
KINDS = ('full', 'phone')
N_PHONES = 7


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(n_states):
    """(dur (4, 7, S) int64, T, seq_len, n_phones).  Random durations with empty states and phones (counters_ref.random_durations; up to 40
    frames for S = 1, up to 12 per state for S = 5 so that T stays below 700), and
      item 0: one segment of 300 frames - longer than a wave and than a 256-thread chunk; total > T: cut,
      item 1: all zero, between two others,
      item 2: a negative duration; total < T; seq_len > total: zeros in between,
      item 3: seq_len < total; n_phones drops two trailing phones that hold non-zero durations."""
    rng = np.random.RandomState(40 + n_states)
    high = 40 if n_states == 1 else 12
    dur = np.stack([ref.random_durations(rng, N_PHONES, n_states, high) for _ in range(4)])
    dur[0, 4, n_states - 1] = 300
    dur[1] = 0
    dur[2, 5, 0] = -4
    dur[3, 5:] = 0
    dur[3, 5:, n_states - 1] = (9, 6)
    n_phones = np.array([N_PHONES, N_PHONES, N_PHONES, 5], dtype=np.int64)
    totals = [ref.total(dur[b], n_phones[b]) for b in range(4)]
    t = totals[0] - 23
    t -= 1 if t % 64 == 0 else 0
    seq_len = np.array([10 ** 6, 50, totals[2] + 9, totals[3] - 11], dtype=np.int64)
    assert 300 < t <= 700 and t % 64 and totals[1] == 0 and 0 < totals[2] < totals[2] + 9 < t and 11 < totals[3] < t
    assert ref.total(dur[3]) == totals[3] + 15 and (dur[2] < 0).sum() == 1
    for a in (dur, seq_len, n_phones):
        a.setflags(write=False)
    return dur, t, seq_len, n_phones


@functools.lru_cache(maxsize=None)
def _want(n_states, kind):
    """The reference's padded output of ``_case``: made once, never written to."""
    dur, t, seq_len, n_phones = _case(n_states)
    want = ref.padded(dur, kind, t, seq_len, n_phones)
    want.setflags(write=False)
    return want


def _valid(n_states):
    dur, t, seq_len, n_phones = _case(n_states)
    return [min(t, ref.total(dur[b], n_phones[b]), int(seq_len[b])) for b in range(4)]


def _device(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _guarded_nan(n, lead):
    """A device allocation of GUARD with ``n`` NaN floats starting ``lead`` floats in: (whole allocation, address of the NaN part)."""
    whole = np.full(lead + n + 5, GUARD, dtype=np.float32)
    whole[lead:lead + n] = np.nan
    dev = torch.from_numpy(whole).to(DEV)
    return dev, dev.data_ptr() + 4 * lead


def _inside(whole, lead, used):
    host = whole.cpu().numpy()
    assert np.all(host[:lead] == GUARD) and np.all(host[lead + used:] == GUARD), 'the kernel wrote outside an output'
    return host[lead:lead + used]


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('blocks', [0, 1, 3], ids=['default', 'one_block', 'three_blocks'])
@pytest.mark.parametrize('n_states', [1, 5])
@pytest.mark.parametrize('kind', KINDS)
def test_kernel_equals_the_reference_bit_for_bit(kind, n_states, blocks):
    """mg_frame_counters_f32 through the C ABI into NaN-filled, guarded outputs that start 3 floats into their allocations: every element
    of the padded raw output is the reference's, zeros included, whatever the number of workgroups per item; the normalised output
    alone and beside the raw one is the device normaliser on it."""
    lib = _lib.load()
    dur_np, t, seq_len_np, n_phones_np = _case(n_states)
    want = _want(n_states, kind)
    cols = ref.COLUMNS[kind]
    dur, seq_len, n_phones = _device(dur_np), _device(seq_len_np), _device(n_phones_np)
    rng = np.random.RandomState(9)
    p0, p1 = _device(rng.rand(cols).astype(np.float32)), _device((rng.rand(cols) * 30 + 1.5).astype(np.float32))
    n, lead = want.size, 3
    masked = torch.arange(t, device=DEV)[None, :, None] < _device(np.array(_valid(n_states)))[:, None, None]
    for outputs in (('raw',), ('raw', 'norm'), ('norm',)):
        held = {name: _guarded_nan(n, lead) for name in outputs}
        with_norm = 'norm' in outputs
        _lib.check(lib.mg_frame_counters_f32(dur.data_ptr(), 4, N_PHONES, n_states, dur.stride(0), dur.stride(1), dur.stride(2),
                                             n_phones.data_ptr(), seq_len.data_ptr(), t, ops.COUNTERS_KINDS[kind][0],
                                             p0.data_ptr() if with_norm else None, p1.data_ptr() if with_norm else None, None, 0,
                                             ops.NORM_MINMAX if with_norm else -1, held['raw'][1] if 'raw' in held else None,
                                             held['norm'][1] if with_norm else None, blocks, None), 'mg_frame_counters_f32')
        torch.cuda.synchronize()
        if 'raw' in held:
            got = _inside(held['raw'][0], lead, n).reshape(want.shape)
            np.testing.assert_array_equal(_bits(got), _bits(want))
        if with_norm:
            got = _inside(held['norm'][0], lead, n).reshape(want.shape)
            twin = ops.normalise(_device(want), p0, p1, ops.NORM_MINMAX)
            np.testing.assert_array_equal(_bits(got), _bits(torch.where(masked, twin, torch.zeros_like(twin))))
    np.testing.assert_array_equal(dur.cpu().numpy(), dur_np)


@pytest.mark.parametrize('kind', KINDS)
def test_ops_without_lengths_and_with_either(kind):
    """seq_len and n_phones are optional, each on its own; t = 0 and B = 0 give empty outputs."""
    dur_np, t, seq_len_np, n_phones_np = _case(5)
    dur = _device(dur_np)
    for seq_len, n_phones in ((None, None), (seq_len_np, None), (None, n_phones_np)):
        raw, norm = ops.frame_counters(dur, t=t, kind=kind, seq_len=None if seq_len is None else _device(seq_len),
                                       n_phones=None if n_phones is None else _device(n_phones))
        assert norm is None
        np.testing.assert_array_equal(_bits(raw), _bits(ref.padded(dur_np, kind, t, seq_len, n_phones)))
    assert ops.frame_counters(dur, t=0, kind=kind)[0].shape == (4, 0, ref.COLUMNS[kind])
    assert ops.frame_counters(dur[:0], t=5, kind=kind)[0].shape == (0, 5, ref.COLUMNS[kind])
    with pytest.raises(ValueError, match='segments'):
        ops.frame_counters(torch.zeros((1, ops.MAX_PHONES // 5 + 1, 5), dtype=torch.int64, device=DEV), t=4)
    with pytest.raises(ValueError):
        ops.frame_counters(dur, t=t, kind='minimal')
    with pytest.raises(ValueError):
        ops.frame_counters(dur, t=t, want_raw=False)
    with pytest.raises(TypeError):
        ops.frame_counters(dur.int(), t=t)
    with pytest.raises(ValueError):
        ops.frame_counters(dur, t=t, seq_len=_device(seq_len_np[:3]))


@pytest.mark.parametrize('kind', KINDS)
def test_strided_durations_are_read_in_place(kind):
    dur5, t, seq_len_np, n_phones_np = _case(5)
    dur1 = _case(1)[0]
    seq_len, n_phones = _device(seq_len_np), _device(n_phones_np)

    def run(d, **kw):
        return ops.frame_counters(d, t=t, kind=kind, seq_len=seq_len, n_phones=n_phones, **kw)[0]

    # (B, P, 1)[..., 0]: the loader's phone durations as a (B, P) view
    loader = _device(dur1)
    view = loader[..., 0]
    assert view.dim() == 2 and view.data_ptr() == loader.data_ptr()
    assert torch.equal(run(view), run(loader)) and torch.equal(run(view), run(view.contiguous()))
    # a (B, S, P) tensor transposed: states along the slow axis
    swapped = _device(np.ascontiguousarray(dur5.transpose(0, 2, 1))).transpose(1, 2)
    assert not swapped.is_contiguous() and swapped.stride() == (5 * N_PHONES, 1, N_PHONES)
    want = run(_device(dur5))
    assert torch.equal(run(swapped), want)
    np.testing.assert_array_equal(_bits(want), _bits(ref.padded(dur5, kind, t, seq_len_np, n_phones_np)))
    # a slice with a storage offset inside a larger tensor of other values
    big = np.full((6, N_PHONES + 4, 8), 77, dtype=np.int64)
    big[1:5, 3:3 + N_PHONES, 2:7] = dur5
    part = _device(big)[1:5, 3:3 + N_PHONES, 2:7]
    assert part.storage_offset() > 0 and not part.is_contiguous()
    assert torch.equal(run(part), want)
    # an expanded (stride 0) batch: every item the same durations
    same = _device(dur5[3])[None].expand(4, -1, -1)
    assert same.stride(0) == 0
    got = run(same, blocks_per_item=2)
    for b in range(4):
        np.testing.assert_array_equal(_bits(got[b]), _bits(ref.padded(dur5[3:4], kind, t, seq_len_np[b:b + 1], n_phones_np[b:b + 1])[0]))


@pytest.mark.parametrize('n_states', [1, 5])
def test_normalised_twin(n_states):
    """Plain min-max, plain mean-variance and per-item tables: bit-equal to the existing device normalisers applied to the raw output,
    zeros on the pad frames; a row index outside the table gives NaN in that item's valid frames; a constant column under min-max is 0."""
    dur_np, t, seq_len_np, n_phones_np = _case(n_states)
    dur, seq_len, n_phones = _device(dur_np), _device(seq_len_np), _device(n_phones_np)
    valid = _valid(n_states)
    masked = torch.arange(t, device=DEV)[None, :, None] < _device(np.array(valid))[:, None, None]
    rng = np.random.RandomState(12)
    for kind in KINDS:
        cols = ref.COLUMNS[kind]
        want_raw = _device(_want(n_states, kind))
        for norm_kind in (ops.NORM_MINMAX, ops.NORM_MVN):
            p0, p1 = _device((rng.rand(cols) * 2).astype(np.float32)), _device((rng.rand(cols) * 40 + 2.5).astype(np.float32))
            raw, norm = ops.frame_counters(dur, t=t, kind=kind, seq_len=seq_len, n_phones=n_phones, p0=p0, p1=p1, norm_kind=norm_kind)
            assert torch.equal(raw, want_raw)
            twin = ops.normalise(raw, p0, p1, norm_kind)
            assert torch.equal(norm, torch.where(masked, twin, torch.zeros_like(twin)))
            alone = ops.frame_counters(dur, t=t, kind=kind, seq_len=seq_len, n_phones=n_phones, p0=p0, p1=p1, norm_kind=norm_kind, want_raw=False)
            assert alone[0] is None and torch.equal(alone[1], norm)
            # tables of three rows; item 2 names a row outside them, item 0 a negative one in the second round
            t0, t1 = _device((rng.rand(3, cols) * 2).astype(np.float32)), _device((rng.rand(3, cols) * 40 + 2.5).astype(np.float32))
            for rows in ([2, 0, 3, 1], [-1, 1, 0, 2]):
                item_row = torch.tensor(rows, dtype=torch.int32, device=DEV)
                raw, norm = ops.frame_counters(dur, t=t, kind=kind, seq_len=seq_len, n_phones=n_phones, p0=t0, p1=t1, norm_kind=norm_kind,
                                               item_row=item_row)
                assert torch.equal(raw, want_raw)
                twin = ops.normalise_items(raw, t0, t1, item_row, norm_kind)
                assert torch.equal(norm.isnan(), twin.isnan() & masked)
                assert torch.equal(torch.nan_to_num(norm, nan=-7.0), torch.nan_to_num(torch.where(masked, twin, torch.zeros_like(twin)), nan=-7.0))
                bad = [b for b, r in enumerate(rows) if not 0 <= r < 3][0]
                assert valid[bad] > 0 and bool(norm[bad, :valid[bad]].isnan().all()) and bool((norm[bad, valid[bad]:] == 0).all())
    # a constant column (the state index of a phone-level alignment is 1 on every frame) with mmin == mmax: 0, not a division by zero
    if n_states == 1:
        mmin, mmax = torch.zeros(9, device=DEV), torch.full((9,), 50.0, device=DEV)
        mmin[3] = mmax[3] = 1.0
        raw, norm = ops.frame_counters(dur, t=t, seq_len=seq_len, n_phones=n_phones, p0=mmin, p1=mmax, norm_kind=ops.NORM_MINMAX)
        assert bool((raw[:, :, 3][masked[:, :, 0]] == 1.0).all()) and bool((norm[:, :, 3] == 0.0).all()) and bool((norm[:, :, 2][masked[:, :, 0]] > 0).all())


def test_data_frame_counters_on_tensors():
    dur_np = _case(5)[0]
    dur = _device(dur_np)
    totals = [ref.total(d) for d in dur_np]
    for kind in KINDS:
        got = data.frame_counters(dur, kind)                                       # T: the largest sum of durations
        assert got.shape == (4, max(totals), ref.COLUMNS[kind]) and got.dtype == torch.float32
        np.testing.assert_array_equal(_bits(got), _bits(ref.padded(dur_np, kind, max(totals))))
        for max_len in (max(totals) + 5, 100):                                     # longer: zero padded; shorter: cut
            got = data.frame_counters(dur, kind, max_len=max_len)
            np.testing.assert_array_equal(_bits(got), _bits(ref.padded(dur_np, kind, max_len)))
    seq_len, n_phones = torch.tensor([[5], [9], [700], [33]]), torch.tensor([7, 7, 2, 7], dtype=torch.int32)          # any integer type, host or device
    got = data.frame_counters(dur, seq_len=seq_len, n_phones=n_phones, max_len=120)
    np.testing.assert_array_equal(_bits(got), _bits(ref.padded(dur_np, 'full', 120, [5, 9, 700, 33], [7, 7, 2, 7])))
    # (B, P) and int32 durations; the host form of one item gives the same bits
    flat = _device(_case(1)[0][..., 0].astype(np.int32))
    got = data.frame_counters(flat)
    for b in (0, 2, 3):
        host = data.frame_counters(np.clip(_case(1)[0][b], 0, None))
        np.testing.assert_array_equal(_bits(got[b, :len(host)]), _bits(host))
        assert bool((got[b, len(host):] == 0).all())
    with pytest.raises(_lib.MorganaHipError):
        data.frame_counters(torch.from_numpy(np.array(dur_np)))
    with pytest.raises(TypeError):
        data.frame_counters(dur.float())


def test_capture_and_replay_of_the_bare_launch():
    """One capture of ops.frame_counters, replayed, then replayed again on durations changed in place."""
    first, t, seq_len_np, n_phones_np = _case(5)
    second = np.array(first[::-1])
    dur, seq_len, n_phones = _device(first), _device(seq_len_np), _device(n_phones_np)
    p0, p1 = torch.zeros(9, device=DEV), torch.full((9,), 37.0, device=DEV)
    args = dict(t=t, seq_len=seq_len, n_phones=n_phones, p0=p0, p1=p1, norm_kind=ops.NORM_MINMAX)
    eager_first = ops.frame_counters(dur, **args)
    eager_second = ops.frame_counters(_device(second), **args)
    assert not torch.equal(eager_first[0], eager_second[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.frame_counters(dur, **args)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, eager_first):
        assert torch.equal(got, want)
    dur.copy_(_device(second))
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, eager_second):
        assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- loader and fit
SPEAKERS = ('anna', 'bert')
LAB_DIM = 12
STATES = 5


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    """6 utterances of 30 to 200 frames, two speakers, in two data directories that differ in one folder: ``train/counters`` holds the
    host form's counters of ``dur``, ``train5/counters`` those of ``state_dur`` (5 states).  lab, dur, state_dur, n_frames, lf0_deltas and
    speaker_id are the same in both."""
    root = tmp_path_factory.mktemp('counters_corpus')
    rng = np.random.RandomState(61)
    names = ['utt%02d' % i for i in range(6)]
    frames = []
    for i, name in enumerate(names):
        n_phones = int(rng.randint(4, 8))
        while True:
            state_dur = ref.random_durations(rng, n_phones, STATES, high=9 if i else 12)
            total = int(state_dur.sum())
            if 30 <= total <= 200:
                break
        frames.append(total)
        dur = state_dur.sum(axis=1, keepdims=True)
        lab = rng.randn(n_phones, LAB_DIM).astype(np.float32)
        targets = rng.randn(total, 3).astype(np.float32)
        for split, counters in (('train', data.frame_counters(dur)), ('train5', data.frame_counters(state_dur))):
            for folder, value in (('lab', lab), ('dur', dur), ('state_dur', state_dur), ('lf0_deltas', targets), ('counters', counters)):
                os.makedirs(root / split / folder, exist_ok=True)
                np.save(root / split / folder / (name + '.npy'), value)
            for folder, text in (('n_frames', str(total)), ('speaker_id', SPEAKERS[i % 2])):
                os.makedirs(root / split / folder, exist_ok=True)
                (root / split / folder / (name + '.txt')).write_text(text + '\n')
    assert min(frames) >= 30 and max(frames) <= 200 and len(set(frames)) > 3
    (root / 'ids.scp').write_text('\n'.join(names) + '\n')
    (root / 'speakers.txt').write_text('\n'.join(SPEAKERS) + '\n')
    return root, names


def _sources(computed, dur_name):
    sources = {'lab': data.NumpyBinarySource('lab'), 'dur': data.NumpyBinarySource('dur'), 'state_dur': data.NumpyBinarySource('state_dur'),
               'lf0_deltas': data.NumpyBinarySource('lf0_deltas'), 'n_frames': data.TextSource('n_frames'),
               'speaker_id': data.StringSource('speaker_id')}
    sources['counters'] = data.FrameCountersSource('counters', dur_name=dur_name) if computed else data.NumpyBinarySource('counters')
    return sources


def _normalisers(root, by_speaker, fitted=True):
    rng = np.random.RandomState(5)
    out = {'lab': data.MeanVarianceNormaliser('lab'), 'lf0_deltas': data.MeanVarianceNormaliser('lf0_deltas')}
    out['lab'].set_params({'mean': rng.randn(LAB_DIM).astype(np.float32), 'std_dev': (rng.rand(LAB_DIM) + 0.5).astype(np.float32)})
    out['lf0_deltas'].set_params({'mean': rng.randn(3).astype(np.float32), 'std_dev': (rng.rand(3) + 0.5).astype(np.float32)})
    group = lambda: {'mmin': (rng.rand(9) * 0.5).astype(np.float32), 'mmax': (rng.rand(9) * 30 + 2).astype(np.float32)}
    if by_speaker:
        out['counters'] = data.SpeakerDependentMinMaxNormaliser('counters', str(root / 'speakers.txt'))
        if fitted:
            out['counters'].set_params({s: group() for s in SPEAKERS})
    else:
        out['counters'] = data.MinMaxNormaliser('counters')
        if fitted:
            out['counters'].set_params(group())
    return out


def _same_batch(have, batch):
    assert sorted(have) == sorted(batch)
    for key, value in batch.items():
        if isinstance(value, torch.Tensor):
            assert have[key].dtype == value.dtype and torch.equal(have[key], value), key
        else:
            assert have[key] == value, key


@pytest.mark.parametrize('dur_name,split', [('dur', 'train'), ('state_dur', 'train5')])
@pytest.mark.parametrize('by_speaker', [False, True], ids=['plain', 'per_speaker'])
def test_device_batches_computed_against_files(corpus, by_speaker, dur_name, split):
    """``DeviceBatches`` with a FrameCountersSource against the same loader over the twin directory's counters files (the host form's):
    ``counters``, ``normalised_counters`` and every other feature identical; one mg_frame_counters_f32 launch per batch."""
    root, names = corpus
    normalisers = _normalisers(root, by_speaker)
    by_file = data.FilesDataset(_sources(False, dur_name), split, 'ids.scp', normalisers, data_root=str(root))
    computed = data.FilesDataset(_sources(True, dur_name), split, 'ids.scp', normalisers, data_root=str(root))
    assert 'counters' not in computed.raw(0) and 'counters' in by_file.raw(0)
    _lib.CALL_LOG = log = []
    try:
        got = list(data.DeviceBatches(computed, 4, normalisers, DEV))
    finally:
        _lib.CALL_LOG = None
    assert log.count('mg_frame_counters_f32') == 2
    want = list(data.DeviceBatches(by_file, 4, normalisers, DEV))
    assert len(got) == len(want) == 2
    for have, batch in zip(got, want):
        assert have['counters'].shape == (len(have['name']), int(have['n_frames'].max()), 9) and 'normalised_counters' in have
        _same_batch(have, batch)
    # the specs as arguments, over utterances that are in host memory, give the same batch; data.batch takes them too
    raw = [computed.raw(i) for i in range(4)]
    direct = data.collate_to_device(raw, normalisers, DEV, counter_specs={'counters': data.CountersSpec(dur_name)})
    _same_batch(direct, got[0])
    _same_batch(next(iter(data.batch(computed, batch_size=4, shuffle=False, device=DEV))), got[0])
    # without n_frames in the utterances T is the largest sum of durations: here the same number
    bare = [{k: v for k, v in item.items() if k != 'n_frames'} for item in raw]
    direct = data.collate_to_device(bare, normalisers, DEV, counter_specs={'counters': data.CountersSpec(dur_name)})
    assert torch.equal(direct['counters'], got[0]['counters']) and torch.equal(direct['normalised_counters'], got[0]['normalised_counters'])
    # n_frames shorter than the durations' sum cuts the counters as it cuts every other feature's valid frames
    short = [dict(item, n_frames=item['n_frames'] - 7) for item in raw]
    cut = data.collate_to_device(short, normalisers, DEV, counter_specs={'counters': data.CountersSpec(dur_name)})
    for b, item in enumerate(short):
        n = item['n_frames']
        assert torch.equal(cut['counters'][b, :n], got[0]['counters'][b, :n]) and bool((cut['counters'][b, n:] == 0).all())
        assert bool((cut['normalised_counters'][b, n:] == 0).all())
    # a batch that carries the feature as well, and durations that are missing
    with pytest.raises(ValueError, match='read from files or computed'):
        data.collate_to_device([by_file.raw(0)], normalisers, DEV, counter_specs={'counters': data.CountersSpec(dur_name)})
    with pytest.raises(KeyError):
        data.collate_to_device(raw, normalisers, DEV, counter_specs={'counters': data.CountersSpec('phone_dur')})
    # the host path of the same dataset gives the file's values
    np.testing.assert_array_equal(_bits(computed[2]['counters']), _bits(np.load(root / split / 'counters' / 'utt02.npy')))


@pytest.mark.parametrize('dur_name,split', [('dur', 'train'), ('state_dur', 'train5')])
@pytest.mark.parametrize('by_speaker', [False, True], ids=['plain', 'per_speaker'])
def test_fit_normalisers_computed_against_files(corpus, by_speaker, dur_name, split):
    """The min and max fitted from counters computed on the device equal those fitted from the twin directory's files exactly (and so
    do the frame counts)."""
    root, names = corpus
    results = {}
    for computed in (False, True):
        normalisers = {'counters': _normalisers(root, by_speaker, fitted=False)['counters']}
        sources = {k: v for k, v in _sources(computed, dur_name).items() if k in ('counters', 'speaker_id', dur_name)}
        dataset = data.FilesDataset(sources, split, 'ids.scp', normalisers, data_root=str(root))
        results[computed] = (data.fit_normalisers(dataset, normalisers, device=DEV, batch_size=4)['counters'], normalisers['counters'])
    (want, file_normaliser), (got, normaliser) = results[False], results[True]
    for key in ('count', 'mmin', 'mmax'):
        np.testing.assert_array_equal(got[key], want[key])
    assert got['count'].shape == (2 if by_speaker else 1, 9) and got['count'][:, 0].sum() == want['count'][:, 0].sum() > 6 * 30
    np.testing.assert_allclose(got['mean'], want['mean'], rtol=1e-11)          # float64 sums of < 1000 frames in another order: n * 2^-53
    if by_speaker:
        for a, b in zip(normaliser.tables(DEV), file_normaliser.tables(DEV)):
            assert torch.equal(a, b)
    else:
        for key in ('mmin', 'mmax'):
            np.testing.assert_array_equal(normaliser.fetch_params()[key], file_normaliser.fetch_params()[key])
    with pytest.raises(ValueError, match='no deltas'):
        data.fit_normalisers([{'dur': np.array([[3], [2]])}], {'counters': data.MinMaxNormaliser('counters', use_deltas=True)}, device=DEV,
                             counter_specs={'counters': data.CountersSpec()})


def test_gru_f0_model_trains_one_step_on_computed_counters(corpus):
    """models.GRUF0Model on a small input width: one training step from a DeviceBatches batch whose counters were computed gives the loss
    and the updated parameters of the step from the twin directory's batch, bit for bit - its inputs are bit-equal."""
    root, names = corpus
    normalisers = _normalisers(root, False)
    outcome = []
    for computed in (False, True):
        dataset = data.FilesDataset(_sources(computed, 'dur'), 'train', 'ids.scp', normalisers, data_root=str(root))
        batch = next(iter(data.DeviceBatches(dataset, 4, normalisers, DEV)))
        torch.manual_seed(11)
        model = models.GRUF0Model(input_dim=LAB_DIM + 9, precision='fp32', generate=False).to(DEV)
        optimiser = optim.Adam(model.parameters(), lr=0.01)
        loss, _ = model(batch)
        loss.backward()
        optimiser.step()
        ops.check_persistent_status()
        assert bool(torch.isfinite(loss))
        outcome.append([loss.detach().clone()] + [p.detach().clone() for p in model.parameters()])
    assert len(outcome[0]) == len(outcome[1]) > 4
    for a, b in zip(*outcome):
        assert torch.equal(a, b)
