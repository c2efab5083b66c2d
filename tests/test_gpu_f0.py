"""K29 on the device: mg_continuous_lf0_f32 / ops.continuous_lf0 / data.continuous_lf0 and the loaders that use them, against
tests/f0_ref64.py.  Every expectation and every bound comes from that helper (long-double arithmetic; the bound is derived there from
the number formats, not from what the kernel returns).

Measured on an MI355X (printed by the tests; recorded in DESIGN.md section 4.25): see there."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import colstats_ref64 as cref
import f0_ref64 as ref
from morgana_amd import _lib, data, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = np.float32(7.5e33)
CHUNK = 256                      # mg_continuous_lf0_chunk_rows(): frames of one column a workgroup takes per trip
WIDTHS = (1, 3, 4)               # (no 16-byte path in this kernel: D = 4 takes the one path there is)


@functools.lru_cache(maxsize=None)
def _case(width, log_input=False):
    items = ref.case(width, CHUNK)[0]
    return ref.log_case(items) if log_input else items


@functools.lru_cache(maxsize=None)
def _want(width, log_input=False):
    """(ref, vuv, bound) of every item of ``_case``, back to back: made once, never written to."""
    parts = [ref.reference(x, log_input=log_input) for x in _case(width, log_input)]
    want = np.concatenate([p[0] for p in parts], axis=0)
    vuv = np.concatenate([p[1] for p in parts], axis=0)
    limit = np.concatenate([ref.bound(p[0], p[2], p[3], log_input) for p in parts], axis=0)
    for a in (want, vuv, limit):
        a.setflags(write=False)
    return want, vuv, limit


def _guarded(values, lead):
    """A device allocation of GUARD with ``values`` (float32, flat) starting ``lead`` floats in: (whole allocation, address of the view)."""
    whole = np.full(lead + values.size + 5, GUARD, dtype=np.float32)
    whole[lead:lead + values.size] = values.reshape(-1)
    dev = torch.from_numpy(whole).to(DEV)
    return dev, dev.data_ptr() + 4 * lead


def _inside(whole, lead, used):
    host = whole.cpu().numpy()
    assert np.all(host[:lead] == GUARD) and np.all(host[lead + used:] == GUARD), 'the kernel wrote outside an output'
    return host[lead:lead + used]


def _launch(items, in_form, outputs, lead, log_input=False, params=None, fill=0.0):
    """mg_continuous_lf0_f32 through the C ABI on views that start ``lead`` floats into guarded allocations; the padded input holds NaN
    past every length and has T_in = longest + 2, the padded outputs have longest + 3 frames.  ``outputs``: a subset of 'packed',
    'padded', 'norm', 'vuv_padded', 'vuv_packed'.  Returns {output: the valid rows of every item back to back, (N, D)} after checking
    the guards and that every pad frame of a padded output is exactly +0."""
    lib = _lib.load()
    width = items[0].shape[1]
    lens = [len(x) for x in items]
    longest, total = max(lens), sum(lens)
    offsets = seq_len = None
    t_in = 0
    if in_form == 'packed':
        source = np.concatenate(items).reshape(-1)
        offsets = torch.from_numpy(np.cumsum([0] + lens).astype(np.int64)).to(DEV)
    else:
        t_in = longest + 2
        body = np.full((len(items), t_in, width), np.nan, dtype=np.float32)
        for i, x in enumerate(items):
            body[i, :len(x)] = x
        source = body.reshape(-1)
        seq_len = torch.tensor(lens, dtype=torch.int64, device=DEV)
    whole_in, x_ptr = _guarded(source, lead)
    t_out = longest + 3
    sizes = {'packed': total * width, 'vuv_packed': total * width}
    held = {name: _guarded(np.full(sizes.get(name, len(items) * t_out * width), GUARD, dtype=np.float32), lead) for name in outputs}
    ptr = {name: held[name][1] if name in held else None for name in ('packed', 'padded', 'norm', 'vuv_padded', 'vuv_packed')}
    kind, p0, p1, item_row, s = -1, None, None, None, 0
    if params is not None:
        kind, p0, p1, item_row = params
        s = p0.shape[0] if item_row is not None else 0
    vuv_ptr = ptr['vuv_padded'] or ptr['vuv_packed']
    _lib.check(lib.mg_continuous_lf0_f32(x_ptr, width, len(items), None if offsets is None else offsets.data_ptr(),
                                         None if seq_len is None else seq_len.data_ptr(), t_in, int(log_input),
                                         float(ref.threshold(None, log_input)), fill, None if p0 is None else p0.data_ptr(),
                                         None if p1 is None else p1.data_ptr(), None if item_row is None else item_row.data_ptr(), s, kind,
                                         t_out, total, ptr['packed'], ptr['padded'], ptr['norm'], vuv_ptr,
                                         _lib.MG_F0_VUV_PACKED if ptr['vuv_packed'] else _lib.MG_F0_VUV_PADDED, None),
               'mg_continuous_lf0_f32')
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_inside(whole_in, lead, source.size), source)
    got = {}
    for name in outputs:
        flat = _inside(held[name][0], lead, sizes.get(name, len(items) * t_out * width))
        if name in sizes:
            got[name] = flat.reshape(total, width)
            continue
        body = flat.reshape(len(items), t_out, width)
        for i, n in enumerate(lens):
            assert np.all(body[i, n:] == 0.0) and not np.any(np.signbit(body[i, n:])), 'pad frames of item %d of %s are not zero' % (i, name)
        got[name] = np.concatenate([body[i, :n] for i, n in enumerate(lens)], axis=0)
    return got


def _output_sets():
    """Every combination of the optional outputs: packed lf0, padded lf0, the normalised twin, vuv in neither / the padded / the packed
    form - without the empty one."""
    sets = []
    for packed, padded, norm, vuv in itertools.product((False, True), (False, True), (False, True), (None, 'vuv_padded', 'vuv_packed')):
        names = [n for n, on in (('packed', packed), ('padded', padded), ('norm', norm)) if on] + ([vuv] if vuv else [])
        if names:
            sets.append(tuple(names))
    return sets


@pytest.mark.parametrize('width', WIDTHS)
def test_kernel_against_the_reference(width):
    """Both input forms x every output combination, on views 3 floats (one float off a 16-byte boundary) and 4 floats (aligned) into
    their allocations.  lf0 within the bound of f0_ref64 in every form it is written in, vuv exact, the normalised twin bit for bit
    the normaliser's arithmetic on the same launch's lf0, pad frames +0, guards untouched, two calls the same bits."""
    assert _lib.load().mg_continuous_lf0_chunk_rows() == CHUNK
    items = _case(width)
    assert 2 * CHUNK + 1 in [len(x) for x in items] and ref.adjacent_pairs(items) == (True, True)
    want, vuv, limit = _want(width)
    rng = np.random.RandomState(width)
    p0 = torch.from_numpy(rng.randn(width).astype(np.float32) + 5).to(DEV)
    p1 = torch.from_numpy((rng.rand(width) + 0.5).astype(np.float32)).to(DEV)
    worst, differ = 0.0, 0
    host = np.concatenate([data.continuous_lf0(x)[0] for x in items], axis=0)
    first = _launch(items, 'packed', ('packed',), 4)['packed']      # what every later lf0, in whatever form, must repeat bit for bit
    twin = ops.normalise(torch.from_numpy(first).to(DEV), p0, p1, ops.NORM_MVN).cpu().numpy()
    for lead in (3, 4):
        for in_form in ('packed', 'padded'):
            for outputs in _output_sets():
                got = _launch(items, in_form, outputs, lead, params=(ops.NORM_MVN, p0, p1, None) if 'norm' in outputs else None)
                for name in outputs:
                    if name in ('packed', 'padded'):
                        bad = ref.misses(got[name], want, limit)
                        assert not bad, (lead, in_form, outputs, name, bad[:5])
                        worst = max(worst, ref.worst_ratio(got[name], want, limit))
                        differ = max(differ, int(np.sum(got[name] != host)))
                        np.testing.assert_array_equal(got[name], first, err_msg='%s of %s, %s, lead %d' % (name, outputs, in_form, lead))
                    elif name == 'norm':
                        np.testing.assert_array_equal(got[name], twin)
                    else:
                        np.testing.assert_array_equal(got[name], vuv)
    print('D=%d: largest |lf0 - reference| / bound = %.3f over %d elements; %d of them differ from the host form (its log is libm\'s)' % (
        width, worst, want.size, differ))


@pytest.mark.parametrize('width', WIDTHS)
def test_log_input_is_bit_equal_to_the_host_form(width):
    items = _case(width, True)
    assert any((x == np.float32(-1e10)).any() for x in items) and any(np.isnan(x).any() for x in items)
    want, vuv, limit = _want(width, True)
    host = [data.continuous_lf0(x, log_input=True, fill=-2.5) for x in items]
    host_lf0, host_vuv = (np.concatenate([h[i] for h in host], axis=0) for i in (0, 1))
    np.testing.assert_array_equal(host_vuv, vuv)
    for in_form in ('packed', 'padded'):
        got = _launch(items, in_form, ('packed', 'padded', 'vuv_packed'), 3, log_input=True, fill=-2.5)
        np.testing.assert_array_equal(got['packed'], host_lf0)
        np.testing.assert_array_equal(got['padded'], host_lf0)
        np.testing.assert_array_equal(got['vuv_packed'], vuv)
    # a column of an item without a voiced frame is `fill`; everything else is held to the reference (whose fill is 0)
    filled = np.concatenate([np.broadcast_to(~(x > -1e9).any(axis=0, keepdims=True), x.shape) for x in items if len(x)])
    assert np.all(host_lf0[filled] == np.float32(-2.5)) and filled.any()
    rest = ~filled
    assert not ref.misses(host_lf0[rest], want[rest], limit[rest])


def test_neighbouring_items_do_not_leak():
    """A packed batch: [ends unvoiced][starts voiced] and [ends voiced][starts unvoiced].  Each item's result is what it is alone: the
    trailing run of the first holds ITS last voiced value, the leading run of the last holds ITS first voiced value."""
    a = np.float32([[100.0], [0.0], [0.0]])
    b = np.float32([[400.0], [300.0]])
    c = np.float32([[0.0], [0.0], [50.0]])
    d = np.float32([[0.0]] * 70)
    items = (a, b, c, d, b, a)
    alone = [_launch((x,), 'packed', ('packed', 'vuv_packed'), 3) for x in items]
    got = _launch(items, 'packed', ('packed', 'vuv_packed'), 3, fill=-1.0)
    np.testing.assert_array_equal(got['vuv_packed'], np.concatenate([r['vuv_packed'] for r in alone]))
    want = np.concatenate([np.full(x.shape, np.float32(-1.0)) if not (x > 0).any() else r['packed'] for x, r in zip(items, alone)])
    np.testing.assert_array_equal(got['packed'], want)
    np.testing.assert_array_equal(got['packed'][:3, 0], np.full(3, np.float32(np.log(np.float64(100.0)))))
    np.testing.assert_array_equal(got['packed'][5:8, 0], np.full(3, np.float32(np.log(np.float64(50.0)))))


@pytest.mark.parametrize('kind', ['mvn', 'minmax'])
def test_normalised_twin_plain_and_with_tables(kind):
    """norm_out bit for bit ops.normalise (plain) / ops.normalise_items (tables) of the SAME call's lf0; pad frames zero; an item_row
    outside the tables gives NaN in that item's valid frames and nowhere else."""
    width = 3
    items = _case(width)
    lens = [len(x) for x in items]
    code = data._KINDS[kind]['forward']
    rng = np.random.RandomState(11)
    packed = torch.from_numpy(np.concatenate(items)).to(DEV)
    offsets = torch.from_numpy(np.cumsum([0] + lens).astype(np.int64)).to(DEV)
    t = max(lens) + 3

    def params(shape):
        lo = (rng.randn(*shape) + 5).astype(np.float32)
        return torch.from_numpy(lo).to(DEV), torch.from_numpy(lo + np.abs(rng.randn(*shape)).astype(np.float32) + np.float32(0.1)).to(DEV)

    p0, p1 = params((width,))
    lf0, norm, vuv, track = ops.continuous_lf0(packed, offsets=offsets, t=t, want_packed=True, p0=p0, p1=p1, kind=code)
    twin = ops.normalise(lf0, p0, p1, code)
    bounds = np.cumsum([0] + lens)
    for i, n in enumerate(lens):
        assert torch.equal(norm[i, :n], twin[i, :n]) and torch.all(norm[i, n:] == 0) and torch.all(lf0[i, n:] == 0) and torch.all(vuv[i, n:] == 0)
        assert torch.equal(track[bounds[i]:bounds[i + 1]], lf0[i, :n])
    t0, t1 = params((3, width))
    rows = [i % 3 for i in range(len(items))]
    longest = lens.index(2 * CHUNK + 1)
    rows[longest], rows[0] = -1, 3
    assert lens[0] > 0
    item_row = torch.tensor(rows, dtype=torch.int32, device=DEV)
    again, norm, _, _ = ops.continuous_lf0(packed, offsets=offsets, t=t, p0=t0, p1=t1, kind=code, item_row=item_row)
    assert torch.equal(again, lf0)                          # lf0 never sees the tables
    twin = ops.normalise_items(lf0, t0, t1, item_row, code)
    for i, n in enumerate(lens):
        if 0 <= rows[i] < 3:
            assert torch.equal(norm[i, :n], twin[i, :n]) and not torch.isnan(norm[i]).any()
        else:
            assert torch.isnan(norm[i, :n]).all()
        assert torch.all(norm[i, n:] == 0)


def test_continuous_lf0_on_tensors():
    items = _case(3)
    lens = [len(x) for x in items]
    want, vuv, limit = _want(3)
    t = max(lens)
    body = np.full((len(items), t, 3), np.nan, dtype=np.float32)
    for i, x in enumerate(items):
        body[i, :len(x)] = x
    lf0, flag = data.continuous_lf0(torch.from_numpy(body).to(DEV), seq_len=torch.tensor(lens))
    assert lf0.shape == flag.shape == body.shape
    valid = np.concatenate([lf0[i, :n].cpu().numpy() for i, n in enumerate(lens)])
    assert not ref.misses(valid, want, limit)
    np.testing.assert_array_equal(np.concatenate([flag[i, :n].cpu().numpy() for i, n in enumerate(lens)]), vuv)
    for i, n in enumerate(lens):
        assert torch.all(lf0[i, n:] == 0) and torch.all(flag[i, n:] == 0)
    longest = lens.index(t)
    one, one_flag = data.continuous_lf0(torch.from_numpy(items[longest].copy()).to(DEV))
    assert torch.equal(one, lf0[longest]) and torch.equal(one_flag, flag[longest])
    # an item cut by the padded output still interpolates towards the frames behind the cut
    cut = ops.continuous_lf0(torch.from_numpy(items[longest].copy()).to(DEV)[None], seq_len=torch.tensor([t], device=DEV), t=100)[0]
    assert torch.equal(cut[0], lf0[longest, :100])
    with pytest.raises(ValueError):
        ops.continuous_lf0(torch.from_numpy(body).to(DEV), seq_len=torch.tensor(lens, device=DEV))
    with pytest.raises(ValueError, match='NaN'):
        ops.continuous_lf0(torch.from_numpy(body).to(DEV), seq_len=torch.tensor(lens, device=DEV), t=t, voiced_above=float('nan'))


def test_capture_and_replay_of_the_bare_launch():
    """One capture of ops.continuous_lf0 on ops-level tensors, replayed on new inputs written into the captured buffers."""
    first, second = _case(1), ref.case(1, CHUNK, seed=1)[0]
    lens = [len(x) for x in first]
    assert lens == [len(x) for x in second]
    offsets = torch.from_numpy(np.cumsum([0] + lens).astype(np.int64)).to(DEV)
    packed = torch.from_numpy(np.concatenate(first)).to(DEV)
    t = max(lens)
    eager_first = ops.continuous_lf0(packed, offsets=offsets, t=t, want_packed=True)
    eager_second = ops.continuous_lf0(torch.from_numpy(np.concatenate(second)).to(DEV), offsets=offsets, t=t, want_packed=True)
    assert not torch.equal(eager_first[0], eager_second[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.continuous_lf0(packed, offsets=offsets, t=t, want_packed=True)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, eager_first):
        assert (got is None and want is None) or torch.equal(got, want)
    packed.copy_(torch.from_numpy(np.concatenate(second)).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, eager_second):
        assert (got is None and want is None) or torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- loader and fit
SPEAKERS = ('anna', 'bert')
FRAMES = (40, 1, 90, 2, 65, 3, 300)


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    """7 utterances of 1-300 frames, two speakers: the raw f0 track (about 40 % unvoiced, in runs) and mcep - and, for the file-style
    loaders, the lf0 / vuv / lf0_deltas files written from the host forms."""
    root = tmp_path_factory.mktemp('f0_corpus')
    rng = np.random.RandomState(78)
    names = ['utt%02d' % i for i in range(len(FRAMES))]
    tracks = {}
    for i, (name, frames) in enumerate(zip(names, FRAMES)):
        f0 = (80.0 + 250.0 * rng.rand(frames, 1)).astype(np.float32)
        at = 0
        while at < frames:
            run = int(rng.randint(3, 40))
            if rng.rand() < 0.4:
                f0[at:at + run] = 0.0
            at += run
        if i == 1:
            f0[:] = 0.0                                     # an utterance without a voiced frame
        tracks[name] = f0
        lf0, vuv = data.continuous_lf0(f0)
        mcep = (rng.randn(frames, 4) * 2.0 + 5.0).astype(np.float32)
        for folder, value in (('f0', f0), ('lf0', lf0), ('vuv', vuv), ('lf0_deltas', data.compute_deltas(lf0)), ('mcep', mcep)):
            os.makedirs(root / 'train' / folder, exist_ok=True)
            np.save(root / 'train' / folder / (name + '.npy'), value)
        os.makedirs(root / 'train' / 'speaker_id', exist_ok=True)
        (root / 'train' / 'speaker_id' / (name + '.txt')).write_text(SPEAKERS[i % 2] + '\n')
    (root / 'ids.scp').write_text('\n'.join(names) + '\n')
    (root / 'speakers.txt').write_text('\n'.join(SPEAKERS) + '\n')
    return root, names, tracks


def _sources(computed):
    if computed:
        sources = {'lf0': data.ContinuousLF0Source('lf0', use_deltas=True)}
    else:
        sources = {'lf0': data.NumpyBinarySource('lf0', use_deltas=True), 'vuv': data.NumpyBinarySource('vuv')}
    sources.update(mcep=data.NumpyBinarySource('mcep'), speaker_id=data.StringSource('speaker_id'))
    return sources


def _normalisers(root, by_speaker, fitted=True):
    rng = np.random.RandomState(5)
    out = {}
    for key, width in (('lf0', 1), ('mcep', 4)):
        def group(cols):
            return {'mean': (rng.randn(cols) + 5).astype(np.float32), 'std_dev': (rng.rand(cols) + 0.5).astype(np.float32)}
        deltas = key == 'lf0'
        if by_speaker:
            out[key] = data.SpeakerDependentMeanVarianceNormaliser(key, str(root / 'speakers.txt'), use_deltas=deltas)
            if fitted:
                out[key].set_params({s: group(width) for s in SPEAKERS}, {s: group(3 * width) for s in SPEAKERS} if deltas else None)
        else:
            out[key] = data.MeanVarianceNormaliser(key, use_deltas=deltas)
            if fitted:
                out[key].set_params(group(width), group(3 * width) if deltas else None)
    return out


def _track_bounds(tracks, names):
    """Per utterance (reference, bound) of the continuous log-F0 and the bound of |device - host file| = both forms' bounds added."""
    out = {}
    for name in names:
        want, _, scale, interpolated = ref.reference(tracks[name])
        out[name] = (want, ref.bound(want, scale, interpolated))
    return out


DELTA_ABS_SUM = 1.0 + 2 * 0.5 + (1.0 + 2.0 + 1.0)          # sum |coefficient| of the default windows, at most (their largest row sum is 4)


@pytest.mark.parametrize('by_speaker', [False, True], ids=['plain', 'per_speaker'])
def test_device_batches_computed_against_files(corpus, by_speaker):
    """``DeviceBatches`` over the raw f0 track against the same loader over host-computed lf0 / vuv / lf0_deltas files: vuv and every
    other feature torch.equal; lf0 within the bound of f0_ref64 of the reference (the file's lf0 is within it too); the deltas
    within what that moves them by; the normalised twins bit for bit the normaliser on the same batch's raw feature.  One upload and
    one mg_continuous_lf0_f32 launch per batch."""
    root, names, tracks = corpus
    normalisers = _normalisers(root, by_speaker)
    by_file = data.FilesDataset(_sources(False), 'train', 'ids.scp', normalisers, data_root=str(root))
    computed = data.FilesDataset(_sources(True), 'train', 'ids.scp', normalisers, data_root=str(root))
    assert sorted(computed.raw(0)) == ['f0', 'mcep', 'name', 'speaker_id']
    _lib.CALL_LOG = log = []
    try:
        got = list(data.DeviceBatches(computed, 3, normalisers, DEV))
    finally:
        _lib.CALL_LOG = None
    assert log.count('mg_continuous_lf0_f32') == 3 and log.count('mg_deltas_f32') == 3 and log.count('mg_host_pack') == 2 * 3
    want = list(data.DeviceBatches(by_file, 3, normalisers, DEV))
    assert len(got) == len(want) == 3
    limits = _track_bounds(tracks, names)
    for have, batch in zip(got, want):
        assert 'f0' not in have
        assert sorted(set(have) - set(batch)) == ['normalised_lf0_deltas'] and not set(batch) - set(have)
        for key, value in batch.items():
            if key in ('lf0', 'normalised_lf0', 'lf0_deltas'):
                continue
            if isinstance(value, torch.Tensor):
                assert torch.equal(have[key], value), key
            else:
                assert have[key] == value, key
        lf0, deltas = have['lf0'].cpu().numpy(), have['lf0_deltas'].cpu().numpy()
        for i, name in enumerate(have['name']):
            reference, limit = limits[name]
            n = len(reference)
            assert not ref.misses(lf0[i, :n], reference, limit), name
            assert np.all(lf0[i, n:] == 0) and np.all(deltas[i, n:] == 0)
            moved = np.abs(lf0[i, :n] - batch['lf0'][i, :n].cpu().numpy()).max()
            assert moved <= 2 * limit.max()
            file_deltas = batch['lf0_deltas'][i, :n].cpu().numpy().astype(np.float64)
            slack = DELTA_ABS_SUM * 2 * limit.max() + 2 * (2.0 ** -24 * np.abs(file_deltas) + 2.0 ** -50 * DELTA_ABS_SUM * float(np.abs(reference).max()))
            assert np.all(np.abs(deltas[i, :n] - file_deltas) <= slack), name
        if by_speaker:
            (p0, p1), (d0, d1) = normalisers['lf0'].tables(DEV), normalisers['lf0'].tables(DEV, deltas=True)
            twin = ops.normalise_items(have['lf0'], p0, p1, have['speaker_index'], ops.NORM_MVN)
            twin_deltas = ops.normalise_items(have['lf0_deltas'], d0, d1, have['speaker_index'], ops.NORM_MVN)
        else:
            twin = normalisers['lf0'].normalise(have['lf0'])
            twin_deltas = normalisers['lf0'].normalise(have['lf0_deltas'], deltas=True)
        valid = torch.arange(have['lf0'].shape[1], device=DEV)[None, :, None] < torch.tensor(
            [len(tracks[name]) for name in have['name']], device=DEV)[:, None, None]
        assert torch.equal(have['normalised_lf0'], torch.where(valid, twin, torch.zeros_like(twin)))
        assert torch.equal(have['normalised_lf0_deltas'], torch.where(valid, twin_deltas, torch.zeros_like(twin_deltas)))
    # collate_to_device with the specs as arguments gives the same batch as the data sources' own
    raw = [computed.raw(i) for i in range(3)]
    direct = data.collate_to_device(raw, normalisers, DEV, delta_specs={'lf0': data.DeltaSpec()}, f0_specs={'lf0': data.F0Spec()})
    for key, value in got[0].items():
        assert torch.equal(direct[key], value) if isinstance(value, torch.Tensor) else direct[key] == value, key
    # the host path of the same dataset gives the file's values
    item = computed[2]
    np.testing.assert_array_equal(item['lf0'], np.load(root / 'train' / 'lf0' / 'utt02.npy'))
    np.testing.assert_array_equal(item['vuv'], np.load(root / 'train' / 'vuv' / 'utt02.npy'))


@pytest.mark.parametrize('by_speaker', [False, True], ids=['plain', 'per_speaker'])
def test_fit_normalisers_computed_against_host_files(corpus, by_speaker):
    """The statistics of lf0 and lf0_deltas fitted from the raw f0 track against colstats_ref64.two_pass over the host-computed files,
    ALL frames (interpolated ones included).  Bound: colstats_ref64.bounds (the statistics kernel against a two-pass over ITS
    input) plus what the input moves by - every element by at most e (lf0: both forms' f0_ref64 bounds; deltas: sum |c| times that,
    plus two float32 roundings), so the mean by <= e and the variance by <= 2 sqrt(var) e + e^2 (Cauchy-Schwarz)."""
    root, names, tracks = corpus
    normalisers = {'lf0': _normalisers(root, by_speaker, fitted=False)['lf0']}
    sources = {'lf0': data.ContinuousLF0Source('lf0', use_deltas=True), 'speaker_id': data.StringSource('speaker_id')}
    dataset = data.FilesDataset(sources, 'train', 'ids.scp', normalisers, data_root=str(root))
    results = data.fit_normalisers(dataset, normalisers, device=DEV, batch_size=3)
    assert sorted(results) == ['lf0', 'lf0_deltas']
    limit = max(b.max() for _, b in _track_bounds(tracks, names).values())
    item_row = [i % 2 for i in range(len(names))] if by_speaker else None
    groups = 2 if by_speaker else 1
    for key, moved in (('lf0', 2 * limit), ('lf0_deltas', DELTA_ABS_SUM * 2 * limit + 2 * 2.0 ** -24 * 8.0)):
        items = [np.load(root / 'train' / key / (name + '.npy')) for name in names]
        assert max(np.abs(x).max() for x in items) < 8.0
        want = cref.two_pass(items, item_row, groups)
        got = results[key]
        np.testing.assert_array_equal(got['count'], want['count'])
        assert got['count'].sum(axis=0)[0] == sum(FRAMES)
        bound_mean, bound_var = cref.bounds(items, want['count'], n_batches=3)
        err_mean, err_var = np.abs(got['mean'] - want['mean']), np.abs(got['var'] - want['var'])
        slack_var = 2 * np.sqrt(want['var']) * moved + moved ** 2
        print('%s: mean off by %.3e (bound %.3e + %.3e), var off by %.3e (bound %.3e + %.3e)' % (
            key, err_mean.max(), np.max(bound_mean), moved, err_var.max(), np.max(bound_var), np.max(slack_var)))
        assert np.all(err_mean <= bound_mean + moved) and np.all(err_var <= bound_var + slack_var)
    assert normalisers['lf0'].params is not None and normalisers['lf0'].delta_params is not None
    with pytest.raises(ValueError, match='read from files or computed'):
        both = dict(sources, files=data.NumpyBinarySource('lf0'))
        data.fit_normalisers(data.FilesDataset(both, 'train', 'ids.scp', {}, data_root=str(root)), normalisers, device=DEV)
    with pytest.raises(ValueError, match='name it in delta_specs'):
        data.fit_normalisers([{'f0': tracks[names[0]]}], {'lf0': data.MeanVarianceNormaliser('lf0', use_deltas=True)}, device=DEV,
                             f0_specs={'lf0': data.F0Spec()})
