"""K23 on the device: mg_deltas_f32 / ops.deltas / data.compute_deltas and the loaders that use them, against tests/deltas_ref64.py.
Every expectation and every bound comes from that helper (exact rational arithmetic; derived there, not from what the kernel returns)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import deltas_ref64 as ref
from morgana_amd import _lib, data, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = np.float32(7.5e33)
WINDOWS = {'default': ref.DEFAULT_WINDOWS, 'static': ref.STATIC_WINDOW, '5pt': ref.WINDOWS_5PT}
# An empty item, the lengths below every window (1, 2, 3), the edges of a wave, an item over several trips of a workgroup - and one
# item ONE FRAME LONGER THAN TWO ROW CHUNKS of the kernel.  The kernel cuts the destination rows into chunks of
# mg_deltas_chunk_rows(D) = max(1, (2048 if D % 4 == 0 else 256) // D) rows: 256 rows at D = 1, 512 at D = 4, 51 at D = 5, 34 at D = 60.
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 257)
WIDTHS = (1, 4, 5, 60)


def _chunk_rows(width):
    return max(1, (2048 if width % 4 == 0 else 256) // width)


@functools.lru_cache(maxsize=None)
def _case(width):
    """Items float32 (len, width) ~ N(5, 2), the empty one in the middle; made once and never written to."""
    rng = np.random.RandomState(300 + width)
    lengths = LENGTHS[4:] + (2 * _chunk_rows(width) + 1,) + LENGTHS[:4]
    items = tuple((rng.randn(n, width) * 2.0 + 5.0).astype(np.float32) for n in lengths)
    for x in items:
        x.setflags(write=False)
    assert ref.exponent_span(np.concatenate(items)) < 29
    return items


@functools.lru_cache(maxsize=None)
def _want(width, windows, edge):
    """The helper's (exact, rounded, S) of every item of ``_case(width)``, back to back."""
    parts = [ref.reference(x, WINDOWS[windows], edge) for x in _case(width)]
    return tuple(np.concatenate([p[i] for p in parts], axis=0) for i in range(3))


def _guarded(values, lead):
    """A device allocation of GUARD with ``values`` (float32, flat) starting ``lead`` floats in: (whole allocation, address of the view)."""
    whole = np.full(lead + values.size + 5, GUARD, dtype=np.float32)
    whole[lead:lead + values.size] = values.reshape(-1)
    dev = torch.from_numpy(whole).to(DEV)
    return dev, dev.data_ptr() + 4 * lead


def _guards_untouched(whole, lead, used):
    host = whole.cpu().numpy()
    return bool(np.all(host[:lead] == GUARD) and np.all(host[lead + used:] == GUARD))


def _launch(items, windows, edge, in_form, out_form, lead):
    """mg_deltas_f32 through the C ABI on views that start ``lead`` floats into guarded allocations; the padded input holds NaN past
    every length, the padded output is T = longest + 3 frames.  Returns the valid rows of every item back to back, (N, W*D), after
    checking the guards, and - padded output - that every pad frame is exactly zero."""
    lib = _lib.load()
    width, n_win = items[0].shape[1], len(windows)
    lens = [len(x) for x in items]
    longest, total = max(lens), sum(lens)
    win_l, win_u, win_c = ops._window_arrays(windows)
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
    rows = t_out if out_form == 'padded' else total
    n_out = (len(items) * t_out if out_form == 'padded' else total) * n_win * width
    whole_out, out_ptr = _guarded(np.full(n_out, GUARD, dtype=np.float32), lead)
    _lib.check(lib.mg_deltas_f32(x_ptr, width, len(items), None if offsets is None else offsets.data_ptr(),
                                 None if seq_len is None else seq_len.data_ptr(), t_in, n_win, win_l, win_u, win_c, ops.DELTAS_EDGES[edge],
                                 None, None, None, 0, -1, _lib.MG_DELTAS_OUT_PADDED if out_form == 'padded' else _lib.MG_DELTAS_OUT_PACKED,
                                 rows, out_ptr, None, None), 'mg_deltas_f32')
    torch.cuda.synchronize()
    assert _guards_untouched(whole_out, lead, n_out), 'the kernel wrote outside its output'
    assert _guards_untouched(whole_in, lead, source.size)
    got = whole_out.cpu().numpy()[lead:lead + n_out]
    if out_form == 'packed':
        return got.reshape(total, n_win * width)
    got = got.reshape(len(items), t_out, n_win * width)
    for i, n in enumerate(lens):
        assert np.all(got[i, n:] == 0.0) and not np.any(np.signbit(got[i, n:])), 'pad frames of item %d are not zero' % i
    return np.concatenate([got[i, :n] for i, n in enumerate(lens)], axis=0)


@pytest.mark.parametrize('edge', ['replicate', 'zero'])
@pytest.mark.parametrize('windows', ['default', 'static', '5pt'])
@pytest.mark.parametrize('width', WIDTHS)
def test_kernel_against_exact_arithmetic(width, windows, edge):
    """Every input form x output form, on views 3 floats into their allocations (the scalar path whatever D) and 4 floats in (16-byte
    aligned: the vector path for D = 4 and 60).  Default and static windows: bit for bit the correctly rounded float32; 5-point windows:
    |got - exact| <= 2^-24 |exact| + 2^-50 S."""
    assert _lib.load().mg_deltas_chunk_rows(width) == _chunk_rows(width)
    items, want = _case(width), _want(width, windows, edge)
    assert 2 * _chunk_rows(width) + 1 in [len(x) for x in items]
    must_be_rounded = ref.exact_windows(WINDOWS[windows])
    for lead in (3, 4):
        for in_form in ('packed', 'padded'):
            for out_form in ('packed', 'padded'):
                got = _launch(items, WINDOWS[windows], edge, in_form, out_form, lead)
                bad = ref.misses(got, want, must_be_rounded)
                differ = int(np.sum(got != want[1]))
                print('D=%d %s %s lead=%d %s -> %s: %d of %d elements are not the correctly rounded float32, %d outside the bound' % (
                    width, windows, edge, lead, in_form, out_form, differ, got.size, len(bad)))
                assert not bad, (lead, in_form, out_form, bad[:5])


def _packed(items):
    packed = torch.from_numpy(np.concatenate(items)).to(DEV)
    offsets = torch.from_numpy(np.cumsum([0] + [len(x) for x in items]).astype(np.int64)).to(DEV)
    return packed, offsets


def _params(rng, kind, shape):
    lo = rng.randn(*shape).astype(np.float32)
    return torch.from_numpy(lo).to(DEV), torch.from_numpy(lo + np.abs(rng.randn(*shape)).astype(np.float32) + np.float32(0.1)).to(DEV)


@pytest.mark.parametrize('kind', ['mvn', 'minmax'])
@pytest.mark.parametrize('width', [4, 5])
def test_normalised_twin_is_the_normaliser_on_the_raw_output(width, kind):
    """norm_out bit for bit ops.normalise (plain) / ops.normalise_items (tables) of the SAME call's raw_out, in the packed and the padded
    form; pad frames zero; a bad item_row gives NaN in that item's valid frames and nowhere else."""
    items = _case(width)
    lens = [len(x) for x in items]
    code = data._KINDS[kind]['forward']
    rng = np.random.RandomState(width)
    packed, offsets = _packed(items)
    t = max(lens) + 3
    cols = 3 * width
    p0, p1 = _params(rng, kind, (cols,))
    raw, norm = ops.deltas(packed, ref.DEFAULT_WINDOWS, offsets=offsets, packed_rows=packed.shape[0], p0=p0, p1=p1, kind=code)
    assert torch.equal(norm, ops.normalise(raw, p0, p1, code))
    raw, norm = ops.deltas(packed, ref.DEFAULT_WINDOWS, offsets=offsets, t=t, p0=p0, p1=p1, kind=code)
    twin = ops.normalise(raw, p0, p1, code)
    for i, n in enumerate(lens):
        assert torch.equal(norm[i, :n], twin[i, :n]) and torch.all(norm[i, n:] == 0) and torch.all(raw[i, n:] == 0)
    alone = ops.deltas(packed, ref.DEFAULT_WINDOWS, offsets=offsets, t=t, p0=p0, p1=p1, kind=code, want_raw=False)
    assert alone[0] is None and torch.equal(alone[1], norm)
    # tables: three speakers, item 2 and the item of more than two chunks (4) name none
    t0, t1 = _params(rng, kind, (3, cols))
    rows = [0, 2, 7, 1, -1, 2, 0, 1, 2]
    assert len(rows) == len(items) and lens[4] > 2 * _chunk_rows(width) and lens[2] > 0
    item_row = torch.tensor(rows, dtype=torch.int32, device=DEV)
    raw, norm = ops.deltas(packed, ref.DEFAULT_WINDOWS, offsets=offsets, t=t, p0=t0, p1=t1, kind=code, item_row=item_row)
    twin = ops.normalise_items(raw, t0, t1, item_row, code)
    plain = ops.deltas(packed, ref.DEFAULT_WINDOWS, offsets=offsets, t=t)[0]
    assert torch.equal(raw, plain)                        # the raw output never sees the tables
    for i, n in enumerate(lens):
        if 0 <= rows[i] < 3:
            assert torch.equal(norm[i, :n], twin[i, :n]) and not torch.isnan(norm[i]).any()
        else:
            assert torch.isnan(norm[i, :n]).all()
        assert torch.all(norm[i, n:] == 0)
    raw, norm = ops.deltas(packed, ref.DEFAULT_WINDOWS, offsets=offsets, packed_rows=packed.shape[0], p0=t0, p1=t1, kind=code, item_row=item_row)
    bounds = np.cumsum([0] + lens)
    for i, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        if 0 <= rows[i] < 3:
            one = torch.full((1,), rows[i], dtype=torch.int32, device=DEV)
            assert torch.equal(norm[lo:hi], ops.normalise_items(raw[lo:hi][None], t0, t1, one, code)[0])
        else:
            assert torch.isnan(norm[lo:hi]).all()


@pytest.mark.parametrize('width', WIDTHS)
def test_static_window_alone_is_the_pad_pass(width):
    packed, offsets = _packed(_case(width))
    t = max(len(x) for x in _case(width)) + 3
    raw, norm = ops.deltas(packed, ref.STATIC_WINDOW, offsets=offsets, t=t)
    assert norm is None and torch.equal(raw, ops.pad_normalise(packed, offsets, t)[0])
    cut = ops.deltas(packed, ref.STATIC_WINDOW, offsets=offsets, t=64)[0]       # items longer than T are cut, as the pad pass cuts them
    assert torch.equal(cut, ops.pad_normalise(packed, offsets, 64)[0])


def test_compute_deltas_on_tensors():
    items = _case(5)
    lens = [len(x) for x in items]
    want = _want(5, 'default', 'replicate')[1]
    t = max(lens)
    body = np.full((len(items), t, 5), np.nan, dtype=np.float32)
    for i, x in enumerate(items):
        body[i, :len(x)] = x
    got = data.compute_deltas(torch.from_numpy(body).to(DEV), seq_len=torch.tensor(lens, device=DEV))
    assert got.shape == (len(items), t, 15) and got.dtype == torch.float32
    bounds = np.cumsum([0] + lens)
    for i, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        np.testing.assert_array_equal(got[i, :lens[i]].cpu().numpy(), want[lo:hi])
        assert torch.all(got[i, lens[i]:] == 0)
        if lens[i]:
            single = data.compute_deltas(torch.from_numpy(items[i]).to(DEV))
            np.testing.assert_array_equal(single.cpu().numpy(), want[lo:hi])
            np.testing.assert_array_equal(data.compute_deltas(items[i]), want[lo:hi])      # the host form: the same bits
    with pytest.raises(RuntimeError, match='no backward'):
        data.compute_deltas(torch.zeros((4, 5), device=DEV, requires_grad=True))


# ---------------------------------------------------------------------------------------------------------------- loader and fit
SPEAKERS = ('anna', 'bert')
FEATURES = (('lf0', 1), ('mcep', 4), ('bap', 5))


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    """7 utterances of 1-90 frames, two speakers: lf0, mcep, bap and integer dur - and, for the file-style loaders, the _deltas files
    written from the host form of compute_deltas."""
    root = tmp_path_factory.mktemp('deltas_corpus')
    rng = np.random.RandomState(77)
    names = ['utt%02d' % i for i in range(7)]
    for i, (name, frames) in enumerate(zip(names, (40, 1, 90, 2, 65, 3, 64))):
        for key, width in FEATURES:
            x = (rng.randn(frames, width) * 2.0 + 5.0).astype(np.float32)
            for folder, value in ((key, x), (key + '_deltas', data.compute_deltas(x))):
                os.makedirs(root / 'train' / folder, exist_ok=True)
                np.save(root / 'train' / folder / (name + '.npy'), value)
        os.makedirs(root / 'train' / 'dur', exist_ok=True)
        np.save(root / 'train' / 'dur' / (name + '.npy'), rng.randint(1, 9, size=(max(frames // 5, 1), 1)).astype(np.int64))
        os.makedirs(root / 'train' / 'speaker_id', exist_ok=True)
        (root / 'train' / 'speaker_id' / (name + '.txt')).write_text(SPEAKERS[i % 2] + '\n')
    (root / 'ids.scp').write_text('\n'.join(names) + '\n')
    (root / 'speakers.txt').write_text('\n'.join(SPEAKERS) + '\n')
    return root


def _sources(deltas):
    sources = {key: data.NumpyBinarySource(key, use_deltas=True, deltas=deltas) for key, _ in FEATURES}
    sources.update(dur=data.NumpyBinarySource('dur'), speaker_id=data.StringSource('speaker_id'))
    return sources


def _normalisers(root, by_speaker, fitted=True):
    rng = np.random.RandomState(5)
    out = {}
    for key, width in FEATURES:
        def group(cols):
            return {'mean': rng.randn(cols).astype(np.float32), 'std_dev': (rng.rand(cols) + 0.5).astype(np.float32)}
        if by_speaker:
            out[key] = data.SpeakerDependentMeanVarianceNormaliser(key, str(root / 'speakers.txt'), use_deltas=True)
            if fitted:
                out[key].set_params({s: group(width) for s in SPEAKERS}, {s: group(3 * width) for s in SPEAKERS})
        else:
            out[key] = data.MeanVarianceNormaliser(key, use_deltas=True)
            if fitted:
                out[key].set_params(group(width), group(3 * width))
    return out


@pytest.mark.parametrize('by_speaker', [False, True], ids=['plain', 'per_speaker'])
def test_device_batches_computed_against_files(corpus, by_speaker):
    """Every tensor of every file-style batch is torch.equal to the computed batch's.  The file-style loader has no normalised twin of
    the deltas it reads; the computed batch's twin is held to the normaliser applied to the deltas both batches agree on."""
    normalisers = _normalisers(corpus, by_speaker)
    by_file = data.FilesDataset(_sources('file'), 'train', 'ids.scp', normalisers, data_root=str(corpus))
    computed = data.FilesDataset(_sources('compute'), 'train', 'ids.scp', normalisers, data_root=str(corpus))
    assert 'lf0_deltas' in by_file.raw(0) and 'lf0_deltas' not in computed.raw(0)
    _lib.CALL_LOG = log = []
    try:
        got = list(data.DeviceBatches(computed, 3, normalisers, DEV))
    finally:
        _lib.CALL_LOG = None
    assert log.count('mg_deltas_f32') == 3 * len(FEATURES) and log.count('mg_host_pack') == 3 * len(FEATURES)      # no second upload
    want = list(data.DeviceBatches(by_file, 3, normalisers, DEV))
    assert len(got) == len(want) == 3
    for have, batch in zip(got, want):
        for key, value in batch.items():
            if isinstance(value, torch.Tensor):
                assert torch.equal(have[key], value), key
            else:
                assert have[key] == value, key
        lens = batch['lf0'].shape[1]
        for key, width in FEATURES:
            twin = have['normalised_%s_deltas' % key]
            assert twin.shape == batch[key + '_deltas'].shape == (batch[key].shape[0], lens, 3 * width)
            if by_speaker:
                p0, p1 = normalisers[key].tables(DEV, deltas=True)
                full = ops.normalise_items(batch[key + '_deltas'], p0, p1, batch['speaker_index'], ops.NORM_MVN)
            else:
                full = normalisers[key].normalise(batch[key + '_deltas'], deltas=True)
            valid = (batch[key + '_deltas'] != 0).any(dim=2, keepdim=True)      # N(5, 2) statics: a valid frame is never all zero
            assert torch.equal(twin, torch.where(valid, full, torch.zeros_like(full))), key
        assert sorted(set(have) - set(batch)) == sorted('normalised_%s_deltas' % key for key, _ in FEATURES)
    # the host path of the same dataset: FilesDataset.__getitem__ gives the same deltas
    item = computed[2]
    np.testing.assert_array_equal(item['mcep_deltas'], np.load(corpus / 'train' / 'mcep_deltas' / 'utt02.npy'))


@pytest.mark.parametrize('by_speaker', [False, True], ids=['plain', 'per_speaker'])
def test_fit_normalisers_computed_against_files(corpus, by_speaker):
    results, written = {}, {}
    for deltas in ('file', 'compute'):
        normalisers = _normalisers(corpus, by_speaker, fitted=False)
        dataset = data.FilesDataset(_sources(deltas), 'train', 'ids.scp', normalisers, data_root=str(corpus))
        out_dir = 'norm_%s_%s' % (deltas, by_speaker)
        results[deltas] = data.fit_normalisers(dataset, normalisers, device=DEV, batch_size=3, out_dir=out_dir, data_root=str(corpus))
        written[deltas] = {}
        for folder, _, files in os.walk(corpus / out_dir):
            for name in files:
                with open(os.path.join(folder, name)) as f:
                    written[deltas][os.path.relpath(os.path.join(folder, name), corpus / out_dir)] = json.load(f)
    assert sorted(results['file']) == sorted(results['compute']) == sorted([k for k, _ in FEATURES] + [k + '_deltas' for k, _ in FEATURES])
    for key, result in results['file'].items():
        for field, value in result.items():
            np.testing.assert_array_equal(results['compute'][key][field], value, err_msg='%s %s' % (key, field))
    assert len(written['file']) == 6 * (2 if by_speaker else 1) and written['compute'] == written['file']
    with pytest.raises(ValueError, match='read from files or computed'):
        data.fit_normalisers(data.FilesDataset(_sources('file'), 'train', 'ids.scp', {}, data_root=str(corpus)),
                             _normalisers(corpus, False, fitted=False), device=DEV, delta_specs={'lf0': data.DeltaSpec()})


# ---------------------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize('windows, lengths', [('default', (1, 2, 3, 65, 300)), ('5pt', (5, 65, 300))], ids=['default', '5pt'])
def test_mlpg_inverts_the_zero_edge_deltas(windows, lengths):
    """ops.mlpg(compute_deltas(x, edge='zero')) against x, unit variances, no burn-in, float64 out: pins the tap orientation to the
    reference-pinned MLPG.  With o = W x + r (r: the float32 rounding of the observations, from the helper) MLPG returns
    x + (W^T W)^-1 W^T r, and W^T W >= I because the static window is the identity: |got - x| <= ||W^T r||_2 per column, plus the 1e-11
    max|x| test_mlpg_vs_oracle grants the float64 solve.  A reversed window misses it by O(1)."""
    wins = WINDOWS[windows]
    width, t = 2, max(lengths)
    rng = np.random.RandomState(len(lengths))
    items = [(rng.randn(n, width) * 2.0 + 5.0).astype(np.float32) for n in lengths]
    body = np.zeros((len(items), t, width), dtype=np.float32)
    for i, x in enumerate(items):
        body[i, :len(x)] = x
    seq_len = torch.tensor(lengths, dtype=torch.int64, device=DEV)
    observed = data.compute_deltas(torch.from_numpy(body).to(DEV), wins, edge='zero', seq_len=seq_len)
    got = ops.mlpg(observed, torch.ones(len(wins) * width, device=DEV), wins, padding_size=0, seq_len=seq_len, out_dtype=torch.float64)
    got = got.cpu().numpy()
    for i, x in enumerate(items):
        n = len(x)
        want = ref.reference(x, wins, 'zero')
        np.testing.assert_array_equal(observed[i, :n].cpu().numpy()[:, :width], x)
        assert not ref.misses(observed[i, :n].cpu().numpy(), want, must_be_rounded=ref.exact_windows(wins))
        r = ref.residual(want)
        mats = ref.window_matrices(wins, n)
        for col in range(width):
            back = sum(mats[w].T @ r[:, w * width + col] for w in range(len(wins)))
            bound = np.linalg.norm(back) + 1e-11 * np.abs(x).max()
            miss = np.abs(got[i, :n, col] - x[:, col].astype(np.float64)).max()
            print('%s len %d column %d: max |mlpg(deltas(x)) - x| %.3g, bound %.3g' % (windows, n, col, miss, bound))
            assert miss <= bound
        assert np.all(got[i, n:] == 0)
