"""K33 on the device: mg_spectrum_mcep and mg_aperiodicity_bap through ops / data, against tests/analysis_ref64.py.  Every bound is
derived from the number formats and the operation counts, never from what the kernel returns.  u = 2^-53 is the unit roundoff of
float64, U = 2^-24 that of float32.

mel-cepstrum   c[t,m] is a K-term float64 dot product of table[m,:] and l[t,:].  In any fixed order, fused or not, such a sum is
               within K u sum_k |table l| of the exact one to first order; 2 K u covers the second order and a pairwise or blocked
               order.  Each table entry carries one rounding (u), and the device logarithm is within 2 ulp of log(x): since
               l = 0.5 log(x) exactly halves it, that is 2 * 2 u |l| - the allowance csrc/f0.hip's test uses for the device log.
               Together (2 K + 1 + 4) u sum_k |table[m,k]| |l[t,k]| <= (2 K + 8) u sum_k |table| |l|, the issue's middle term; the
               reference's own error (an FFT and a recursion in float64, 4e-15 of max |c| on the host) lies inside the same term,
               which is 3e-12 at K = 1025 and 2.6e-14 at K = 5.  The float32 store adds one rounding to nearest, U |c|, and 2^-149
               where the result is subnormal.  Asserted:
                   |c^ - c| <= U |c| + (2 K + 8) u sum_k |table[m,k]| |l[t,k]| + 2^-149
               and the float64 output is held to the middle term alone.  With log_input the logarithm is the host's: the same bound.
round trip     K32 gives L^ with |L^ - L| <= (M + 2) U sum |c| (its own asserted bound); x = 2 L^ is exact and l = 0.5 x is L^ again.
               The analysis is linear in l, so the error of L^ reaches c through the table: at most max_m sum_k |table[m,k]| times it.
               table . basis^T = I to 2e-15 and the float64 contraction add less than 1e-13 sum |c|.
aperiodicity   dB(k) = clamp(20 log10(ap)) has magnitude <= 60: the device log10 is within 2 ulp and the product adds one rounding,
               3 u * 60 per value (the clamp does not increase an error).  The two values enter with weights 1 - w and w, which sum
               to 1: 180 u.  The difference carries one rounding (<= 60 u, times w <= 1) and the fma one (<= 60 u); w itself is one
               division, u on a factor of magnitude <= 60.  That is 360 u; the reference's own NumPy arithmetic is the same chain,
               so the two can differ by twice that: 720 u < 1024 u = 1.2e-13.  The float32 store adds U |bap|.  Asserted:
                   |bap^ - bap| <= U |bap| + 1024 u."""
import functools
import os

import numpy as np
import pytest
import torch

import analysis_ref64 as ref
import vocoder_ref64 as voc
from morgana_amd import _lib, data, ops, viz

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = 2.0 ** -24
u = 2.0 ** -53
CANARY = 7.5e33
SETTINGS = ((1, 8, 0.0), (3, 8, 0.42), (25, 512, 0.42), (60, 2048, 0.77), (61, 1024, 0.58), (128, 64, 0.3))
IDS = ['M%d-F%d-a%g' % s for s in SETTINGS]
IDENTITY_SETTINGS = ((60, 2048, 0.77), (25, 1024, 0.58), (60, 1024, 0.58), (40, 512, 0.42))
KINDS = ('cepstral', 'white')
NP_OF = {torch.float32: np.float32, torch.float64: np.float64}


def _tile():
    return _lib.load().mg_analysis_tile_frames()


def _lengths():
    tile = _tile()
    return [0, 1, 3, tile - 1, tile, tile + 1]


def _offsets(lens):
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the cached cases are read-only


def _with_canary(rows, cols, dtype=torch.float32, extra=3):
    return torch.full((rows + extra, cols), CANARY, dtype=dtype, device=DEV)


def _check_canary(out, rows):
    assert torch.all(out[rows:] == CANARY), 'rows from packed_rows on were written'
    return out[:rows]


def _cepstra(rng, n, order):
    c = rng.randn(n, order) / np.maximum(np.arange(order), 1)[None, :]
    c[:, 0] = rng.uniform(-4, 4, size=n)
    return c


@functools.lru_cache(maxsize=None)
def _table(order, fft_size, alpha):
    table = ops.mcep_analysis_table(order, alpha, fft_size)
    table.setflags(write=False)
    return table


@functools.lru_cache(maxsize=None)
def _spectrum_case(order, fft_size, alpha, kind, in_dtype):
    """(lengths, packed power spectrum as in_dtype, reference c float64 of that rounded input, the bound's sum_k |table| |l|): made
    once, never written to.  'cepstral': exp(2 L) of decaying random cepstra; 'white': the log spectrum uniform in [-20, 5] per bin."""
    rng = np.random.RandomState(1000 * order + fft_size + (7 if kind == 'white' else 0))
    lens = _lengths()
    rows, k = sum(lens), fft_size // 2 + 1
    if kind == 'cepstral':
        log_sp = 2.0 * voc.log_spectrum(_cepstra(rng, rows, order), alpha, fft_size)
        assert np.max(np.abs(log_sp)) < 80, 'the case would leave float32'
    else:
        log_sp = rng.uniform(-20.0, 5.0, size=(rows, k))
    sp = np.exp(log_sp).astype(in_dtype)
    l = 0.5 * np.log(sp.astype(np.float64))
    want = ref.mcep_of_half_log(l, order, alpha, fft_size)
    weight = np.abs(l) @ np.abs(_table(order, fft_size, alpha)).T
    for a in (sp, want, weight):
        a.setflags(write=False)
    return tuple(lens), sp, want, weight


def _run_mcep(sp, lens, order, alpha, out_dtype=torch.float32, rows=None, **kwargs):
    rows = sum(lens) if rows is None else rows
    out = _with_canary(rows, order, out_dtype)
    x = sp if isinstance(sp, torch.Tensor) else _dev(sp)
    got = ops.spectrum_mcep(x, order, alpha, offsets=_dev(_offsets(lens)), out=out, out_dtype=out_dtype, packed_rows=rows, **kwargs)
    assert got.data_ptr() == out.data_ptr()
    return _check_canary(out, rows)


def _mcep_bound(weight, k):
    return (2 * k + 8) * u * weight


@pytest.mark.parametrize('in_dtype', [np.float64, np.float32], ids=['in64', 'in32'])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('order,fft_size,alpha', SETTINGS, ids=IDS)
def test_mcep_against_the_float64_restatement(order, fft_size, alpha, kind, in_dtype):
    lens, sp, want, weight = _spectrum_case(order, fft_size, alpha, kind, in_dtype)
    k = fft_size // 2 + 1
    wide = _run_mcep(sp, lens, order, alpha, torch.float64)
    narrow = _run_mcep(sp, lens, order, alpha, torch.float32)
    again = _run_mcep(sp, lens, order, alpha, torch.float64)
    assert torch.equal(wide, again), 'a second call gave other bits'
    assert narrow.dtype == torch.float32 and torch.equal(narrow, wide.float()), 'the float32 output is not the float64 result rounded'
    middle = _mcep_bound(weight, k)
    err64 = np.abs(wide.cpu().numpy() - want)
    print('M=%d F=%d %s %s: float64 output, largest error / bound = %.4f (bound %.2e)' % (
        order, fft_size, kind, np.dtype(in_dtype).name, np.max(err64 / middle), np.max(middle)))
    assert np.all(err64 <= middle)
    bound32 = U * np.abs(want) + middle + 2.0 ** -149
    err32 = np.abs(narrow.cpu().numpy().astype(np.float64) - want)
    print('M=%d F=%d %s %s: float32 output, largest error / bound = %.4f' % (order, fft_size, kind, np.dtype(in_dtype).name,
                                                                           np.max(err32 / bound32)))
    assert np.all(err32 <= bound32)
    # the log spectrum as input: the host's logarithm, the same contraction
    log_sp = np.log(sp.astype(np.float64)).astype(in_dtype)
    want_log = ref.mcep(log_sp, order, alpha, fft_size, log_input=True)
    weight_log = np.abs(0.5 * log_sp.astype(np.float64)) @ np.abs(_table(order, fft_size, alpha)).T
    from_log = _run_mcep(log_sp, lens, order, alpha, torch.float64, log_input=True).cpu().numpy()
    assert np.all(np.abs(from_log - want_log) <= _mcep_bound(weight_log, k))


@pytest.mark.parametrize('in_dtype', [np.float64, np.float32], ids=['in64', 'in32'])
@pytest.mark.parametrize('order,fft_size,alpha', SETTINGS, ids=IDS)
def test_mcep_padded_input_gives_the_packed_bits(order, fft_size, alpha, in_dtype):
    """NaN in every padding frame: it never reaches the output, and the bits are those of the packed input."""
    lens, sp, _, _ = _spectrum_case(order, fft_size, alpha, 'white', in_dtype)
    want = _run_mcep(sp, lens, order, alpha, torch.float64)
    rows, k = sum(lens), fft_size // 2 + 1
    padded = np.full((len(lens), max(lens) + 2, k), np.nan, dtype=in_dtype)
    for b, (first, n) in enumerate(zip(_offsets(lens), lens)):
        padded[b, :n] = sp[first:first + n]
    seq_len = torch.tensor(lens, dtype=torch.int64, device=DEV)
    out = _with_canary(rows, order, torch.float64)
    ops.spectrum_mcep(_dev(padded), order, alpha, seq_len=seq_len, out=out, out_dtype=torch.float64, packed_rows=rows)
    assert torch.equal(_check_canary(out, rows), want)
    # lengths beyond T_in are clamped; the default packed_rows is B * T and the rows behind the last item are not written
    big = _with_canary(padded.shape[0] * padded.shape[1], order, torch.float64, extra=0)
    ops.spectrum_mcep(_dev(padded), order, alpha, seq_len=seq_len, out=big, out_dtype=torch.float64)
    assert torch.equal(big[:rows], want) and torch.all(big[rows:] == CANARY)
    assert bool(torch.isfinite(want).all())


@pytest.mark.parametrize('poison', [np.nan, 0.0, -1.0], ids=['nan', 'zero', 'negative'])
@pytest.mark.parametrize('order,fft_size,alpha', SETTINGS, ids=IDS)
def test_mcep_a_bad_frame_stays_alone(order, fft_size, alpha, poison):
    """A frame with a NaN, zero or negative bin comes out non-finite and no other frame's bits change: in the middle of an item (an
    ordinary frame directly before and after it), as the first frame of the next item, and in the rows behind packed_rows.  Bins 0
    and K - 1 are the ones an unmasked dead slot of the neighbouring row would read."""
    lens, sp, _, _ = _spectrum_case(order, fft_size, alpha, 'white', np.float64)
    rows, k = sum(lens), fft_size // 2 + 1
    first = _offsets(lens)
    clean = _run_mcep(sp, lens, order, alpha, torch.float64)
    bad_rows = [int(first[3]) + 5, int(first[4]), int(first[5]), rows - 1]      # inside an item; the first frames of the next items; the last
    for bins in ((0,), (k - 1,), (0, 1, 2, k - 1)):
        dirty = sp.copy()
        for r in bad_rows:
            dirty[r, list(bins)] = poison
        got = _run_mcep(dirty, lens, order, alpha, torch.float64)
        keep = np.ones(rows, dtype=bool)
        keep[bad_rows] = False
        assert torch.equal(got[_dev(keep)], clean[_dev(keep)]), 'a frame next to a bad one changed (bins %s)' % (bins,)
        assert not bool(torch.isfinite(got[_dev(~keep)]).any()), 'a bad frame came out finite (bins %s)' % (bins,)
    # behind packed_rows of a larger buffer: never read
    larger = np.concatenate((sp, np.full((2, k), poison)))
    got = _run_mcep(larger, lens, order, alpha, torch.float64, rows=rows)
    assert torch.equal(got, clean)


@pytest.mark.parametrize('order,fft_size,alpha', IDENTITY_SETTINGS, ids=['M%d-F%d-a%g' % s for s in IDENTITY_SETTINGS])
def test_mcep_round_trip_through_the_synthesis_kernel(order, fft_size, alpha):
    rng = np.random.RandomState(order + fft_size)
    lens = _lengths()
    c = _cepstra(rng, sum(lens), order).astype(np.float32)
    offsets = _dev(_offsets(lens))
    log_sp = ops.mcep_spectrum(_dev(c), alpha, fft_size, offsets=offsets, log=True)
    back = ops.spectrum_mcep(log_sp, order, alpha, fft_size, offsets=offsets, log_input=True, out_dtype=torch.float64).cpu().numpy()
    scale = np.abs(c.astype(np.float64)).sum(axis=1, keepdims=True)
    row_sum = np.abs(_table(order, fft_size, alpha)).sum(axis=1).max()
    bound = row_sum * (order + 2) * U * scale + 1e-13 * scale
    err = np.abs(back - c.astype(np.float64))
    print('M=%d F=%d: round trip, largest error / bound = %.4f (row sum %.3f)' % (order, fft_size, np.max(err / bound), row_sum))
    assert np.all(err <= bound)


# ------------------------------------------------------------------------------------------------------------------ the aperiodicity
BAP_SETTINGS = ((16000, 1024, 1), (48000, 2048, 5), (44100, 2048, 5))
BAP_IDS = ['%d-F%d-%d' % s for s in BAP_SETTINGS]


@functools.lru_cache(maxsize=None)
def _aperiodicity_case(sample_rate, fft_size, bands, in_dtype):
    rng = np.random.RandomState(sample_rate // 100 + bands)
    lens = _lengths()
    rows, k = sum(lens), fft_size // 2 + 1
    ap = (10.0 ** (rng.uniform(-65.0, 3.0, size=(rows, k)) / 20.0)).astype(in_dtype)
    special = np.array([0.0, 1.0, 1e-4, 1.5, np.nan, 1e-3], dtype=in_dtype)
    for b in range(bands):                                    # the special values on the bins the bands read, frame after frame
        k0 = 3000 * (b + 1) * fft_size // sample_rate
        for j, value in enumerate(special):
            ap[(2 * j + b) % rows::2 * len(special), k0] = value
            ap[(2 * j + 1 + b) % rows::2 * len(special), k0 + 1] = value
    want = ref.band_aperiodicity(ap, sample_rate, bands, fft_size)
    assert np.isnan(want).any() and (want == -60.0).any() and (want == 0.0).any() and np.isfinite(want).sum() > want.size // 2
    for a in (ap, want):
        a.setflags(write=False)
    return tuple(lens), ap, want


def _run_bap(ap, lens, sample_rate, bands, out_dtype=torch.float32, **kwargs):
    rows = sum(lens)
    out = _with_canary(rows, bands, out_dtype)
    ops.aperiodicity_bap(_dev(ap), sample_rate, bands, offsets=_dev(_offsets(lens)), out=out, out_dtype=out_dtype, packed_rows=rows, **kwargs)
    return _check_canary(out, rows)


@pytest.mark.parametrize('in_dtype', [np.float64, np.float32], ids=['in64', 'in32'])
@pytest.mark.parametrize('sample_rate,fft_size,bands', BAP_SETTINGS, ids=BAP_IDS)
def test_aperiodicity_against_the_float64_restatement(sample_rate, fft_size, bands, in_dtype):
    lens, ap, want = _aperiodicity_case(sample_rate, fft_size, bands, in_dtype)
    wide = _run_bap(ap, lens, sample_rate, bands, torch.float64)
    narrow = _run_bap(ap, lens, sample_rate, bands)
    assert torch.equal(narrow.double().nan_to_num(nan=1.0), wide.float().double().nan_to_num(nan=1.0))
    assert torch.equal(wide.nan_to_num(nan=1.0), _run_bap(ap, lens, sample_rate, bands, torch.float64).nan_to_num(nan=1.0))
    nan = np.isnan(want)
    for got, bound, name in ((wide.cpu().numpy(), 1024 * u, 'float64'), (narrow.cpu().numpy().astype(np.float64), U * np.abs(want) + 1024 * u,
                                                                         'float32')):
        assert np.array_equal(np.isnan(got), nan), 'a NaN moved'
        err = np.where(nan, 0.0, np.abs(got - want))
        print('%d Hz F=%d %d bands %s: %s output, largest error / bound = %.4f' % (
            sample_rate, fft_size, bands, np.dtype(in_dtype).name, name, np.max(err / np.where(nan, 1.0, bound + 0 * want))))
        assert np.all(err <= np.where(nan, 1.0, bound + 0 * want))
    # the default band count and the FFT size read off the input
    if bands == ops.default_n_bands(sample_rate):
        auto = ops.aperiodicity_bap(_dev(ap), sample_rate, offsets=_dev(_offsets(lens)))
        assert torch.equal(auto.nan_to_num(nan=1.0), narrow.nan_to_num(nan=1.0))


@pytest.mark.parametrize('sample_rate,fft_size,bands', BAP_SETTINGS, ids=BAP_IDS)
def test_aperiodicity_padded_input_gives_the_packed_bits(sample_rate, fft_size, bands):
    lens, ap, _ = _aperiodicity_case(sample_rate, fft_size, bands, np.float32)
    want = _run_bap(ap, lens, sample_rate, bands)
    rows, k = sum(lens), fft_size // 2 + 1
    padded = np.full((len(lens), max(lens) + 2, k), 0.5, dtype=np.float32)
    for b, (first, n) in enumerate(zip(_offsets(lens), lens)):
        padded[b, :n] = ap[first:first + n]
    out = _with_canary(rows, bands)
    ops.aperiodicity_bap(_dev(padded), sample_rate, bands, seq_len=torch.tensor(lens, dtype=torch.int64, device=DEV), out=out, packed_rows=rows)
    assert torch.equal(_check_canary(out, rows).nan_to_num(nan=1.0), want.nan_to_num(nan=1.0))
    assert torch.equal(torch.isnan(out[:rows]), torch.isnan(want))


def test_aperiodicity_inverts_the_decoder_on_anchor_bins():
    """48 kHz / 2048: every anchor is a bin, so coding what K32 decoded returns the (clamped) coded value to K32's own bound: its
    aperiodicity is within 64 U relative (tests/test_gpu_vocoder.py), 20 log10(1 + 64 U) = 8.69 * 64 U dB."""
    rng = np.random.RandomState(5)
    lens = _lengths()
    bap = rng.uniform(-58.0, -0.5, size=(sum(lens), 5)).astype(np.float32)
    offsets = _dev(_offsets(lens))
    ap = ops.bap_aperiodicity(_dev(bap), 48000, 2048, offsets=offsets)
    back = ops.aperiodicity_bap(ap, 48000, 5, offsets=offsets, out_dtype=torch.float64).cpu().numpy()
    assert np.all(np.abs(back - bap) <= 20.0 / np.log(10.0) * 64 * U * 1.001 + 1024 * u)


# ------------------------------------------------------------------------------------------------------------- the chain and the tool
def test_world_parameters_invert_world_features():
    """48 kHz, the defaults (alpha 0.77, FFT 2048, 5 bands): what world_features made of (lf0, vuv, mcep, bap) codes back.
    mcep: K32's spectrum is within d = 2 (M + 2) U sum |c| + 8 U relative (its asserted bound), so l = 0.5 log(sp) is off by at most
    0.5 d (1 + d) and c by the table's largest row sum times that, plus this kernel's own float32 store.  bap: as above.  vuv: f0 is 0
    exactly where vuv <= 0.5 and a positive number elsewhere, so vuv comes back exactly."""
    rng = np.random.RandomState(11)
    order, t, seq_len = 60, 12, np.array([12, 7, 1])
    mcep = _cepstra(rng, 3 * t, order).astype(np.float32).reshape(3, t, order)
    bap = rng.uniform(-40.0, -1.0, size=(3, t, 5)).astype(np.float32)
    lf0 = rng.uniform(4.5, 5.5, size=(3, t, 1)).astype(np.float32)
    vuv = (rng.rand(3, t, 1) > 0.4).astype(np.float32)
    features = viz.synthesis.world_features(lf0, vuv, mcep, bap, 48000, seq_len)
    coded = data.world_parameters(*zip(*features), 48000, n_mcep=order)
    row_sum = np.abs(_table(order, 2048, 0.77)).sum(axis=1).max()
    assert len(coded) == 3
    for b, (got_lf0, got_vuv, got_mcep, got_bap) in enumerate(coded):
        n = seq_len[b]
        assert got_lf0.shape == (n, 1) and got_vuv.shape == (n, 1) and got_mcep.shape == (n, order) and got_bap.shape == (n, 5)
        assert all(a.dtype == np.float32 for a in (got_lf0, got_vuv, got_mcep, got_bap))
        assert np.array_equal(got_vuv, vuv[b, :n])
        assert np.all(np.isfinite(got_lf0))
        c = mcep[b, :n].astype(np.float64)
        d = 2 * (order + 2) * U * np.abs(c).sum(axis=1, keepdims=True) + 8 * U
        bound = row_sum * 0.5 * d * (1 + d) + U * np.abs(c) + 1e-12
        print('item %d: mcep chain, largest error / bound = %.4f' % (b, np.max(np.abs(got_mcep - c) / bound)))
        assert np.all(np.abs(got_mcep - c) <= bound)
        assert np.all(np.abs(got_bap - bap[b, :n].astype(np.float64)) <= 20.0 / np.log(10.0) * 64 * U * 1.001 + 60 * U + 1024 * u)
    one = data.world_parameters(*features[1], 48000, n_mcep=order)
    assert all(np.array_equal(a, b) for a, b in zip(one, coded[1]))


def test_extract_world_features_writes_what_the_ops_return(tmp_path):
    rng = np.random.RandomState(3)
    tile, k = _tile(), 513
    ids, lens = ['a', 'b', 'c'], [1, 5, _tile() + 1]
    in_dir, out_dir = str(tmp_path / 'in'), str(tmp_path / 'out')
    os.makedirs(os.path.join(in_dir, 'sp'))
    os.makedirs(os.path.join(in_dir, 'ap'))
    sps = [np.exp(rng.uniform(-20.0, 5.0, size=(n, k))) for n in lens]
    aps = [rng.uniform(1e-4, 1.0, size=(n, k)).astype(np.float32) for n in lens]
    for utt, sp, ap in zip(ids, sps, aps):
        np.save(os.path.join(in_dir, 'sp', utt + '.npy'), sp)
        np.save(os.path.join(in_dir, 'ap', utt + '.npy'), ap)
    # 5 frames of float64 and float32 are 30 780 bytes: the first two utterances share a batch, the third has its own
    frames = data.extract_world_features(ids, in_dir, out_dir, 16000, n_mcep=25, device=DEV, max_batch_bytes=40000)
    assert frames == sum(lens) and tile + 1 == lens[2]
    offsets = _dev(_offsets(lens))
    mcep = ops.spectrum_mcep(_dev(np.concatenate(sps)), 25, 0.58, offsets=offsets).cpu().numpy()
    bap = ops.aperiodicity_bap(_dev(np.concatenate(aps)), 16000, offsets=offsets).cpu().numpy()
    for utt, first, n in zip(ids, _offsets(lens), lens):
        got_mcep, got_bap = np.load(os.path.join(out_dir, 'mcep', utt + '.npy')), np.load(os.path.join(out_dir, 'bap', utt + '.npy'))
        assert got_mcep.dtype == np.float32 and got_mcep.shape == (n, 25) and got_bap.dtype == np.float32 and got_bap.shape == (n, 1)
        assert np.array_equal(got_mcep, mcep[first:first + n]) and np.array_equal(got_bap, bap[first:first + n])
    with pytest.raises(FileExistsError, match="'a'"):
        data.extract_world_features(ids, in_dir, out_dir, 16000, n_mcep=25, device=DEV)
    assert data.extract_world_features(ids, in_dir, out_dir, 16000, n_mcep=25, device=DEV, overwrite=True) == sum(lens)
    np.save(os.path.join(in_dir, 'ap', 'b.npy'), aps[1][:4])
    with pytest.raises(ValueError, match="'b'"):
        data.extract_world_features(ids, in_dir, str(tmp_path / 'other'), 16000, n_mcep=25, device=DEV)
    assert not os.path.exists(str(tmp_path / 'other'))


# ---------------------------------------------------------------------------------- a packed input whose items do not start at row 0
@pytest.mark.parametrize('entry', ['spectrum_mcep', 'aperiodicity_bap'])
def test_packed_items_between_rows_of_no_item(entry):
    """Items [tile - 1, 0, 2] whose offsets start at tile + 1 - the first row tile holds no item - and end 3 rows before packed_rows:
    the rows in front of the first item and behind the last keep the canary, the rows between are the bits of the same items packed
    from row 0.  The input rows of no item are NaN: nothing of them reaches an item."""
    tile = _tile()
    offsets = _offsets([tile - 1, 0, 2]) + (tile + 1)
    lo, hi = int(offsets[0]), int(offsets[-1])
    rows = hi + 3
    x = np.full((rows, 5), np.nan)                               # fft_size 8
    x[lo:hi] = np.random.RandomState(tile).uniform(1e-3, 1.0, size=(hi - lo, 5))
    x = _dev(x)
    if entry == 'spectrum_mcep':
        cols = 2

        def run(rows_of, off, **kwargs):
            return ops.spectrum_mcep(x[rows_of], 2, 0.42, offsets=off, **kwargs)
    else:
        cols = 1

        def run(rows_of, off, **kwargs):
            return ops.aperiodicity_bap(x[rows_of], 16000, 1, offsets=off, **kwargs)

    out = _with_canary(rows, cols)
    run(slice(None), _dev(offsets), out=out, packed_rows=rows)
    want = run(slice(lo, hi), _dev(offsets - lo))
    assert want.shape == (hi - lo, cols) and bool(torch.isfinite(want).all())
    assert torch.all(out[:lo] == CANARY), 'rows in front of the first item were written'
    assert torch.all(out[hi:] == CANARY), 'rows behind the last item were written'
    assert torch.equal(out[lo:hi], want), 'the items moved to row 0 give other bits'
