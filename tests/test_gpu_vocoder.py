"""K32 on the device: mg_mcep_spectrum_f32, mg_bap_aperiodicity_f32 and mg_smooth_f0_f32 through ops / viz.synthesis / the model hook,
against tests/vocoder_ref64.py.  Every bound is derived from the number formats and the kernel's operation count (u = 2^-24, the unit
roundoff of float32), never from what the kernel returns:

spectrum   L^ is M fmaf in a chain from 0 (one rounding each; the first is the rounding of a product) over a table whose entries carry
           one rounding of a value of magnitude <= 1:  |L^ - L| <= (M + 1) u sum_m |c_m| to first order - inside the issue's
           (M + 2) u sum |c_m|, which is what is asserted.  2 L^ is exact; expf is within 1 ulp = 2 u and the error of its argument
           enters relatively:  |sp^ - sp| / sp <= 2 (M + 2) u sum |c_m| + 8 u.
aperiod.   w carries one rounding (u), b - a one (|b - a| <= 60), the fmaf one of a result of magnitude <= 60:
           |dB^ - dB| <= 60 (2 u) + 60 u = 180 u.  The factor ln10 / 20 = 0.1151 carries one rounding and the product one, on an
           argument of magnitude <= 6.91:  |arg^ - arg| <= 180 u * 0.1151 + 6.91 * 2 u < 35 u; expf adds 2 u:  < 37 u relative, inside
           the issue's estimate of 64 u, which is what is asserted.
f0         float64 throughout (exp within an ulp of float64, sums of at most 65 positive terms), rounded to float32 once: within one
           float32 ulp of the reference; 2 ulps are asserted, as the issue sets."""
import functools
import os
import wave

import numpy as np
import pytest
import torch

import vocoder_ref64 as ref
from morgana_amd import _lib, data, models, ops, synthetic, viz

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = 2.0 ** -24
CANARY = 7.5e33
SETTINGS = ((1, 8, 0.0), (2, 8, 0.42), (25, 512, 0.42), (60, 2048, 0.77), (61, 1024, 0.58), (128, 64, 0.3))
IDS = ['M%d-F%d-a%g' % s for s in SETTINGS]


def _tile():
    return _lib.load().mg_vocoder_tile_frames()


def _lengths():
    tile = _tile()
    return [0, 1, 3, tile - 1, tile, tile + 1]


def _offsets(lens):
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


def _padded(items, width, fill=np.nan):
    """(B, longest + 2, width) float32 with `fill` in every frame past an item's length."""
    t = max(len(x) for x in items) + 2
    out = np.full((len(items), t, width), fill, dtype=np.float32)
    for b, x in enumerate(items):
        out[b, :len(x)] = x
    return out


def _with_canary(rows, cols, dtype=torch.float32, extra=3):
    return torch.full((rows + extra, cols), CANARY, dtype=dtype, device=DEV)


def _check_canary(out, rows):
    assert torch.all(out[rows:] == CANARY), 'rows from packed_rows on were written'
    return out[:rows]


@functools.lru_cache(maxsize=None)
def _spectrum_case(order, fft_size, alpha):
    """(items, packed cepstra float32, reference L float64, sum |c| per frame): made once, never written to."""
    rng = np.random.RandomState(1000 * order + fft_size)
    items = []
    for n in _lengths():
        c = rng.randn(n, order) / np.maximum(np.arange(order), 1)[None, :]
        c[:, 0] = rng.uniform(-4, 4, size=n)
        items.append(c.astype(np.float32))
    packed = np.concatenate(items)
    L = ref.log_spectrum(packed, alpha, fft_size)
    scale = np.abs(packed.astype(np.float64)).sum(axis=1, keepdims=True)
    for a in (packed, L, scale):
        a.setflags(write=False)
    return tuple(items), packed, L, scale


def _run_spectrum(packed, lens, alpha, fft_size, **kwargs):
    rows, k = len(packed), fft_size // 2 + 1
    dtype = kwargs.get('out_dtype', torch.float32)
    out = _with_canary(rows, k, dtype)
    got = ops.mcep_spectrum(torch.from_numpy(packed).to(DEV), alpha, fft_size, offsets=torch.from_numpy(_offsets(lens)).to(DEV), out=out,
                            packed_rows=rows, **kwargs)
    assert got.data_ptr() == out.data_ptr()
    return _check_canary(out, rows)


@pytest.mark.parametrize('order,fft_size,alpha', SETTINGS, ids=IDS)
def test_spectrum_against_the_float64_reference(order, fft_size, alpha):
    items, packed, L, scale = _spectrum_case(order, fft_size, alpha)
    lens = [len(x) for x in items]
    assert np.max(np.abs(2 * L)) < 80, 'the case would hide behind an overflow'
    sp = _run_spectrum(packed, lens, alpha, fft_size)
    log_sp = _run_spectrum(packed, lens, alpha, fft_size, log=True)
    again = _run_spectrum(packed, lens, alpha, fft_size)
    wide = _run_spectrum(packed, lens, alpha, fft_size, out_dtype=torch.float64)
    assert torch.equal(sp, again), 'a second call gave other bits'
    assert wide.dtype == torch.float64 and torch.equal(wide, sp.double()), 'the float64 output is not the float32 result widened'
    sp, log_sp = sp.cpu().numpy().astype(np.float64), log_sp.cpu().numpy().astype(np.float64)
    l_bound = (order + 2) * U * scale
    l_err = np.abs(log_sp / 2 - L)
    print('M=%d F=%d: largest |L^ - L| / bound = %.3f' % (order, fft_size, np.max(l_err / l_bound)))
    assert np.all(l_err <= l_bound)
    want = np.exp(2 * L)
    rel = np.abs(sp - want) / want
    sp_bound = 2 * (order + 2) * U * scale + 8 * U
    print('M=%d F=%d: largest relative error of sp / bound = %.3f' % (order, fft_size, np.max(rel / sp_bound)))
    assert np.all(rel <= sp_bound)
    # log=True is 2 L^ of the same accumulation: its exponential is the spectrum to expf's own ulp
    assert np.all(np.abs(np.exp(log_sp) - sp) <= 4 * U * sp)
    # the identities of the host file on the device output: bins 0 and F / 2 are plain and alternating sums of the cepstra
    c = packed.astype(np.float64)
    assert np.all(np.abs(log_sp[:, 0] / 2 - c.sum(axis=1)) <= l_bound[:, 0] * (1 + 1e-6))
    assert np.all(np.abs(log_sp[:, -1] / 2 - (c * (-1.0) ** np.arange(order)).sum(axis=1)) <= l_bound[:, 0] * (1 + 1e-6))


@pytest.mark.parametrize('order,fft_size', [(1, 8), (25, 512), (60, 2048)])
def test_spectrum_without_warping_is_the_real_fft(order, fft_size):
    items, packed, _, scale = _spectrum_case(order, fft_size, 0.42 if order == 25 else 0.77 if order == 60 else 0.0)
    log_sp = _run_spectrum(packed, [len(x) for x in items], 0.0, fft_size, log=True).cpu().numpy().astype(np.float64)
    want = np.fft.rfft(packed.astype(np.float64), fft_size, axis=1).real
    assert np.all(np.abs(log_sp / 2 - want) <= (order + 2) * U * scale * (1 + 1e-6))


@pytest.mark.parametrize('order,fft_size,alpha', [s for s in SETTINGS if s[0] >= 2], ids=[i for s, i in zip(SETTINGS, IDS) if s[0] >= 2])
def test_spectrum_first_order_closed_form(order, fft_size, alpha):
    """Only c_1 set: L = c_1 ((1 + a^2) cos w - 2 a) / (1 + a^2 - 2 a cos w)."""
    lens = _lengths()
    packed = np.zeros((sum(lens), order), dtype=np.float32)
    packed[:, 1] = np.float32(1.7)
    w = 2 * np.pi * np.arange(fft_size // 2 + 1) / fft_size
    want = np.float64(np.float32(1.7)) * ((1 + alpha ** 2) * np.cos(w) - 2 * alpha) / (1 + alpha ** 2 - 2 * alpha * np.cos(w))
    log_sp = _run_spectrum(packed, lens, alpha, fft_size, log=True).cpu().numpy().astype(np.float64)
    assert np.all(np.abs(log_sp / 2 - want[None, :]) <= (order + 2) * U * 1.7 * (1 + 1e-6))


@pytest.mark.parametrize('order,fft_size,alpha', SETTINGS, ids=IDS)
def test_spectrum_padded_input_gives_the_packed_bits(order, fft_size, alpha):
    """NaN in every padding frame: it never reaches the output, and the bits are those of the packed input."""
    items, packed, _, _ = _spectrum_case(order, fft_size, alpha)
    lens = [len(x) for x in items]
    want = _run_spectrum(packed, lens, alpha, fft_size)
    rows, k = len(packed), fft_size // 2 + 1
    padded = torch.from_numpy(_padded(items, order)).to(DEV)
    seq_len = torch.tensor(lens, dtype=torch.int64, device=DEV)
    for dtype in (torch.float32, torch.float64):
        out = _with_canary(rows, k, dtype)
        ops.mcep_spectrum(padded, alpha, fft_size, seq_len=seq_len, packed_rows=rows, out=out, out_dtype=dtype)
        got = _check_canary(out, rows)
        assert not torch.isnan(got).any()
        assert torch.equal(got, want.to(dtype))
    # lengths past T_in are clamped, negative ones count as 0; packed_rows cuts the output
    seq_len2 = seq_len.clone()
    seq_len2[0], seq_len2[1] = -5, 1
    out = _with_canary(2, k)
    ops.mcep_spectrum(padded, alpha, fft_size, seq_len=seq_len2, packed_rows=2, out=out)
    assert torch.equal(_check_canary(out, 2), want[:2])          # item 1 (one frame), then the first frame of item 2
    # the reference-style function: device tensors in, packed device tensor and offsets out
    sp, offsets = viz.synthesis.mcep_to_spectrum(padded, alpha, fft_size, seq_len=lens)
    assert sp.is_cuda and sp.dtype == torch.float32 and torch.equal(sp, want) and offsets.tolist() == _offsets(lens).tolist()
    sp, offsets = viz.synthesis.mcep_to_spectrum(padded, alpha, fft_size, seq_len=seq_len, dtype=torch.float64)
    assert sp.shape[0] == padded.shape[0] * padded.shape[1] and torch.equal(sp[:rows], want.double())
    assert offsets.is_cuda and offsets.tolist() == _offsets(lens).tolist()


def test_spectrum_propagates_non_finite_cepstra_to_their_frame_alone():
    items, packed, _, _ = _spectrum_case(25, 512, 0.42)
    lens = [len(x) for x in items]
    want = _run_spectrum(packed, lens, 0.42, 512)
    dirty = packed.copy()
    dirty[2, 24] = np.nan
    dirty[5, 0] = np.inf
    dirty[7, 10] = -np.inf                                       # -inf * basis: exp(-inf) = 0 where the basis is positive, inf where negative
    got = _run_spectrum(dirty, lens, 0.42, 512)
    assert torch.isnan(got[2]).all() and torch.all(got[5] == float('inf'))
    row10 = ops.mcep_basis_table(25, 0.42, 512)[10]
    assert (row10 > 0).any() and (row10 < 0).any() and not (row10 == 0).any()
    assert np.array_equal(got[7].cpu().numpy(), np.where(row10 > 0, np.float32(0), np.float32(np.inf)))
    keep = [r for r in range(len(packed)) if r not in (2, 5, 7)]
    assert torch.equal(got[keep], want[keep])


# ------------------------------------------------------------------------------------------------------------------------ aperiodicity
@functools.lru_cache(maxsize=None)
def _bap_case(bands):
    rng = np.random.RandomState(bands)
    items = [rng.uniform(-75, 8, size=(n, bands)).astype(np.float32) for n in _lengths()]
    items[2][0, :] = -60.0
    items[2][1, :] = 0.0
    items[2][2, 0] = -0.0
    return tuple(items)


@pytest.mark.parametrize('bands,sample_rate,fft_size', [(1, 16000, 1024), (5, 48000, 2048)], ids=['16k', '48k'])
def test_aperiodicity_against_the_float64_reference(bands, sample_rate, fft_size):
    items = _bap_case(bands)
    lens = [len(x) for x in items]
    packed = np.concatenate(items)
    assert (packed < -60).any() and (packed > 0).any(), 'the clamp is not exercised'
    rows, k = len(packed), fft_size // 2 + 1
    offsets = torch.from_numpy(_offsets(lens)).to(DEV)
    want = ref.aperiodicity(packed, sample_rate, fft_size)
    outs = {}
    for dtype in (torch.float32, torch.float64):
        out = _with_canary(rows, k, dtype)
        ops.bap_aperiodicity(torch.from_numpy(packed).to(DEV), sample_rate, fft_size, offsets=offsets, out=out, packed_rows=rows,
                             out_dtype=dtype)
        outs[dtype] = _check_canary(out, rows)
    got32 = outs[torch.float32]
    assert torch.equal(outs[torch.float64], got32.double())
    assert torch.equal(got32, ops.bap_aperiodicity(torch.from_numpy(packed).to(DEV), sample_rate, fft_size, offsets=offsets))
    got = got32.cpu().numpy().astype(np.float64)
    rel = np.abs(got - want) / want
    print('Nb=%d fs=%d: largest relative error / (64 u) = %.3f' % (bands, sample_rate, np.max(rel) / (64 * U)))
    assert np.all(rel <= 64 * U)
    clamped = np.clip(packed.astype(np.float64), -60, 0)
    assert np.all(np.abs(got[:, 0] - 1e-3) <= 64 * U * 1e-3) and np.all(np.abs(got[:, -1] - 1.0) <= 64 * U)
    per_band = int(round(3000 * fft_size / sample_rate))       # 192 at 16 kHz / 1024, 128 at 48 kHz / 2048: exact anchors
    assert per_band * sample_rate == 3000 * fft_size
    for i in range(1, bands + 1):
        anchor = 10.0 ** (clamped[:, i - 1] / 20.0)
        assert np.all(np.abs(got[:, per_band * i] - anchor) <= 64 * U * anchor)
    # a padded input with NaN in the padding gives the same bits
    seq_len = torch.tensor(lens, dtype=torch.int64, device=DEV)
    out = _with_canary(rows, k)
    ops.bap_aperiodicity(torch.from_numpy(_padded(items, bands)).to(DEV), sample_rate, fft_size, seq_len=seq_len, packed_rows=rows, out=out)
    assert torch.equal(_check_canary(out, rows), got32)
    ap, offs = viz.synthesis.bap_to_aperiodicity(_padded(items, bands), sample_rate, fft_size, seq_len=lens)      # an array is uploaded
    assert ap.is_cuda and torch.equal(ap, got32) and offs.tolist() == _offsets(lens).tolist()
    with pytest.raises(ValueError, match='bands'):
        ops.bap_aperiodicity(torch.zeros(4, 3, device=DEV), 16000, 1024, offsets=torch.tensor([0, 4], device=DEV))


# -------------------------------------------------------------------------------------------------------------------------------- f0
def _f0_lengths():
    return [0, 1, 6, 7, 8, _lib.load().mg_smooth_f0_chunk_rows() + 3, 9]


@functools.lru_cache(maxsize=None)
def _f0_case(width):
    """Adjacent items at very different levels (100 Hz, 400 Hz, ...): a window that leaks across a boundary shows at once."""
    rng = np.random.RandomState(40 + width)
    lf0, vuv = [], []
    for i, n in enumerate(_f0_lengths()):
        level = np.log(100.0) if i % 2 else np.log(400.0)
        lf0.append((level + rng.uniform(-0.2, 0.2, size=(n, width))).astype(np.float32))
        vuv.append(rng.choice(np.array([0.1, 0.5, 0.9, 1.0], dtype=np.float32), size=(n, width)))
    return tuple(lf0), tuple(vuv)


@pytest.mark.parametrize('window', [1, 3, 7])
@pytest.mark.parametrize('width', [1, 2])
def test_smoothed_f0_against_the_float64_reference(width, window):
    lf0, vuv = _f0_case(width)
    lens = [len(x) for x in lf0]
    want = np.concatenate([ref.smooth_f0(a, b, window) for a, b in zip(lf0, vuv)])
    packed_l, packed_v = np.concatenate(lf0), np.concatenate(vuv)
    rows = len(packed_l)
    offsets = torch.from_numpy(_offsets(lens)).to(DEV)
    outs = {}
    for dtype in (torch.float32, torch.float64):
        out = _with_canary(rows, width, dtype)
        ops.smooth_f0(torch.from_numpy(packed_l).to(DEV), torch.from_numpy(packed_v).to(DEV), offsets=offsets, window=window, out=out,
                      packed_rows=rows, out_dtype=dtype)
        outs[dtype] = _check_canary(out, rows)
    got32 = outs[torch.float32]
    assert torch.equal(outs[torch.float64], got32.double())
    got = got32.cpu().numpy()
    unvoiced = packed_v <= np.float32(0.5)
    assert unvoiced.any() and (~unvoiced).any()
    assert np.all(got[unvoiced] == 0.0) and np.all(want[unvoiced] == 0.0)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)
    print('D=%d window=%d: largest error = %.3f float32 ulps' % (width, window, np.max(err / ulp)))
    assert np.all(err <= 2 * ulp)
    # padded, NaN past every length in both inputs: the same bits
    seq_len = torch.tensor(lens, dtype=torch.int64, device=DEV)
    out = _with_canary(rows, width)
    ops.smooth_f0(torch.from_numpy(_padded(lf0, width)).to(DEV), torch.from_numpy(_padded(vuv, width)).to(DEV), seq_len=seq_len,
                  window=window, packed_rows=rows, out=out)
    assert torch.equal(_check_canary(out, rows), got32)
    if width == 1:
        f0, offs = viz.synthesis.smooth_f0(_padded(lf0, 1), _padded(vuv, 1), seq_len=lens, window=window)
        assert torch.equal(f0, got32) and offs.tolist() == _offsets(lens).tolist()


def test_wrappers_check_their_arguments_on_the_device():
    x = torch.zeros(4, 3, device=DEV)
    off = torch.tensor([0, 4], device=DEV)
    with pytest.raises(ValueError, match='exactly one'):
        ops.mcep_spectrum(x, 0.4, 64)
    with pytest.raises(ValueError, match='power of two'):
        ops.mcep_spectrum(x, 0.4, 48, offsets=off)
    with pytest.raises(ValueError, match='window'):
        ops.smooth_f0(x, x, offsets=off, window=4)
    with pytest.raises(ValueError, match='does not match'):
        ops.smooth_f0(x, x[:, :1], offsets=off)
    with pytest.raises(TypeError):
        ops.mcep_spectrum(x, 0.4, 64, offsets=off, out_dtype=torch.float16)
    with pytest.raises(ValueError, match='out '):
        ops.mcep_spectrum(x, 0.4, 64, offsets=off, out=torch.zeros(3, 33, device=DEV))
    assert ops.mcep_spectrum(x[:0], 0.4, 64, offsets=torch.zeros(1, dtype=torch.int64, device=DEV)).shape == (0, 33)
    assert ops.mcep_basis(3, 0.4, 64, DEV) is ops.mcep_basis(3, 0.4, 64, torch.device(DEV))      # the cache


# ------------------------------------------------------------------------------------------------------------------------ end to end
def _all_files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files)


def test_model_hook_hands_world_features_to_the_synthesiser(tmp_path):
    feats_np = synthetic.make_acoustic_batch(3, (20, 40), seed=22, with_raw=True)
    feats = data.to_device(feats_np, DEV)
    torch.manual_seed(5)
    model = models.LSTMAcousticModel(precision='fp32', num_layers=2).to(DEV)
    synthetic.acoustic_normalisers(model, device=DEV)
    with torch.no_grad():
        outputs = model.predict(feats)
    n_frames = [int(n) for n in feats_np['n_frames']]
    plain, synth = str(tmp_path / 'plain'), str(tmp_path / 'synth')
    model.analysis_for_valid_batch(feats, outputs, out_dir=plain)
    today = sorted('feats/%s/%s.npy' % (s, n) for s in ('lf0', 'vuv', 'mcep', 'bap') for n in feats_np['name'])
    assert _all_files(plain) == today, 'without a synthesiser the hook writes the feature files and nothing else'

    calls = []

    def synthesiser(f0, sp, ap, sample_rate):
        calls.append((f0, sp, ap, sample_rate))
        return np.sin(np.arange(80 * len(f0)) / 10.0) * 0.5

    rate, fft_size = 48000, 2048                                 # 5 bands of 3 kHz need fs / 2 > 15 kHz
    model.analysis_for_valid_batch(feats, outputs, out_dir=synth, sample_rate=rate, synthesiser=synthesiser)
    assert _all_files(synth) == sorted(today + ['synth/%s.wav' % n for n in feats_np['name']])
    assert len(calls) == 3
    k = fft_size // 2 + 1
    mcep = outputs['mcep'].cpu().numpy()
    for b, (f0, sp, ap, sample_rate) in enumerate(calls):
        n = n_frames[b]
        assert sample_rate == rate
        for a, shape in ((f0, (n,)), (sp, (n, k)), (ap, (n, k))):
            assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags['C_CONTIGUOUS'] and a.shape == shape
        assert np.all(f0 >= 0) and np.all(ap > 0) and np.all(ap <= 1) and np.all(sp >= 0)
        want = ref.spectrum(mcep[b, :n], 0.77, fft_size)
        scale = np.abs(mcep[b, :n].astype(np.float64)).sum(axis=1, keepdims=True)
        normal = (want > 1e-30) & (want < 1e30)                  # an untrained model's cepstra: float32 may overflow or go subnormal
        assert normal.any()
        limit = (2 * (mcep.shape[2] + 2) * U * scale + 8 * U) * want
        assert np.all(np.abs(sp - want)[normal] <= limit[normal])
        with wave.open(os.path.join(synth, 'synth', feats_np['name'][b] + '.wav'), 'rb') as f:
            assert (f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()) == (rate, 1, 2, 80 * n)
    with pytest.raises(KeyError, match='bap'):
        model.analysis_for_valid_batch(feats, {k_: v for k_, v in outputs.items() if k_ != 'bap'}, out_dir=synth, sample_rate=rate,
                                       synthesiser=synthesiser)
    with pytest.raises(ValueError, match='no default alpha'):
        model.analysis_for_valid_batch(feats, outputs, out_dir=synth, sample_rate=32000, synthesiser=synthesiser)


# ---------------------------------------------------------------------------------- a packed input whose items do not start at row 0
@pytest.mark.parametrize('entry', ['mcep_spectrum', 'bap_aperiodicity', 'smooth_f0'])
def test_packed_items_between_rows_of_no_item(entry):
    """Items [tile - 1, 0, 2] whose offsets start at tile + 1 - the first row tile holds no item - and end 3 rows before packed_rows:
    the rows in front of the first item and behind the last keep the canary, the rows between are the bits of the same items packed
    from row 0.  The input rows of no item are NaN: nothing of them reaches an item."""
    tile = _tile()
    offsets = _offsets([tile - 1, 0, 2]) + (tile + 1)
    lo, hi = int(offsets[0]), int(offsets[-1])
    rows = hi + 3
    rng = np.random.RandomState(tile)

    def packed(low, high, width):
        x = np.full((rows, width), np.nan, dtype=np.float32)
        x[lo:hi] = rng.uniform(low, high, size=(hi - lo, width))
        return torch.from_numpy(x).to(DEV)

    if entry == 'mcep_spectrum':
        mcep, cols = packed(-1.0, 1.0, 2), 5

        def run(rows_of, off, **kwargs):
            return ops.mcep_spectrum(mcep[rows_of], 0.42, 8, offsets=off, **kwargs)
    elif entry == 'bap_aperiodicity':
        bap, cols = packed(-70.0, 5.0, 1), 5

        def run(rows_of, off, **kwargs):
            return ops.bap_aperiodicity(bap[rows_of], 16000, 8, offsets=off, **kwargs)
    else:
        lf0, vuv, cols = packed(4.0, 6.0, 1), packed(0.0, 1.0, 1), 1

        def run(rows_of, off, **kwargs):
            return ops.smooth_f0(lf0[rows_of], vuv[rows_of], offsets=off, **kwargs)

    out = _with_canary(rows, cols)
    run(slice(None), torch.from_numpy(offsets).to(DEV), out=out, packed_rows=rows)
    want = run(slice(lo, hi), torch.from_numpy(offsets - lo).to(DEV))
    assert want.shape == (hi - lo, cols) and bool(torch.isfinite(want).all())
    assert torch.all(out[:lo] == CANARY), 'rows in front of the first item were written'
    assert torch.all(out[hi:] == CANARY), 'rows behind the last item were written'
    assert torch.equal(out[lo:hi], want), 'the items moved to row 0 give other bits'
