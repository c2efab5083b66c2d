"""K31 on the device: mg_quantise_durations_f32 / ops.quantise_durations / data.quantise_durations, models.DurationModel and
models.with_predicted_durations.  The quantiser is held bit for bit to tests/durations_ref.py (python floats up to the fixed-point
value, python integers and the SEQUENTIAL emit rule from there) on dur, phone_dur, n_frames and flags; tests/test_durations_host.py
asserts that no input built here has a segment the reference alone cannot decide."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import durations_ref as ref
from morgana_amd import _lib, data, models, ops, optim

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = -77777777
N_PHONES = 7
LO, HI = 1, 60
ROUNDINGS = ('carry', 'nearest')


def _device(a):
    return torch.from_numpy(np.array(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def case(n_states, log_input):
    """(pred (4, 7, S) float32 in the normalised space, mean (S,), std_dev (S,), n_phones, total):
      item 0: ordinary gamma-distributed durations,
      item 1: n_phones = 0, between two others: its rows are NaN and must not be read,
      item 2: a NaN, a -3.0, a +inf and a value above HI,
      item 3: n_phones = 5, with non-zero predictions in the dropped phones.
    With ``log_input`` the de-normalised value is the logarithm of the duration."""
    rng = np.random.RandomState(310 + 2 * n_states + log_input)
    frames = rng.gamma(2.0, 4.0 if n_states == 1 else 1.5, size=(4, N_PHONES, n_states)) + 0.05
    if log_input:
        mean = (1.2 + 0.1 * rng.rand(n_states)).astype(np.float32)
        std_dev = (0.7 + 0.1 * rng.rand(n_states)).astype(np.float32)
        value = np.log(frames)
    else:
        mean = (6.0 + rng.rand(n_states)).astype(np.float32)
        std_dev = (4.0 + rng.rand(n_states)).astype(np.float32)
        value = frames
    pred = ((value - mean.astype(np.float64)) / std_dev.astype(np.float64)).astype(np.float32)
    pred[1] = np.nan
    last = n_states - 1
    above = math.log(3.0 * HI) if log_input else 3.0 * HI
    pred[2, 0, 0], pred[2, 1, last], pred[2, 3, 0] = np.nan, -3.0, np.inf
    pred[2, 5, last] = np.float32((above - float(mean[last])) / float(std_dev[last]))
    n_phones = np.array([N_PHONES, 0, N_PHONES, 5], dtype=np.int64)
    natural = ref.batch(pred, n_phones, mean, std_dev, log_input=bool(log_input), lo=LO, hi=HI)[2]
    total = np.array([natural[0] + 7, 30, natural[2] - 3, natural[3] + 11], dtype=np.int64)
    assert np.all(pred[3, 5:] != 0) and natural[1] == 0 and natural.min(initial=10 ** 9, where=n_phones > 0) > 12
    for a in (pred, mean, std_dev, n_phones, total):
        a.setflags(write=False)
    return pred, mean, std_dev, n_phones, total


@functools.lru_cache(maxsize=None)
def long_case():
    """(pred (2, 300, 5) float32 in frames, n_phones, total): n = 1500 segments, more than a workgroup's pass.  Item 0: one segment of
    40 frames followed by 1100 zeros - with lo = 1 the running maximum and the sum are carried across every chunk boundary.  Item 1:
    257 phones, n = 1285, no multiple of the chunk."""
    rng = np.random.RandomState(77)
    pred = (rng.gamma(2.0, 1.5, size=(2, 300, 5)) + 0.05).astype(np.float32)
    flat = pred[0].reshape(-1)
    flat[100] = 40.0
    flat[101:1201] = 0.0
    n_phones = np.array([300, 257], dtype=np.int64)
    natural = ref.batch(pred, n_phones, lo=1, hi=ref.MAX_FRAMES)[2]
    total = np.array([natural[0] + 400, natural[1] - 250], dtype=np.int64)
    for a in (pred, n_phones, total):
        a.setflags(write=False)
    return pred, n_phones, total


def model_case(n_phones_max, n_states=1):
    """A batch of 4 for DurationModel: normalised_lab (4, P, 600), natural dur (4, P, S), its mvn twin, n_phones, n_frames."""
    rng = np.random.RandomState(500 + n_phones_max + n_states)
    n_phones = {1: (1, 1, 1, 1), 7: (7, 3, 5, 1), 40: (40, 17, 33, 2)}[n_phones_max]
    lab = rng.rand(4, n_phones_max, 600).astype(np.float32)
    dur = rng.randint(1, 21, size=(4, n_phones_max, n_states)).astype(np.int64)
    for b, n in enumerate(n_phones):
        lab[b, n:], dur[b, n:] = 0., 0
    mean, std_dev = np.full(n_states, 8.0, dtype=np.float32), np.full(n_states, 4.0, dtype=np.float32)
    norm = ((dur - 8.0) / 4.0).astype(np.float32)
    for b, n in enumerate(n_phones):
        norm[b, n:] = 0.
    return dict(normalised_lab=lab, dur=dur, normalised_dur=norm, n_phones=np.array(n_phones, dtype=np.int64),
                n_frames=dur.sum(axis=(1, 2))), mean, std_dev


def all_reference_inputs():
    """Every (pred, n_phones, p0, p1, log_input, lo, hi) this file hands the quantiser with log_input: the host test counts their
    undecided segments under the reference alone."""
    for n_states in (1, 5):
        pred, mean, std_dev, n_phones, _ = case(n_states, 1)
        yield pred, n_phones, mean, std_dev, True, LO, HI


# ---------------------------------------------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def _want(n_states, log_input, rounding, with_total):
    pred, mean, std_dev, n_phones, total = case(n_states, log_input)
    got = ref.batch(pred, n_phones, mean, std_dev, total=total if with_total else None, log_input=bool(log_input), lo=LO, hi=HI,
                    rounding=rounding)
    assert got[4] == 0, 'the reference cannot decide %d segments of this case on its own' % got[4]
    return got[:4]


def _equal(got, want):
    for g, w, name in zip(got, want, ('dur', 'phone_dur', 'n_frames', 'flags')):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=name)


def _guarded(n, lead, dtype):
    whole = torch.full((lead + n + 5,), GUARD, dtype=dtype, device=DEV)
    return whole, whole.data_ptr() + whole.element_size() * lead


def _inside(whole, lead, n):
    host = whole.cpu().numpy()
    assert np.all(host[:lead] == GUARD) and np.all(host[lead + n:] == GUARD), 'the kernel wrote outside an output'
    return host[lead:lead + n]


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('with_total', [False, True], ids=['free', 'fitted'])
@pytest.mark.parametrize('log_input', [0, 1], ids=['frames', 'log'])
@pytest.mark.parametrize('rounding', ROUNDINGS)
@pytest.mark.parametrize('n_states', [1, 5])
def test_kernel_equals_the_reference_bit_for_bit(n_states, rounding, log_input, with_total):
    """mg_quantise_durations_f32 through the C ABI into guarded outputs that start 3 elements into their allocations: dur, phone_dur,
    n_frames and flags are the reference's; the NaN rows of the item without phones are never read (a read would set flag bit 0)."""
    lib = _lib.load()
    pred_np, mean, std_dev, n_phones_np, total_np = case(n_states, log_input)
    want = _want(n_states, log_input, rounding, with_total)
    pred, p0, p1, n_phones, total = (_device(a) for a in (pred_np, mean, std_dev, n_phones_np, total_np))
    lead = 3
    sizes = (4 * N_PHONES * n_states, 4 * N_PHONES, 4, 4)
    held = [_guarded(n, lead, torch.int32 if k == 3 else torch.int64) for k, n in enumerate(sizes)]
    _lib.check(lib.mg_quantise_durations_f32(pred.data_ptr(), 4, N_PHONES, n_states, pred.stride(0), pred.stride(1), pred.stride(2),
                                             n_phones.data_ptr(), p0.data_ptr(), p1.data_ptr(), None, 0, log_input, 1.0, LO, HI,
                                             ops.DUR_ROUNDINGS[rounding], total.data_ptr() if with_total else None, held[0][1], held[1][1],
                                             held[2][1], held[3][1], None), 'mg_quantise_durations_f32')
    torch.cuda.synchronize()
    got = [_inside(whole, lead, n).reshape(w.shape) for (whole, _), n, w in zip(held, sizes, want)]
    _equal(got, want)
    assert want[3][1] == (ops.DUR_FLAG_NO_FIT if with_total else 0) and want[3][2] & ops.DUR_FLAG_INVALID and not want[3][0] & 3
    assert np.all(want[0][1] == 0) and np.all(want[0][3, 5:] == 0) and want[2][1] == 0
    np.testing.assert_array_equal(pred.cpu().numpy().view(np.uint32), pred_np.view(np.uint32))


@pytest.mark.parametrize('with_total', [False, True], ids=['free', 'fitted'])
@pytest.mark.parametrize('rounding', ROUNDINGS)
def test_a_long_item_carries_the_sum_and_the_maximum_over_chunks(rounding, with_total):
    """n = 1500 segments of an item (six chunks of a workgroup): 40 frames then 1100 empty segments under lo = 1 keep the running maximum
    of the carry rule above the rounded sum over four chunk boundaries."""
    pred_np, n_phones_np, total_np = long_case()
    want = ref.batch(pred_np, n_phones_np, total=total_np if with_total else None, lo=1, hi=ref.MAX_FRAMES, rounding=rounding)[:4]
    got = ops.quantise_durations(_device(pred_np), n_phones=_device(n_phones_np), lo=1, rounding=rounding,
                                 total=_device(total_np) if with_total else None)
    _equal(got, want)
    if rounding == 'carry':
        assert np.all(want[0][0].reshape(-1)[101:1201] == 1) and want[0][0].reshape(-1)[100] >= 40
        if not with_total:
            assert want[3][0] & ops.DUR_FLAG_PUSHED
        else:
            assert want[2][1] == total_np[1] and not want[3][1]


@pytest.mark.parametrize('n_states', [1, 5])
def test_strided_predictions_are_read_in_place(n_states):
    """``pred`` as a column slice [:, :, 3:3+S] of a wider tensor and as a transposed view: the bits of the contiguous copy."""
    pred_np, mean, std_dev, n_phones_np, total_np = case(n_states, 0)
    want = _want(n_states, 0, 'carry', True)
    args = dict(n_phones=_device(n_phones_np), p0=_device(mean), p1=_device(std_dev), lo=LO, hi=HI, total=_device(total_np))
    wide = torch.full((4, N_PHONES, n_states + 6), float('nan'), device=DEV)
    wide[:, :, 3:3 + n_states] = _device(pred_np)
    sliced = wide[:, :, 3:3 + n_states]
    turned = _device(pred_np).transpose(1, 2).contiguous().transpose(1, 2)
    assert not turned.is_contiguous() or n_states == 1
    assert sliced.data_ptr() != wide.data_ptr() and sliced.stride(1) == n_states + 6
    for view in (sliced, turned):
        _equal(ops.quantise_durations(view, **args), want)


def test_normaliser_operands_plain_and_per_speaker():
    """Plain vectors against tables with item_row: every item under its own row is the reference under that row; an index outside the
    table gives zeros and DUR_FLAG_NO_ROW alone."""
    pred_np, mean, std_dev, n_phones_np, total_np = case(5, 0)
    tables0 = np.stack([mean, mean + np.float32(1.5), mean - np.float32(0.75)])
    tables1 = np.stack([std_dev, std_dev * np.float32(0.5), std_dev + np.float32(1.25)])
    item_row = np.array([2, 0, 7, 1], dtype=np.int32)
    for rounding, with_total in itertools.product(ROUNDINGS, (False, True)):
        want = ref.batch(pred_np, n_phones_np, tables0, tables1, item_row=item_row, total=total_np if with_total else None, lo=LO, hi=HI,
                         rounding=rounding)[:4]
        got = ops.quantise_durations(_device(pred_np), n_phones=_device(n_phones_np), p0=_device(tables0), p1=_device(tables1),
                                     item_row=_device(item_row), lo=LO, hi=HI, rounding=rounding,
                                     total=_device(total_np) if with_total else None)
        _equal(got, want)
        assert want[3][2] == ops.DUR_FLAG_NO_ROW and np.all(want[0][2] == 0) and want[2][0] > 0
    normaliser = data.SpeakerDependentMeanVarianceNormaliser('dur', None).set_params(
        {name: {'mean': tables0[k], 'std_dev': tables1[k]} for k, name in enumerate(('anna', 'bert', 'cleo'))})
    good = np.array([2, 0, 1, 1], dtype=np.int32)
    want = ref.batch(pred_np, n_phones_np, tables0, tables1, item_row=good, lo=LO, hi=HI)[:4]
    _equal(data.quantise_durations(_device(pred_np), n_phones=_device(n_phones_np), normaliser=normaliser, speaker_index=_device(good),
                                   min_frames=LO, max_frames=HI), want)


@pytest.mark.parametrize('log_input', [0, 1], ids=['frames', 'log'])
@pytest.mark.parametrize('n_states', [1, 5])
def test_device_form_equals_host_form(n_states, log_input):
    """data.quantise_durations on a device batch against its NumPy form on every item's valid phones, scale included."""
    pred_np, mean, std_dev, n_phones_np, total_np = case(n_states, log_input)
    normaliser = data.MeanVarianceNormaliser('dur').set_params({'mean': mean, 'std_dev': std_dev})
    for rounding, with_total in itertools.product(ROUNDINGS, (False, True)):
        kwargs = dict(normaliser=normaliser, log_input=bool(log_input), min_frames=LO, max_frames=HI, rounding=rounding)
        dur, phone_dur, n_frames, flags = data.quantise_durations(_device(pred_np), n_phones=_device(n_phones_np),
                                                                  total=_device(total_np) if with_total else None, **kwargs)
        want = _want(n_states, log_input, rounding, with_total)
        _equal((dur, phone_dur, n_frames, flags), want)
        for b in (0, 2, 3):
            n = int(n_phones_np[b])
            host = data.quantise_durations(pred_np[b, :n], total=int(total_np[b]) if with_total else None, **kwargs)
            np.testing.assert_array_equal(host[0], want[0][b, :n])
            np.testing.assert_array_equal(host[1], want[1][b, :n])
            assert (host[2], host[3]) == (want[2][b], want[3][b])
    flat = data.quantise_durations(_device(pred_np[:, :, 0].copy()), n_phones=_device(n_phones_np), min_frames=LO, max_frames=HI)
    assert tuple(flat[0].shape) == (4, N_PHONES)
    _equal(flat, ref.batch(pred_np[:, :, 0], n_phones_np, lo=LO, hi=HI)[:4])


def test_capture_and_replay_of_the_bare_launch():
    """One capture of ops.quantise_durations, replayed, then replayed on a prediction and totals changed in place: the eager bits."""
    first, mean, std_dev, n_phones_np, total_np = case(5, 0)
    second = np.array(first[::-1])
    second_total = np.array(total_np[::-1])
    pred, total, n_phones = _device(first), _device(total_np), _device(np.array([N_PHONES, N_PHONES, 5, 0], dtype=np.int64))
    args = dict(n_phones=n_phones, p0=_device(mean), p1=_device(std_dev), lo=LO, hi=HI)
    eager_first = ops.quantise_durations(pred, total=total, **args)
    eager_second = ops.quantise_durations(_device(second), total=_device(second_total), **args)
    assert not torch.equal(eager_first[0], eager_second[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.quantise_durations(pred, total=total, **args)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, eager_first):
        assert torch.equal(got, want)
    pred.copy_(_device(second))
    total.copy_(_device(second_total))
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, eager_second):
        assert torch.equal(got, want)


def test_wrapper_refusals_on_the_device():
    pred = torch.zeros((2, 3, 2), device=DEV)
    with pytest.raises(ValueError):
        ops.quantise_durations(pred, rounding='floor')
    with pytest.raises(ValueError):
        ops.quantise_durations(pred, lo=5, hi=4)
    with pytest.raises(ValueError):
        ops.quantise_durations(pred, hi=ops.DUR_MAX_FRAMES + 1)
    with pytest.raises(ValueError):
        ops.quantise_durations(pred, scale=0.)
    with pytest.raises(ValueError):
        ops.quantise_durations(pred, p0=torch.zeros(2, device=DEV))
    with pytest.raises(ValueError):
        ops.quantise_durations(pred, p0=torch.zeros(3, device=DEV), p1=torch.ones(3, device=DEV))
    with pytest.raises(ValueError):
        ops.quantise_durations(pred, item_row=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.quantise_durations(pred, total=torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(TypeError):
        ops.quantise_durations(pred.double())
    with pytest.raises(_lib.MorganaHipError):
        ops.quantise_durations(pred.cpu())
    with pytest.raises(RuntimeError):
        data.quantise_durations(pred.clone().requires_grad_(True))
    lib = _lib.load()
    out = torch.zeros(64, dtype=torch.int64, device=DEV)
    bad = lib.mg_quantise_durations_f32(pred.data_ptr(), 70000, 3, 2, 6, 2, 1, None, None, None, None, 0, 0, 1.0, 1, 4, 0, None, out.data_ptr(),
                                        out.data_ptr(), out.data_ptr(), out.data_ptr(), None)
    assert bad == _lib.MG_EINVAL and '70000' in _lib.last_error()
    bad = lib.mg_quantise_durations_f32(pred.data_ptr(), 1, 1 << 12, 1 << 12, 6, 2, 1, None, None, None, None, 0, 0, 1.0, 1, 4, 0, None,
                                        out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), None)
    assert bad == _lib.MG_EINVAL
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- the model
_STACK = {'first': 0, 'grus': (3, 5, 7), 'middle': 9, 'last': 12}


def _float64_restatement(model, feats):
    """The stack and the masked MSE of DurationModel in float64 torch on the host -> (loss, prediction, {parameter name: gradient})."""
    state = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    leaves = {k: state[k].clone().requires_grad_(True) for k in ('layers.0.weight', 'layers.0.bias', 'layers.12.weight', 'layers.12.bias')}
    x = torch.from_numpy(feats['normalised_lab']).double()
    h = torch.sigmoid(x @ leaves['layers.0.weight'].t() + leaves['layers.0.bias'])
    for k in _STACK['grus']:
        gru = nn.GRU(h.shape[-1], 64, batch_first=True).double()
        with torch.no_grad():
            for name in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0'):
                getattr(gru, name).copy_(state['layers.%d.layer.%s' % (k, name)])
        h, _ = gru(h)                                      # causal: the valid phones do not see the padded ones behind them
    h = torch.sigmoid(h @ state['layers.9.weight'].t() + state['layers.9.bias'])
    pred = h @ leaves['layers.12.weight'].t() + leaves['layers.12.bias']
    target = torch.from_numpy(feats['normalised_dur']).double()
    lens = torch.from_numpy(feats['n_phones'])
    mask = (torch.arange(pred.shape[1])[None, :] < lens[:, None])[..., None].double()
    loss = (((pred - target) ** 2 * mask).sum(dim=1) / lens[:, None].double()).mean()
    loss.backward()
    return float(loss.detach()), (pred * mask).detach().numpy(), {k: v.grad.numpy() for k, v in leaves.items()}


def _rel_err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def _model(feats_np, mean, std_dev, n_states=1):
    torch.manual_seed(11)
    model = models.DurationModel(n_states=n_states, precision='fp32').to(DEV)
    model.normalisers = model.normaliser_sources()
    model.normalisers['dur'].set_params({'mean': mean, 'std_dev': std_dev})
    return model, data.to_device(feats_np, DEV)


@pytest.mark.parametrize('n_phones_max', [1, 7, 40])
def test_duration_model_against_float64_and_training(n_phones_max):
    """predict / loss of DurationModel (B = 4, fp32) against the float64 restatement at the bars tests/test_gpu_configs.py holds the
    GRU F0 model to in fp32 (loss 1e-4, prediction 1e-4, gradients 1e-3 of the largest element), the gradients of the first and the
    last Linear likewise; three eager Adam steps lower the loss; eval() after fit_to('n_frames') returns the target length wherever
    the minimum did not push it out."""
    feats_np, mean, std_dev = model_case(n_phones_max)
    model, feats = _model(feats_np, mean, std_dev)
    model.train()
    want_loss, want_pred, want_grads = _float64_restatement(model, feats_np)
    loss, out = model(feats)
    loss.backward()
    ops.check_persistent_status()
    valid = (np.arange(n_phones_max)[None, :] < feats_np['n_phones'][:, None])[..., None]
    np.testing.assert_allclose(loss.item(), want_loss, rtol=1e-4)
    assert _rel_err(np.where(valid, out['normalised_dur'].detach().cpu().numpy(), 0), want_pred) < 1e-4
    grads = dict(model.named_parameters())
    for name, want in want_grads.items():
        assert _rel_err(grads[name].grad.cpu().numpy(), want) < 1e-3, name
    assert out['normalised_dur'].requires_grad and not out['dur'].requires_grad and out['dur'].dtype == torch.int64
    assert tuple(out['dur'].shape) == (4, n_phones_max, 1) and tuple(out['phone_dur'].shape) == (4, n_phones_max)
    want = ref.batch(out['normalised_dur'].detach().cpu().numpy(), feats_np['n_phones'], mean, std_dev)[:4]
    _equal((out['dur'], out['phone_dur'], out['n_frames'], out['dur_flags']), want)
    # train() mode never fits, even after fit_to
    model.fit_to('n_frames')
    _equal(tuple(model.predict(feats)[k] for k in ('dur', 'phone_dur', 'n_frames', 'dur_flags')), want)
    # three Adam steps
    opt = optim.Adam(model.parameters(), lr=3e-3)
    first = None
    for _ in range(3):
        opt.zero_grad()
        loss, _ = model(feats)
        first = loss.item() if first is None else first
        loss.backward()
        opt.step()
    assert model(feats)[0].item() < first
    # eval(): fitted to the natural length
    model.eval()
    with torch.no_grad():
        out = model.predict(feats)
    flags, n_frames = out['dur_flags'].cpu().numpy(), out['n_frames'].cpu().numpy()
    fitted = (flags & ops.DUR_FLAG_PUSHED) == 0
    assert fitted.any() or n_phones_max == 1
    np.testing.assert_array_equal(n_frames[fitted], feats_np['n_frames'][fitted])
    np.testing.assert_array_equal(out['phone_dur'].sum(dim=1).cpu().numpy(), n_frames)
    with torch.no_grad():
        free = model.fit_to(None).predict(feats)
    assert model._fit_key is None and torch.equal(free['phone_dur'].sum(dim=1), free['n_frames'])
    assert not (free['dur_flags'].cpu().numpy() & ops.DUR_FLAG_NO_FIT).any()
    ops.check_persistent_status()


@pytest.mark.parametrize('n_states', [1, 5])
def test_predicted_durations_feed_the_acoustic_model(n_states):
    """DurationModel -> with_predicted_durations -> GRUF0Model.eval().predict: n_frames.max() frames, bit-equal to the same model on a
    batch collate_to_device builds (counter_specs=) from those same integer durations."""
    rng = np.random.RandomState(90 + n_states)
    lens = (9, 4, 6, 2)
    utterances = []
    for b, n in enumerate(lens):
        dur = rng.randint(1, 9, size=(n, n_states)).astype(np.int64)
        utterances.append({'name': 'utt%d' % b, 'lab': (rng.rand(n, 600) * 3).astype(np.float32), 'dur': dur, 'n_phones': n,
                           'n_frames': int(dur.sum())})
    lab_norm = data.MinMaxNormaliser('lab').set_params({'mmin': np.zeros(600, np.float32), 'mmax': np.full(600, 3, np.float32)})
    counters_norm = data.MinMaxNormaliser('counters').set_params({'mmin': np.zeros(9, np.float32),
                                                                  'mmax': np.array([1, 1, 30, 5, 5, 60, 1, 1, 1], np.float32)})
    dur_norm = data.MeanVarianceNormaliser('dur').set_params({'mean': np.full(n_states, 4.5, np.float32),
                                                              'std_dev': np.full(n_states, 2.5, np.float32)})
    natural = data.collate_to_device(utterances, {'lab': lab_norm, 'dur': dur_norm}, DEV)
    assert tuple(natural['normalised_dur'].shape) == (4, 9, n_states)
    torch.manual_seed(5)
    duration_model = models.DurationModel(n_states=n_states, precision='fp32').to(DEV).eval()
    duration_model.normalisers = {'lab': lab_norm, 'dur': dur_norm}
    with torch.no_grad():
        predicted = duration_model.predict(natural)
    kept = dict(natural)
    feats = models.with_predicted_durations(natural, predicted, {'lab': lab_norm, 'counters': counters_norm})
    assert natural.keys() == kept.keys() and all(natural[k] is kept[k] for k in kept)
    assert 'normalised_dur' not in feats and feats['normalised_lab'] is natural['normalised_lab'] and feats['name'] == natural['name']
    assert tuple(feats['dur'].shape) == (4, 9, 1) and ('state_dur' in feats) == (n_states > 1)
    t = int(predicted['n_frames'].max())
    assert tuple(feats['normalised_counters'].shape) == (4, t, 9) and torch.equal(feats['n_frames'], predicted['n_frames'])
    # the same integer durations through the loader
    dur_host, phone_host = predicted['dur'].cpu().numpy(), predicted['phone_dur'].cpu().numpy()
    again = []
    for b, n in enumerate(lens):
        item = {'name': 'utt%d' % b, 'lab': utterances[b]['lab'], 'dur': phone_host[b, :n, None].copy(), 'n_phones': n,
                'n_frames': int(phone_host[b, :n].sum())}
        if n_states > 1:
            item['state_dur'] = dur_host[b, :n].copy()
        again.append(item)
    spec = data.CountersSpec('state_dur' if n_states > 1 else 'dur')
    loaded = data.collate_to_device(again, {'lab': lab_norm, 'counters': counters_norm}, DEV, counter_specs={'counters': spec})
    assert torch.equal(loaded['normalised_counters'], feats['normalised_counters']) and torch.equal(loaded['counters'], feats['counters'])
    assert torch.equal(loaded['dur'], feats['dur'])
    torch.manual_seed(6)
    acoustic = models.GRUF0Model(precision='fp32').to(DEV).eval()
    with torch.no_grad():
        got = acoustic.predict(feats)['normalised_lf0_deltas']
        want = acoustic.predict(loaded)['normalised_lf0_deltas']
    ops.check_persistent_status()
    assert tuple(got.shape) == (4, t, 3)
    assert torch.equal(got, want)
