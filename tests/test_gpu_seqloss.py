"""losses.sequence_loss on the HIP path (csrc/seqmean.hip, mg_seq_mean_f32 / mg_seq_mean_bwd_f32): the reference's recorded numbers
and the float64 restatement with its derived bounds (tests/seqloss_ref64.py), both kernels and every stride pattern bit for bit, chunk
and finishing-pass edges, the mask's semantics, determinism, capture into a graph (no host read) and models.Stream(loss=callable)."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import parity_report
import seqloss_ref64
from morgana_amd import _lib, data, losses, models, ops, synthetic, utils

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = seqloss_ref64.U

identity = losses.sequence_loss(lambda predictions, targets: predictions)


def _dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_(True) if grad else t


def _lengths(seq_len):
    return None if seq_len is None else _dev(np.asarray(seq_len, dtype=np.int64))


def _run(feature_loss, seq_len):
    """The wrapper on a stored feature loss -> (loss as a 0-d device tensor, d loss / d feature loss as numpy)."""
    x = feature_loss if torch.is_tensor(feature_loss) else _dev(feature_loss)
    x = x.detach().requires_grad_(True)
    loss = identity(x, None, _lengths(seq_len))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    (grad,) = torch.autograd.grad(loss, x)
    assert grad.shape == x.shape and grad.is_contiguous()
    return loss.detach(), grad.cpu().numpy()


def _check_against_ref64(name, feature_loss, seq_len):
    """Loss and every gradient element inside the kernel-against-restatement bounds; returns (loss, grad, ref)."""
    ref = seqloss_ref64.seq_mean(feature_loss, seq_len)
    loss, grad = _run(feature_loss, seq_len)
    loss = float(loss.item())
    loss_err, grad_err = abs(loss - ref['loss']), np.abs(grad.astype(np.float64) - ref['grad'])
    worst = float((grad_err / np.maximum(np.abs(ref['grad']), 1e-300)).max() / U)
    print('%s: loss %.9g, err %.3e (bound %.3e); worst gradient err %.3f of 2^-24 |g|' % (name, loss, loss_err, ref['kernel_loss_bound'], worst))
    parity_report.note(loss_err / ref['kernel_loss_bound'], label='%s: loss err / derived bound' % name, bound=1.0)
    parity_report.note(worst, label='%s: gradient err / (2^-24 |g|)' % name, bound=1.0)
    assert loss_err <= ref['kernel_loss_bound'], (name, loss_err, ref['kernel_loss_bound'])
    assert np.all(grad_err <= ref['kernel_grad_bound']), (name, worst)
    assert np.all(grad[~ref['mask']] == 0.0), name
    return loss, grad, ref


# ---------------------------------------------------------------------------------------------------------------- 1. golden cases
@pytest.mark.parametrize('name', seqloss_ref64.GOLDEN_CASES)
def test_golden_cases_through_an_identity_loss(golden, name):
    _, _, seq_len, feature_loss, want_loss, want_grad, _ = seqloss_ref64.golden_case(golden(seqloss_ref64.GOLDEN), name)
    loss, grad, ref = _check_against_ref64(name, feature_loss, seq_len)
    loss_err, grad_err = abs(loss - want_loss), np.abs(grad.astype(np.float64) - want_grad)
    print('%s: against the golden values: loss err %.3e (bound %.3e)' % (name, loss_err, ref['kernel_loss_bound'] + ref['golden_loss_bound']))
    assert loss_err <= ref['kernel_loss_bound'] + ref['golden_loss_bound'], (name, loss_err)
    assert np.all(grad_err <= ref['kernel_grad_bound'] + ref['golden_grad_bound']), name


# ------------------------------------------------------------------------------------------------------------------ 2. end to end
def _l1(predictions, targets):
    return F.l1_loss(predictions, targets, reduction='none')


def _huber(predictions, targets):
    return F.smooth_l1_loss(predictions, targets, reduction='none')


def _signed(predictions, targets):
    return predictions - targets


@pytest.mark.parametrize('name, loss_fn', [('l1_ragged', _l1), ('huber', _huber), ('signed', _signed)])
def test_end_to_end_with_the_loss_function_on_the_device(golden, name, loss_fn):
    pred, target, seq_len, feature_loss, want_loss, _, want_grad = seqloss_ref64.golden_case(golden(seqloss_ref64.GOLDEN), name)
    x = _dev(pred, grad=True)
    loss = losses.sequence_loss(loss_fn)(x, _dev(target), _lengths(seq_len))
    loss.backward()
    ref = seqloss_ref64.seq_mean(feature_loss, seq_len)
    loss_err = abs(loss.item() - want_loss)
    grad_err = np.abs(x.grad.cpu().numpy().astype(np.float64) - want_grad)
    worst = float((grad_err / np.maximum(np.abs(want_grad.astype(np.float64)), 1e-300)).max() / U)
    print('%s: loss err %.3e; worst grad_pred err %.3f of 2^-24 |value| (bound 3)' % (name, loss_err, worst))
    parity_report.note(worst / 3.0, label='%s: grad_pred err / (3 2^-24 |value|)' % name, bound=1.0)
    # the feature loss may differ from the recorded one by a rounding of each element (the device's own l1 / smooth_l1): 2^-24 A64
    assert loss_err <= ref['kernel_loss_bound'] + ref['golden_loss_bound'] + U * ref['abs_loss'], (name, loss_err)
    assert np.all(grad_err <= 3 * U * np.abs(want_grad)), (name, worst)


def test_feature_loss_narrower_than_the_predictions(golden):
    """A Gaussian negative log likelihood over (mean | log-variance) columns halves the width: D' = 5 from predictions of 10."""
    pred, target, seq_len, feature_loss, want_loss, _, want_grad = seqloss_ref64.golden_case(golden(seqloss_ref64.GOLDEN), 'nll')

    @losses.sequence_loss
    def nll(predictions, targets):
        mu, logvar = predictions[:, :, :5], predictions[:, :, 5:]
        return 0.5 * (logvar + (targets - mu) ** 2 * torch.exp(-logvar))

    x = _dev(pred, grad=True)
    loss = nll(x, _dev(target), _lengths(seq_len).int())                    # narrower integers are widened
    loss.backward()
    # exp and the products round differently on the device: a loose check that the plumbing is right, the tight ones are above
    assert abs(loss.item() - want_loss) <= 1e-5 * abs(want_loss)
    assert parity_report.rel_err(x.grad.cpu().numpy(), want_grad, 'nll grad_pred') <= 1e-5


# ------------------------------------------------------------------------------------------------- 3. both kernels, every stride pattern
def _layouts(values):
    """The same (B, T, D) values in device tensors of different strides and alignments: name -> tensor."""
    b, t, d = values.shape
    out = {'contiguous': _dev(values)}
    wide = np.full((b, t, d + 4), 1e30, dtype=np.float32)
    wide[:, :, 3:3 + d] = values
    out['column slice'] = _dev(wide)[:, :, 3:3 + d]
    for shift in (1, 2, 3):
        flat = torch.full((values.size + 8,), 1e30, dtype=torch.float32, device=DEV)
        flat[shift:shift + values.size] = _dev(values).reshape(-1)
        view = flat[shift:shift + values.size].view(b, t, d)
        assert view.data_ptr() % 16 == 4 * shift and view.is_contiguous()
        out['base %d floats off' % shift] = view
    out['feature-major storage'] = _dev(np.ascontiguousarray(values.transpose(2, 0, 1))).permute(1, 2, 0)
    gaps = torch.full((b, t + 2, d), 1e30, dtype=torch.float32, device=DEV)
    gaps[:, :t] = _dev(values)
    out['batch stride with a gap'] = gaps[:, :t]
    for name, x in out.items():
        assert x.shape == values.shape and np.array_equal(x.cpu().numpy(), values), name
    return out


@pytest.mark.parametrize('shape, seq_len', [((2, 8, 4), [8, 3]), ((3, 7, 5), [7, 4, 1]), ((2, 300, 61), [300, 17])])
def test_every_layout_gives_the_same_bits(shape, seq_len):
    """(2, 8, 4): T D a multiple of 4 and aligned; (3, 7, 5): not a multiple of 4, so utterances 1 and 2 start off a 16-byte boundary;
    (2, 300, 61): three chunks an utterance.  Contiguous rows at every misalignment (the 16-byte loads behind a scalar head and tail),
    a column slice, a gap between utterances and feature-major storage (one element per load) - one summation order, the same bits."""
    values = np.random.RandomState(sum(shape)).standard_normal(shape).astype(np.float32)
    n = _lengths(seq_len)
    want = ops.masked_seq_mean(_dev(values), n)
    ref = seqloss_ref64.seq_mean(values, seq_len)
    assert abs(want.item() - ref['loss']) <= ref['kernel_loss_bound']
    for name, x in _layouts(values).items():
        before = x.clone()
        got = ops.masked_seq_mean(x, n)
        assert torch.equal(got, want), (name, got.item(), want.item())
        assert torch.equal(identity(x, None, n), want), name
        assert torch.equal(x, before), name                                  # only read


def test_misaligned_slice_and_expanded_operand_are_read_in_place():
    rng = np.random.RandomState(9)
    n = _lengths([7, 4, 1])
    six = _dev(rng.standard_normal((3, 7, 6)).astype(np.float32))
    view = six[:, :, 1:]                                                    # the base is 4 bytes off a 16-byte boundary
    assert view.data_ptr() % 16 == 4 and not view.is_contiguous()
    assert torch.equal(ops.masked_seq_mean(view, n), ops.masked_seq_mean(view.contiguous(), n))
    column = _dev(rng.standard_normal((3, 7, 1)).astype(np.float32))
    for expanded in (column.expand(3, 7, 5), column[:, :1].expand(3, 7, 1), column[:1].expand(3, 7, 1)):
        assert 0 in expanded.stride()
        assert torch.equal(ops.masked_seq_mean(expanded, n), ops.masked_seq_mean(expanded.contiguous(), n))
    # through the wrapper: a loss function that returns a broadcast view, and the gradient that flows back through the expand
    x = column.clone().requires_grad_(True)
    loss = losses.sequence_loss(lambda p, y: p.expand(3, 7, 5))(x, None, n)
    loss.backward()
    x2 = column.clone().requires_grad_(True)
    loss2 = identity(x2.expand(3, 7, 5).contiguous(), None, n)
    loss2.backward()
    assert torch.equal(loss.detach(), loss2.detach()) and torch.equal(x.grad, x2.grad)


# ------------------------------------------------------------------------------------------------------------ 4. / 5. chunks, finish
def test_more_than_one_chunk_per_utterance():
    chunk = _lib.load().mg_seq_mean_chunk()
    shape = (2, 300, 61)
    assert 2 * chunk < shape[1] * shape[2] < 3 * chunk and (shape[1] * shape[2]) % chunk != 0
    values = np.random.RandomState(4).standard_normal(shape).astype(np.float32)
    values[1, 200:] = 1e6                                                   # pad frames of utterance 1, in its last chunks: masked out
    _, grad, ref = _check_against_ref64('three chunks', values, [300, 17])
    assert np.all(grad[0] == grad[0, 0, 0]) and np.all(grad[1, :17] == grad[1, 0, 0]) and grad[1, 0, 0] > grad[0, 0, 0] > 0
    # exactly one chunk and one element more
    for t in (chunk, chunk + 1):
        ones = np.ones((1, t, 1), dtype=np.float32)
        loss, grad = _run(ones, [t - 3])
        assert loss.item() == 1.0 and np.all(grad[0, :t - 3] == np.float32(1.0 / (t - 3))) and np.all(grad[0, t - 3:] == 0.0)


def test_more_utterances_than_the_finishing_pass_has_threads():
    b = 300
    values = np.random.RandomState(5).standard_normal((b, 2, 1)).astype(np.float32)
    seq_len = 1 + (np.arange(b) % 2)
    _, grad, ref = _check_against_ref64('300 utterances', values, seq_len)
    assert np.array_equal(grad[:, 1, 0] != 0, seq_len == 2)
    # an utterance beyond the first 256 counts: change one and the loss moves by its share
    values2 = values.copy()
    values2[299, 0, 0] += 300.0
    loss2, _ = _run(values2, seq_len)
    assert abs((loss2.item() - ref['loss']) - 300.0 / 2 / b) <= 1e-5


# -------------------------------------------------------------------------------------------------------------------- 6. semantics
def test_mask_semantics():
    values = np.random.RandomState(6).standard_normal((3, 7, 5)).astype(np.float32)
    plain_loss, plain_grad = _run(values, [7, 4, 1])
    # a NaN or an Inf in a pad frame reaches the loss, as in the reference (every frame is multiplied by its mask value)
    for poison in (np.nan, np.inf):
        poisoned = values.copy()
        poisoned[1, 5, 2] = poison
        loss, grad = _run(poisoned, [7, 4, 1])
        assert np.isnan(loss.item()) and np.array_equal(grad, plain_grad)
    # an utterance without a valid frame: a NaN loss, NaN gradients on that utterance only
    for empty in (0, -2):
        loss, grad = _run(values, [7, empty, 1])
        assert np.isnan(loss.item()) and np.isnan(grad[1]).all()
        assert np.array_equal(grad[[0, 2]], plain_grad[[0, 2]])
    # lengths beyond T are T; no lengths are all-T lengths, bit for bit
    long_loss, long_grad = _run(values, [7, 4, 9])
    full_loss, full_grad = _run(values, [7, 4, 7])
    assert torch.equal(long_loss, full_loss) and np.array_equal(long_grad, full_grad)
    none_loss, none_grad = _run(values, None)
    all_loss, all_grad = _run(values, [7, 7, 7])
    assert torch.equal(none_loss, all_loss) and np.array_equal(none_grad, all_grad)
    assert abs(none_loss.item() - values.astype(np.float64).mean()) <= 2 * U * np.abs(values).mean()


def test_upstream_gradient_is_read_on_the_device():
    values = np.random.RandomState(7).standard_normal((3, 7, 5)).astype(np.float32)
    x = _dev(values, grad=True)
    scale = torch.tensor(-0.375, device=DEV)
    (identity(x, None, _lengths([7, 4, 1])) * scale).backward()
    ref = seqloss_ref64.seq_mean(values, [7, 4, 1], grad_scale=-0.375)
    assert np.all(np.abs(x.grad.cpu().numpy() - ref['grad']) <= ref['kernel_grad_bound'])
    with pytest.raises(RuntimeError):                                       # no double backward
        y = _dev(values, grad=True)
        (g,) = torch.autograd.grad(identity(y, None, None), y, create_graph=True)
        g.sum().backward()


# -------------------------------------------------------------------------------------------------------------------- 7. determinism
def test_two_calls_give_the_same_bits():
    values = np.random.RandomState(8).standard_normal((2, 300, 61)).astype(np.float32)
    x = _dev(values)
    first, second = _run(x, [300, 17]), _run(x, [300, 17])
    assert torch.equal(first[0], second[0]) and np.array_equal(first[1], second[1])


# ------------------------------------------------------------------------------------------------------------------- 8. no host read
def test_forward_and_backward_capture_into_a_graph():
    rng = np.random.RandomState(10)
    shape = (3, 40, 7)
    pred, target = _dev(rng.standard_normal(shape).astype(np.float32), grad=True), _dev(rng.standard_normal(shape).astype(np.float32))
    n = _lengths([40, 11, 0])
    l1 = losses.sequence_loss(_l1)
    static_loss, static_grad = torch.zeros((), device=DEV), torch.zeros(shape, device=DEV)

    def step():
        loss = l1(pred, target, n)
        (grad,) = torch.autograd.grad(loss, pred)
        return loss.detach(), grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grad = step()
        static_loss.copy_(loss)
        static_grad.copy_(grad)
    for seq_len in ([40, 11, 0], [17, 40, 3]):                              # refreshed inputs, lengths included
        with torch.no_grad():
            pred.copy_(_dev(rng.standard_normal(shape).astype(np.float32)))
            target.copy_(_dev(rng.standard_normal(shape).astype(np.float32)))
            n.copy_(_lengths(seq_len))
        graph.replay()
        torch.cuda.synchronize()
        want_loss, want_grad = step()
        assert torch.equal(static_loss, want_loss) or (torch.isnan(static_loss) and torch.isnan(want_loss))
        assert torch.equal(torch.nan_to_num(static_grad, nan=-7.0), torch.nan_to_num(want_grad, nan=-7.0))
        assert torch.isnan(want_loss).item() == (0 in seq_len)


# -------------------------------------------------------------------------------------------------------------- 9. stream integration
def _two_stream_model(custom):
    torch.manual_seed(13)
    layers = utils.SequentialWithRecurrent(nn.Linear(609, 32), nn.Sigmoid(), nn.Linear(32, 3 + 6), precision='fp32')
    squared = losses.sequence_loss(lambda p, y: (p - y) ** 2)
    streams = [models.Stream('lf0', 3, 'mse'), models.Stream('mcep', 6, loss=squared if custom else 'mse')]
    model = models.StreamModel(layers, streams, fused_loss=False).to(DEV)
    model.output_dims = {'lf0': 3, 'mcep': 6}
    return model


def test_stream_model_with_a_callable_loss():
    feats = synthetic.make_acoustic_batch(2, (9, 12), streams=(('lf0', 3, 'mse'), ('mcep', 6, 'mse')), seed=71, with_raw=True)
    t = feats['normalised_counters'].shape[1]
    assert t == 12 and feats['n_frames'].min() < 12
    feats = data.to_device(feats, DEV)
    custom, plain = _two_stream_model(True), _two_stream_model(False)
    plain.load_state_dict(custom.state_dict())
    for model in (custom, plain):
        synthetic.acoustic_normalisers(model, device=DEV)
        model.mode = 'train'
        model.metrics.reset_state('train')
    loss_c, out_c = custom(feats)
    loss_p, out_p = plain(feats)
    loss_c.backward()
    loss_p.backward()
    assert set(out_c) == set(out_p) == {'normalised_lf0_deltas', 'lf0', 'normalised_mcep_deltas', 'mcep'}
    assert parity_report.rel_err(out_c['mcep'].cpu().numpy(), out_p['mcep'].cpu().numpy(), 'MLPG trajectory of the callable stream') <= 1e-6
    summands = t * 6                                                        # of one utterance of the custom stream
    rel = abs(loss_c.item() - loss_p.item()) / abs(loss_p.item())
    print('callable stream against mse: loss %.9g vs %.9g, rel %.3e (bound %.3e)' % (loss_c.item(), loss_p.item(), rel, summands * U))
    assert parity_report.note(rel, 'callable stream vs mse: loss') <= summands * U
    for (name, p), (_, q) in zip(custom.named_parameters(), plain.named_parameters()):
        assert parity_report.rel_err(p.grad.cpu().numpy(), q.grad.cpu().numpy(), 'callable stream vs mse: d' + name) <= 1e-5, name
