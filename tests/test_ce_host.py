"""Host-side checks of the categorical cross entropy (no GPU): the float64 restatement against the reference's recorded numbers,
torch's own fp32 CPU kernel inside the derived fp32 bound on every input the GPU tests use, argument validation of mg_masked_ce_f32,
the host layer's refusals and the collate of an integer per-frame feature."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ce_ref64
from morgana_amd import _lib, data, losses

GOLDEN_CASES = ('ragged', 'full', 'c2', 'c65', 'ignore')


def _golden_case(g, name):
    seq_len = g.get(name + '__seq_len')
    return g[name + '__pred'], g[name + '__target'], seq_len


def _torch_cpu(pred, target, seq_len):
    """torch's fp32 CPU evaluation, composed as the reference composes it: per-frame losses, total loss, d loss / d pred."""
    x = torch.from_numpy(np.array(pred, dtype=np.float32)).requires_grad_(True)
    y = torch.from_numpy(np.array(target, dtype=np.int64))
    frame = F.cross_entropy(x.transpose(1, 2), y, reduction='none').unsqueeze(-1)
    b, t = y.shape
    n = torch.full((b,), t, dtype=torch.int64) if seq_len is None else torch.from_numpy(np.array(seq_len)).clamp(0, t)
    mask = (torch.arange(t)[None, :] < n[:, None]).to(frame.dtype).unsqueeze(-1)
    loss = torch.mean(torch.sum(frame * mask, dim=1) / torch.sum(mask, dim=1))
    loss.backward()
    return frame.detach().numpy()[:, :, 0], float(loss.detach()), x.grad.numpy()


def _all_inputs():
    for c in ce_ref64.SWEEP_CLASSES:
        yield 'sweep C=%d' % c, ce_ref64.sweep_case(c)
    for name, case in ce_ref64.range_cases().items():
        yield name, case


def test_ref64_matches_the_reference_golden(golden):
    g = golden('g18_ce.npz')
    assert sorted(str(n) for n in g['cases']) == sorted(GOLDEN_CASES)
    for name in GOLDEN_CASES:
        pred, target, seq_len = _golden_case(g, name)
        ref = ce_ref64.ce(pred, target, seq_len)
        assert abs(ref['loss'] - float(g[name + '__loss'])) <= 1e-4 * abs(float(g[name + '__loss'])), name
        want = g[name + '__grad'].astype(np.float64)
        assert np.abs(ref['grad'] - want).max() <= 1e-4 * np.abs(want).max(), name
    # the golden 'ignore' case really has ignored valid frames and the ragged cases really have pad frames
    _, target, seq_len = _golden_case(g, 'ignore')
    valid = np.arange(target.shape[1])[None, :] < seq_len[:, None]
    assert ((target == -100) & valid).sum() >= 2 and (~valid).sum() > 0


def test_torch_cpu_fp32_sits_inside_the_derived_bound():
    """The bound must hold for an honest fp32 evaluation that is not the kernel: torch's CPU F.cross_entropy, per frame, in total and
    for every gradient element, on every input of the GPU tests."""
    for name, (pred, target, seq_len) in _all_inputs():
        ref = ce_ref64.ce(pred, target, seq_len)
        frame, loss, grad = _torch_cpu(pred, target, seq_len)
        mask = ref['mask']
        err = np.abs(frame.astype(np.float64) - ref['frame_loss'])[mask]
        assert np.all(err <= ref['frame_bound'][mask]), (name, float((err / ref['frame_bound'][mask]).max()))
        assert abs(loss - ref['loss']) <= ref['loss_bound'], (name, abs(loss - ref['loss']), ref['loss_bound'])
        gerr = np.abs(grad.astype(np.float64) - ref['grad'])
        assert np.all(gerr <= ref['grad_bound']), (name, float((gerr / np.maximum(ref['grad_bound'], 1e-300)).max()))
        assert np.all(grad[~mask] == 0.0)
        # the bound is a rounding bound, not a tolerance: a few hundred units of roundoff of the loss's own scale at most
        assert ref['loss_bound'] <= 2e-4 * max(abs(ref['loss']), 1.0), name


def test_ref64_edge_semantics():
    pred, target, seq_len = ce_ref64.sweep_case(5)
    ref = ce_ref64.ce(pred, target, seq_len)
    assert np.all(ref['grad'][1, 3:] == 0.0) and np.all(ref['argmax'][1, 3:] == 0)
    pred3, target3, _ = ce_ref64.sweep_case(65)
    assert ce_ref64.ce(pred3, target3, seq_len)['argmax'][0, 1] == 32               # the tie's lower index
    bad = target.copy()
    bad[0, 2] = 5
    out = ce_ref64.ce(pred, bad, seq_len)
    assert np.isnan(out['loss']) and np.all(out['grad'][0, 2] == 0.0) and np.isfinite(out['grad']).all()
    ignored = target.copy()
    ignored[0, 2] = -100
    out = ce_ref64.ce(pred, ignored, seq_len)
    assert np.isfinite(out['loss']) and np.all(out['grad'][0, 2] == 0.0) and out['frame_loss'][0, 2] == 0.0
    empty = ce_ref64.ce(pred, target, np.array([5, 0]))
    assert np.isnan(empty['loss']) and np.all(empty['grad'][1] == 0.0)
    assert ce_ref64.depth(64) == 16 and ce_ref64.depth(1024) == 136


def test_masked_ce_validates_its_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.mg_masked_ce_workspace_bytes(4, 100, 64) >= 4 * 7 * 4
    assert lib.mg_masked_ce_workspace_bytes(4, 100, 2000) >= 4 * 25 * 4

    def call(pred=16, ldp=8, col0=0, target=16, b=2, t=3, c=8, loss=16, grad=None, ldg=0, gcol0=0, ws=16, ws_bytes=1 << 20):
        return lib.mg_masked_ce_f32(pred, ldp, col0, target, None, b, t, c, 1.0, 1.0, 0.0, loss, grad, ldg, gcol0, None, ws, ws_bytes, None)

    assert call(c=0) == -1 and 'C=0' in _lib.last_error()
    assert call(c=-3) == -1 and 'mg_masked_ce_f32' in _lib.last_error()
    assert call(pred=None) == -1 and 'NULL' in _lib.last_error()
    assert call(target=None) == -1 and call(loss=None) == -1
    assert call(c=_lib.MG_CE_MAX_CLASSES + 1, ldp=_lib.MG_CE_MAX_CLASSES + 1) == -1 and 'cap' in _lib.last_error()
    assert call(b=0) == -1 and call(t=0) == -1 and call(b=65536) == -1
    assert call(ldp=7) == -1 and 'ldp=7' in _lib.last_error()                      # the row stride must cover col0 + C
    assert call(ldp=10, col0=3) == -1 and call(col0=-1) == -1
    assert call(grad=16, ldg=8, gcol0=1) == -1 and 'ldg=8' in _lib.last_error()
    assert call(ws=None) == -3 and call(ws_bytes=4) == -3                          # MG_EWORKSPACE
    with pytest.raises(ValueError):
        _lib.check(call(c=0), 'mg_masked_ce_f32')


def test_ce_refuses_float_targets_and_cpu_tensors():
    pred = torch.zeros(2, 3, 4)
    with pytest.raises(TypeError):
        losses.ce(pred, torch.zeros(2, 3))
    with pytest.raises(TypeError):
        losses.ce(pred, torch.zeros(2, 3, 1, dtype=torch.float64))
    with pytest.raises(TypeError):
        losses.ce(pred, torch.zeros(2, 3, dtype=torch.bool))
    with pytest.raises(_lib.MorganaHipError):
        losses.ce(pred, torch.zeros(2, 3, dtype=torch.int64), torch.tensor([3, 2]))
    with pytest.raises(_lib.MorganaHipError):
        losses.ce(pred, torch.zeros(2, 3, 1, dtype=torch.uint8))                   # widened, then refused for the device only
    with pytest.raises(RuntimeError, match=r'The size of tensor a \(3\) must match the size of tensor b \(4\) at non-singleton dimension 1'):
        losses.ce(pred, torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(ValueError):
        losses.multi_stream(torch.zeros(2, 3, 9), [torch.zeros(2, 3, dtype=torch.int64)] * 2, ['ce', 'ce'])
    with pytest.raises(_lib.MorganaHipError):
        losses.multi_stream(torch.zeros(2, 3, 9), [torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.int32)], ['mse', 'ce'])


def test_stream_table_knows_the_categorical_kind():
    from morgana_amd import models
    st = models.Stream('phone', 40, 'ce')
    assert st.is_categorical and not st.is_delta and st.output_key == 'phone_logits'
    for st in models.LSTMAcousticModel(num_layers=1).streams:                      # the shipped table is unchanged
        assert not st.is_categorical and st.output_key == ('vuv' if st.name == 'vuv' else 'normalised_%s_deltas' % st.name)


@pytest.mark.parametrize('dtype', [np.int64, np.int32, np.uint8])
def test_integer_frame_feature_survives_the_collate(dtype):
    """An integer per-frame feature (class indices, (T, 1)) comes out of collate_fn and collate_to_device zero padded, with its
    integer type (int64 stays int64; losses.ce widens the narrower ones) and un-normalised."""
    rng = np.random.RandomState(5)
    lens = [4, 7, 2]
    batch = [{'name': 'u%d' % i, 'n_frames': n, 'lf0': rng.rand(n, 1).astype(np.float32),
              'phone_class': rng.randint(1, 40, size=(n, 1)).astype(dtype)} for i, n in enumerate(lens)]
    want = np.zeros((3, 7, 1), dtype=dtype)
    for i, item in enumerate(batch):
        want[i, :lens[i]] = item['phone_class']
    torch_dtype = {np.int64: torch.int64, np.int32: torch.int32, np.uint8: torch.uint8}[dtype]
    plain = data.collate_fn(batch)
    assert plain['phone_class'].dtype == torch_dtype and np.array_equal(plain['phone_class'].numpy(), want)
    norms = {'lf0': data.MeanVarianceNormaliser('lf0').set_params({'mean': np.array([0.5], np.float32), 'std_dev': np.array([2.0], np.float32)})}
    # (the float features' pad-and-normalise pass needs the device: tests/test_gpu_ce.py runs the whole batch through it)
    out = data.collate_to_device([{k: v for k, v in item.items() if k != 'lf0'} for item in batch], norms, 'cpu')
    assert out['phone_class'].dtype == torch_dtype and np.array_equal(out['phone_class'].numpy(), want)
    assert 'normalised_phone_class' not in out
    assert out['n_frames'].dtype == torch.int64 and out['n_frames'].tolist() == lens
    widened = losses._class_targets(torch.zeros(3, 7, 40), out['phone_class'])
    assert widened.dtype == torch.int64 and tuple(widened.shape) == (3, 7) and np.array_equal(widened.numpy(), want[:, :, 0].astype(np.int64))
