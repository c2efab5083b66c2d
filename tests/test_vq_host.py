"""The vector-quantisation layers without a GPU: the float64 restatement of the kernels (tests/vq_ref64.py) against torch's float64
autograd of the textbook formulation, against central finite differences and a hand-computed EMA step; the inputs of the GPU tests
(every row decided under the reference alone); the C ABI's argument checks; the host layers' refusals."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from morgana_amd import _lib, ops
from morgana_amd import functional as F_hip

import vq_ref64 as ref


# ------------------------------------------------------------------------------------------------------ the restatement itself
def _textbook(z, codebook, grad_latent, grad_loss, cw, beta):
    """z_q = E[argmin cdist]; latent = z_e + sg(z_q - z_e); loss = cw mse(sg(z_e), z_q) + beta mse(z_e, sg(z_q)) - torch float64."""
    z_e = torch.from_numpy(z).double().requires_grad_(True)
    e = torch.from_numpy(codebook).double().requires_grad_(True)
    index = torch.argmin(((z_e.detach()[:, None, :] - e.detach()[None, :, :]) ** 2).sum(-1), dim=1)
    z_q = e[index]
    latent = z_e + (z_q - z_e).detach()
    loss = cw * F.mse_loss(z_e.detach(), z_q) + beta * F.mse_loss(z_e, z_q.detach())
    ((latent * torch.from_numpy(grad_latent).double()).sum() + grad_loss * loss).backward()
    return index.numpy(), latent.detach().numpy(), loss.item(), z_e.grad.numpy(), e.grad.numpy()


@pytest.mark.parametrize('n,k,d', [(1, 1, 1), (5, 2, 3), (64, 65, 16), (257, 63, 17)])
def test_restatement_equals_torch_float64_autograd_of_the_textbook_formulation(n, k, d):
    z, codebook = ref.case(n, k, d, seed=1)
    rng = np.random.RandomState(n + k + d)
    grad_latent, grad_loss, cw, beta = rng.standard_normal((n, d)), 1.7, 0.8, 0.25
    index, latent, loss, dz, de = _textbook(z, codebook, grad_latent, grad_loss, cw, beta)
    got = ref.assign(z, codebook)
    assert np.array_equal(got['index'], index) and got['n_valid'] == n
    np.testing.assert_allclose(got['quantised'].astype(np.float64), latent, rtol=1e-12, atol=1e-12)      # z + (q - z) rounds twice
    assert abs((cw + beta) * got['vq'] - loss) <= 1e-12 * abs(loss)
    assert np.array_equal(got['counts'], np.bincount(index, minlength=k))
    p = np.bincount(index, minlength=k) / n
    assert abs(got['perplexity'] - np.exp(-(p[p > 0] * np.log(p[p > 0])).sum())) <= 1e-12 * got['perplexity']
    got_dz, got_de, members = ref.backward(z, got['quantised'], got['index'], n, grad_latent, grad_loss, cw, beta, k)
    np.testing.assert_allclose(got_dz, dz, rtol=1e-12, atol=1e-12 * np.abs(dz).max())
    np.testing.assert_allclose(got_de, de, rtol=1e-12, atol=1e-12 * max(np.abs(de).max(), 1e-300))
    assert np.array_equal(members, got['counts']) and (got_de[members == 0] == 0).all()


def test_restatement_gradients_equal_central_differences_with_assignments_held_fixed():
    n, k, d, cw, beta, g, h = 9, 4, 3, 0.8, 0.25, 1.3, 1e-5
    z, codebook = ref.case(n, k, d, seed=2)
    out = ref.assign(z, codebook)
    index = out['index']
    dz, de, _ = ref.backward(z, out['quantised'], index, n, None, g, cw, beta, k)
    z64, e64 = z.astype(np.float64), codebook.astype(np.float64)
    for i in range(n):
        for j in range(d):
            hi, lo = z64.copy(), z64.copy()
            hi[i, j] += h
            lo[i, j] -= h
            fd = g * (ref.loss_value(hi, e64, index, n, cw, beta)[1] - ref.loss_value(lo, e64, index, n, cw, beta)[1]) / (2 * h)
            assert abs(fd - dz[i, j]) <= 1e-8 * max(np.abs(dz).max(), 1.0), (i, j, fd, dz[i, j])       # the commitment part alone reaches z
    for i in range(k):
        for j in range(d):
            hi, lo = e64.copy(), e64.copy()
            hi[i, j] += h
            lo[i, j] -= h
            fd = g * (ref.loss_value(z64, hi, index, n, cw, beta)[0] - ref.loss_value(z64, lo, index, n, cw, beta)[0]) / (2 * h)
            assert abs(fd - de[i, j]) <= 1e-8 * max(np.abs(de).max(), 1.0), (i, j, fd, de[i, j])       # the codebook part alone reaches E


def test_restatement_ema_on_a_hand_computed_three_code_case():
    z = np.array([[1.0], [3.0], [10.0]], dtype=np.float32)
    index, counts = np.array([0, 0, 2]), np.array([2, 0, 1])
    size, sums, codebook = ref.ema_update(z, index, counts, cluster_size=[1.0, 1.0, 1.0], ema_sum=[[2.0], [5.0], [8.0]], decay=0.5, eps=1e-5)
    assert size.tolist() == [1.5, 0.5, 1.0]                      # 0.5 * 1 + 0.5 * (2, 0, 1)
    assert sums[:, 0].tolist() == [3.0, 2.5, 9.0]                # 0.5 * (2, 5, 8) + 0.5 * (1 + 3, 0, 10)
    total = 3.0                                                  # 1.5 + 0.5 + 1.0
    for k, (n_k, m_k) in enumerate(((1.5, 3.0), (0.5, 2.5), (1.0, 9.0))):
        want = m_k / ((n_k + 1e-5) / (total + 3 * 1e-5) * total)
        assert abs(codebook[k, 0] - want) <= 1e-15 * want
    assert abs(codebook[1, 0] - 5.0) < 1e-3                      # the code without members decays in both states and stays where it was
    # a code whose size has decayed to nothing does not divide by zero
    _, _, cb = ref.ema_update(z, index, counts, cluster_size=[1.0, 0.0, 1.0], ema_sum=[[2.0], [5.0], [8.0]], decay=0.5)
    assert np.isfinite(cb).all()


def test_restatement_edge_rules():
    codebook = np.array([[0.0, 1.0], [0.0, 1.0], [5.0, 5.0]], dtype=np.float32)
    out = ref.assign(np.array([[0.0, 1.0], [np.nan, 0.0], [4.0, 4.0]], dtype=np.float32), codebook)
    assert out['index'].tolist() == [0, 0, 2] and out['best'][0] == 0.0 and np.isnan(out['best'][1]) and np.isnan(out['vq'])
    ragged = ref.assign(np.full((2, 3, 2), np.nan, dtype=np.float32), codebook, seq_len=[0, 0])
    assert ragged['n_valid'] == 0 and (ragged['index'] == -1).all() and not ragged['quantised'].any()
    z = np.zeros((2, 3, 2), dtype=np.float32)
    z[0, 2] = z[1, 1:] = np.nan                                  # pad rows: poisoned, never looked at
    part = ref.assign(z, codebook, seq_len=[2, 1])
    assert part['index'].tolist() == [0, 0, -1, 0, -1, -1] and part['n_valid'] == 3 and part['vq'] == 1.0 / 2.0
    assert part['counts'].tolist() == [3, 0, 0] and part['perplexity'] == 1.0


# --------------------------------------------------------------------------------------------------- the inputs of the GPU tests
def test_every_row_of_the_gpu_test_inputs_is_decided_under_the_reference_alone():
    """The GPU tests compare codes on decided rows only and may leave out at most 1 % of the rows; the chosen data leaves out none."""
    cases = list(ref.assign_cases())
    assert len(cases) == len(ref.ASSIGN_N) * (len(ref.ASSIGN_K) + 1) * len(ref.ASSIGN_D)
    assert {ref.tile_codes(d) + 1 for d in ref.ASSIGN_D} == {8193, 2731, 482, 127}
    for n, k, d in cases:
        z, codebook = ref.case(n, k, d)
        out = ref.assign(z, codebook)
        assert out['decided'].all(), (n, k, d, int((~out['decided']).sum()))
        assert out['counts'].sum() == n


def test_the_margin_flags_a_near_tie_and_passes_a_clear_win():
    codebook = np.array([[1.0, 0.0], [1.0 + 2.0 ** -23, 0.0], [3.0, 0.0]], dtype=np.float32)
    midpoint = np.array([[1.0 + 2.0 ** -24, 1e3]], dtype=np.float64)
    assert not ref.assign(midpoint, codebook)['decided'][0]      # 1e6 + 2^-48 either way: below the rounding of the sum
    assert ref.assign(np.array([[1.0, 0.5]], dtype=np.float32), codebook)['decided'][0]


# ------------------------------------------------------------------------------------------------------------ the C ABI, host side
def test_vq_entry_points_validate_their_arguments_without_a_gpu():
    lib = _lib.load()
    assert (_lib.MG_VQ_MAX_CODES, _lib.MG_VQ_MAX_DIM) == (65536, 256)
    assert [lib.mg_vq_tile_codes(d) for d in ref.ASSIGN_D] == [ref.tile_codes(d) for d in ref.ASSIGN_D]
    assert lib.mg_vq_tile_codes(0) == 0 and lib.mg_vq_tile_codes(257) == 0
    assert lib.mg_vq_workspace_bytes(64, 64) >= 64 * 8 + 8 + 64 * 4 and lib.mg_vq_workspace_bytes(64, 0) == 0
    assert lib.mg_vq_workspace_bytes(0, 8) == 0 and lib.mg_vq_workspace_bytes(8, 65537) == 0

    def assign(z=16, ldz=4, n=8, d=4, seq_len=None, s=1, codebook=16, k=3, index=16, quantised=16, vq=16, counts=16, perplexity=16,
               n_valid=16, ws=16, ws_bytes=1 << 20):
        return lib.mg_vq_assign_f32(z, ldz, n, d, seq_len, s, codebook, k, index, quantised, vq, counts, perplexity, n_valid, ws, ws_bytes, None)

    assert assign(z=None) == -1 and 'NULL' in _lib.last_error()
    assert assign(codebook=None) == -1 and assign(index=None) == -1 and assign(n_valid=None) == -1 and assign(counts=None) == -1
    assert assign(k=0) == -1 and 'K=0' in _lib.last_error()
    assert assign(n=0) == -1 and assign(d=0) == -1 and assign(n=-1) == -1
    assert assign(k=65537) == -1 and 'MG_VQ_MAX_CODES' in _lib.last_error()
    assert assign(d=257, ldz=257) == -1 and 'MG_VQ_MAX_DIM' in _lib.last_error()
    assert assign(n=(1 << 24) + 1) == -1 and 'MG_VQ_MAX_ROWS' in _lib.last_error()
    assert assign(ldz=-4) == -1 and 'stride' in _lib.last_error()
    assert assign(ldz=3) == -1
    assert assign(seq_len=16, s=3) == -1 and 'B rows of S=3' in _lib.last_error()        # 8 rows are no multiple of 3
    assert assign(seq_len=16, s=0) == -1
    assert assign(z=18) == -1 and 'aligned' in _lib.last_error()
    assert assign(index=20) == -1
    assert assign(ws=None) == -3 and assign(ws_bytes=8) == -3                            # MG_EWORKSPACE
    with pytest.raises(ValueError):
        _lib.check(assign(k=0), 'mg_vq_assign_f32')

    def bwd(g_lat=None, g_loss=16, z=16, ldz=4, quantised=16, index=16, n_valid=16, n=8, d=4, k=3, dz=16, de=16):
        return lib.mg_vq_bwd_f32(g_lat, g_loss, z, ldz, quantised, index, n_valid, n, d, k, 1.0, 0.25, dz, de, None)

    assert bwd(g_loss=None) == -1 and 'NULL' in _lib.last_error()
    assert bwd(z=None) == -1 and bwd(quantised=None) == -1 and bwd(index=None) == -1 and bwd(n_valid=None) == -1
    assert bwd(dz=None, de=None) == -1 and 'one of dz and dE' in _lib.last_error()
    assert bwd(k=0) == -1 and bwd(k=65537) == -1 and bwd(d=257, ldz=257) == -1 and bwd(n=0) == -1
    assert bwd(ldz=-1) == -1 and 'stride' in _lib.last_error()
    assert bwd(n_valid=20) == -1 and 'aligned' in _lib.last_error()

    def ema(z=16, ldz=4, index=16, counts=16, n=8, d=4, k=3, decay=0.99, eps=1e-5, size=16, sums=16, codebook=16, ws=16, ws_bytes=1 << 20):
        return lib.mg_vq_ema_f32(z, ldz, index, counts, n, d, k, decay, eps, size, sums, codebook, ws, ws_bytes, None)

    assert ema(z=None) == -1 and 'NULL' in _lib.last_error()
    assert ema(counts=None) == -1 and ema(size=None) == -1 and ema(sums=None) == -1 and ema(codebook=None) == -1
    assert ema(k=0) == -1 and ema(k=65537) == -1 and ema(d=257, ldz=257) == -1 and ema(ldz=-4) == -1
    assert ema(decay=1.5) == -1 and 'decay' in _lib.last_error()
    assert ema(decay=-0.1) == -1 and ema(eps=0.0) == -1
    assert ema(ws=None) == -3 and ema(ws_bytes=0) == -3


# ------------------------------------------------------------------------------------------------------------------ host layers
def test_ops_and_the_node_refuse_cpu_tensors_and_bad_shapes():
    z, codebook = torch.zeros(5, 4), torch.zeros(3, 4)
    with pytest.raises(_lib.MorganaHipError):
        ops.vq_assign(z, codebook)
    with pytest.raises(_lib.MorganaHipError):
        F_hip.VQFn.apply(z, codebook, None, 1.0, 0.25)
    with pytest.raises(_lib.MorganaHipError):
        ops.vq_backward(None, torch.ones(()), z, z, torch.zeros(5, dtype=torch.int64), torch.tensor(5), 3, 1.0, 0.25)
    with pytest.raises(_lib.MorganaHipError):
        ops.vq_ema_update(z, torch.zeros(5, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.ones(3), codebook, codebook, 0.99)
    with pytest.raises(TypeError):
        ops.vq_assign(None, codebook)
