"""Vector quantisation on the HIP path (csrc/vq.hip, ops.vq_*, functional.VQFn) against the float64 restatement of
tests/vq_ref64.py: codes on every decided row, distances, loss, usage and both gradients inside derived bounds, the EMA codebook,
layouts read in place, determinism and capture.

The bounds.  U32 = 2^-24 is one float32 rounding of a result, U64 = 2^-53 one float64 rounding.  Kernel and reference evaluate the
same float64 expressions, in orders that may differ only in how a sum is bracketed; a sum of m terms evaluated in float64 is within
(m - 1) U64 of the sum of the terms' magnitudes whatever the bracketing, so "the float64 term" of a check is (terms + a few) * U64
times the magnitudes summed, doubled for the two evaluations."""
import functools

import numpy as np
import pytest
import torch

from morgana_amd import _lib, ops
from morgana_amd import functional as F_hip

import vq_ref64 as ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U32, U64 = ref.U32, ref.U64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def check_assignment(z, codebook, got, seq_len=None, max_undecided=0.01):
    """(index, quantised, vq, counts, perplexity, n_valid) of ops.vq_assign against the reference of the same inputs."""
    index, quantised, vq, counts, perplexity, n_valid = got
    want = ref.assign(z, codebook, seq_len)
    dim, k = z.shape[-1], codebook.shape[0]
    idx = host(index).reshape(-1)
    decided = want['decided']
    assert (~decided).mean() <= max_undecided
    assert np.array_equal(idx[decided], want['index'][decided])
    assert index.dtype == torch.int64 and tuple(index.shape) == tuple(z.shape[:-1])
    # bit for bit codebook[index], zero rows where the index is -1
    q = host(quantised).reshape(-1, dim)
    rows = np.where((idx >= 0)[:, None], codebook[np.maximum(idx, 0)], np.float32(0))
    assert np.array_equal(q.view(np.uint32), rows.astype(np.float32).view(np.uint32))
    assert n_valid.item() == want['n_valid']
    if decided.all():
        assert np.array_equal(host(counts), want['counts'])
    assert host(counts).sum() == want['n_valid'] and counts.dtype == torch.int32
    n = max(want['n_valid'], 1)
    print('vq %.9g (reference %.9g)  perplexity %.9g (reference %.9g)' % (vq.item(), want['vq'], perplexity.item(), want['perplexity']))
    if np.isnan(want['vq']):
        assert np.isnan(vq.item())
    else:
        # one float32 rounding; 2 x (the N_valid-term sum of distances that are each (D + 2) U64 off, and the division)
        assert abs(vq.item() - want['vq']) <= U32 * want['vq'] + 2 * (n + dim + 4) * U64 * want['vq']
    if np.isnan(want['perplexity']):
        assert np.isnan(perplexity.item())
    elif decided.all():
        # H = -sum_k p ln p: K terms, each a division, a log (a few U64) and a product; exp turns H's absolute error into a relative one
        assert abs(perplexity.item() - want['perplexity']) <= (U32 + (4 * k + 16) * U64) * want['perplexity']
    return want


# ---------------------------------------------------------------------------------------------------------------- 1. assignment
@functools.lru_cache(maxsize=None)
def _case(n, k, d):
    return ref.case(n, k, d)


@pytest.mark.parametrize('d', ref.ASSIGN_D)
@pytest.mark.parametrize('k', ref.ASSIGN_K + ('past_the_tile',))
def test_assignment_matches_the_reference(k, d):
    """K = 'past_the_tile' is mg_vq_tile_codes(D) + 1: the first codebook that needs a second LDS tile (482 codes at D = 16)."""
    tile = _lib.load().mg_vq_tile_codes(d)
    assert tile == ref.tile_codes(d)
    k = tile + 1 if k == 'past_the_tile' else k
    for n in ref.ASSIGN_N:
        assert (n, k, d) in set(ref.assign_cases())
        z, codebook = _case(n, k, d)
        check_assignment(z, codebook, ops.vq_assign(dev(z), dev(codebook)))


# -------------------------------------------------------------------------------------------------------------- 2. ties and edges
def test_duplicated_codes_and_signed_zeros_give_the_lowest_index():
    z, codebook = ref.case(64, 65, 16, seed=3)
    codebook[40] = codebook[7]
    codebook[64] = codebook[7]
    codebook[3] = codebook[50]
    index = host(ops.vq_assign(dev(z), dev(codebook))[0])
    want = ref.assign(z, codebook)['index']
    assert np.array_equal(index, want) and (index == 7).any() and (index == 3).any() and not np.isin(index, (40, 50, 64)).any()
    zeros = np.array([[-0.0, 0.0], [0.0, -0.0], [0.0, 0.0], [1.0, 1.0]], dtype=np.float32)
    for order in ([0, 1, 2, 3], [2, 1, 0, 3], [3, 1, 0, 2]):
        cb = zeros[order]
        idx, q, vq, _, _, _ = ops.vq_assign(dev(np.zeros((3, 2), dtype=np.float32)), dev(cb))
        first = min(i for i, o in enumerate(order) if o != 3)
        assert host(idx).tolist() == [first] * 3 and vq.item() == 0.0
        assert np.array_equal(host(q).view(np.uint32), cb[[first] * 3].view(np.uint32))          # the sign of the chosen zero, kept


def test_a_row_equal_to_a_code_has_distance_zero_and_no_commitment_gradient():
    z, codebook = ref.case(5, 9, 17, seed=4)
    z[:] = codebook[[8, 0, 3, 3, 5]]
    zt = dev(z).requires_grad_(True)
    latent, index, loss, vq, perplexity = F_hip.VQFn.apply(zt, dev(codebook), None, 1.0, 0.25)
    assert host(index).tolist() == [8, 0, 3, 3, 5] and vq.item() == 0.0 and loss.item() == 0.0
    (3.0 * loss).backward()
    assert not zt.grad.any()


def test_one_code():
    z, codebook = ref.case(257, 1, 3, seed=5)
    got = ops.vq_assign(dev(z), dev(codebook))
    want = check_assignment(z, codebook, got)
    assert not host(got[0]).any() and got[3].item() == 257 and got[4].item() == 1.0 and want['perplexity'] == 1.0


def test_codes_a_thousandth_apart_at_offset_a_thousand():
    """|z|^2 - 2 z.e + |e|^2 in float32 rounds each square (4e6) to 0.25: every difference between codes (1e-6) is gone.  The direct
    float64 difference keeps all of them."""
    k, d = 16, 4
    codebook = (1000.0 + 1e-3 * np.arange(k, dtype=np.float64))[:, None].repeat(d, axis=1).astype(np.float32)
    rng = np.random.RandomState(6)
    target = rng.randint(0, k, size=64)
    z = (1000.0 + 1e-3 * (target[:, None] + rng.uniform(-0.3, 0.3, size=(64, d)))).astype(np.float32)
    want = ref.assign(z, codebook)
    assert want['decided'].all() and len(set(want['index'].tolist())) > 8
    z32, e32 = z.astype(np.float32), codebook.astype(np.float32)
    expanded = (z32 * z32).sum(1, dtype=np.float32)[:, None] - np.float32(2) * (z32 @ e32.T) + (e32 * e32).sum(1, dtype=np.float32)[None, :]
    assert not np.array_equal(expanded.argmin(1), want['index'])                       # the data does tell the two forms apart
    got = ops.vq_assign(dev(z), dev(codebook))
    assert np.array_equal(host(got[0]), want['index'])
    check_assignment(z, codebook, got)


def test_nan_rows_and_nan_codes_follow_the_rule():
    z, codebook = ref.case(8, 6, 3, seed=7)
    z[2, 1] = np.nan                                                                   # every distance of row 2 is NaN: code 0, NaN loss
    codebook[4] = np.nan                                                               # a NaN code never wins
    codebook[1] = z[5]                                                                 # ... not even against the exact winner's 0
    index, q, vq, counts, perplexity, _ = ops.vq_assign(dev(z), dev(codebook))
    want = ref.assign(z, codebook)
    assert np.array_equal(host(index), want['index']) and host(index)[2] == 0 and host(index)[5] == 1 and 4 not in host(index)
    assert np.isnan(vq.item()) and np.isnan(want['vq'])
    assert np.array_equal(host(counts), want['counts']) and np.isfinite(perplexity.item())
    assert np.array_equal(host(q).view(np.uint32), codebook[host(index)].view(np.uint32))
    clean = np.delete(z, 2, axis=0)
    assert np.isfinite(ops.vq_assign(dev(clean), dev(codebook))[2].item())


# ---------------------------------------------------------------------------------------------------------------------- 3. layout
def assert_same_bits(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert torch.equal(x.reshape(-1).contiguous().view(torch.uint8), y.reshape(-1).contiguous().view(torch.uint8))


def test_column_slices_and_misaligned_bases_are_read_in_place():
    z, codebook = ref.case(257, 65, 17, seed=8)
    e = dev(codebook)
    plain = ops.vq_assign(dev(z), e)
    wide = torch.full((257, 40), float('nan'), device=DEV)
    wide[:, 11:28] = dev(z)
    view = wide[:, 11:28]
    assert not view.is_contiguous()
    calls = _lib.CALL_LOG = []
    try:
        sliced = ops.vq_assign(view, e)
    finally:
        _lib.CALL_LOG = None
    assert calls == ['mg_vq_assign_f32']
    assert_same_bits(sliced, plain)
    buf = torch.full((257 * 17 + 1,), float('nan'), device=DEV)
    shifted = buf[1:].view(257, 17)
    shifted.copy_(dev(z))
    assert shifted.data_ptr() % 16 == 4
    ebuf = torch.empty(65 * 17 + 3, device=DEV)
    eshift = ebuf[3:].view(65, 17)
    eshift.copy_(e)
    assert_same_bits(ops.vq_assign(shifted, eshift), plain)
    # the gradients read the same views in place
    g = dev(np.random.RandomState(1).standard_normal((257, 17)).astype(np.float32))
    one = torch.full((), 0.7, device=DEV)
    want = ops.vq_backward(g, one, dev(z), plain[1], plain[0], plain[5], 65, 1.0, 0.25)
    assert_same_bits(ops.vq_backward(g, one, view, sliced[1], sliced[0], sliced[5], 65, 1.0, 0.25), want)
    assert_same_bits(ops.vq_backward(g, one, shifted, plain[1], plain[0], plain[5], 65, 1.0, 0.25), want)


def test_ragged_batches_never_read_their_pad_rows():
    b, s, d, k = 5, 7, 3, 9
    rng = np.random.RandomState(9)
    codebook = rng.standard_normal((k, d)).astype(np.float32)
    seq_len = np.array([7, 0, 3, 1, 9], dtype=np.int64)                                # a zero-length item; one length past S
    z = (codebook[rng.randint(0, k, size=(b, s))] + 0.2 * rng.standard_normal((b, s, d))).astype(np.float32)
    valid = ref.valid_rows(z.shape, seq_len).reshape(b, s)
    poisoned = np.where(valid[..., None], z, np.float32(np.nan))
    got = ops.vq_assign(dev(poisoned), dev(codebook), dev(seq_len))
    want = check_assignment(poisoned, codebook, got, seq_len=seq_len)
    assert want['n_valid'] == 7 + 0 + 3 + 1 + 7 and np.isfinite(got[2].item())
    index, q = host(got[0]), host(got[1])
    assert (index[~valid] == -1).all() and (index[valid] >= 0).all() and not q[~valid].any() and np.isfinite(q).all()
    # means over the valid rows only: the loss of the packed valid rows
    packed = ops.vq_assign(dev(z[valid]), dev(codebook))
    assert abs(packed[2].item() - got[2].item()) <= 2 * U32 * got[2].item() and torch.equal(packed[3], got[3])
    # and the gradients: zero rows on the pads, the scale from N_valid
    zt = dev(poisoned).requires_grad_(True)
    et = dev(codebook).requires_grad_(True)
    latent, _, loss, _, _ = F_hip.VQFn.apply(zt, et, dev(seq_len), 1.0, 0.25)
    up = rng.standard_normal((b, s, d)).astype(np.float32)
    ((latent * dev(up)).sum() + loss).backward()
    check_gradients(poisoned, want, up, 1.0, 1.0, 0.25, k, host(zt.grad), host(et.grad))
    assert not host(zt.grad)[~valid].any()


# ------------------------------------------------------------------------------------------------------------------- 4. gradients
def check_gradients(z, want, grad_latent, grad_loss, cw, beta, k, dz, de):
    """Every element of dz and dE against the reference: one float32 rounding of the result, and the float64 term - for dz the two
    products and the sum of its two parts, for dE the sum over the code's members (their count + a few roundings of the magnitudes
    summed), doubled for the two evaluations."""
    dim = z.shape[-1]
    want_dz, want_de, members = ref.backward(z, want['quantised'], want['index'], want['n_valid'], grad_latent, grad_loss, cw, beta, k)
    z2 = np.where((want['index'] >= 0)[:, None], z.reshape(-1, dim).astype(np.float64), 0.0)
    gap = np.abs(z2 - want['quantised'].astype(np.float64))
    scale = abs(grad_loss) * 2.0 / (want['n_valid'] * dim)
    up = np.zeros_like(z2) if grad_latent is None else np.abs(np.asarray(grad_latent, dtype=np.float64).reshape(-1, dim))
    err_dz = np.abs(dz.reshape(-1, dim) - want_dz)
    bound_dz = U32 * np.abs(want_dz) + 2 * 8 * U64 * (up + scale * beta * gap)
    print('dz: worst error / bound %.3f' % (err_dz / np.maximum(bound_dz, 1e-300)).max())
    assert (err_dz <= bound_dz).all()
    mass = np.zeros((k, dim))
    np.add.at(mass, want['index'][want['index'] >= 0], gap[want['index'] >= 0])
    err_de = np.abs(de - want_de)
    bound_de = U32 * np.abs(want_de) + 2 * (members[:, None] + 8) * U64 * scale * cw * mass
    print('dE: worst error / bound %.3f' % (err_de / np.maximum(bound_de, 1e-300)).max())
    assert (err_de <= bound_de).all()
    assert not de[members == 0].any() and not np.signbit(de[members == 0]).any()               # unused codes: exactly +0
    return want_dz, want_de


@pytest.mark.parametrize('n,k,d', [(1, 2, 1), (5, 63, 3), (257, 65, 17), (300, 4, 64)])
def test_gradients_are_inside_the_derived_bounds(n, k, d):
    z, codebook = ref.case(n, k, d, seed=10)
    want = ref.assign(z, codebook)
    assert want['decided'].all()
    rng = np.random.RandomState(n)
    up = rng.standard_normal((n, d)).astype(np.float32)
    for grad_loss, cw, beta, with_latent in ((1.0, 1.0, 0.25, True), (-2.75, 0.6, 1.5, True), (0.3, 1.0, 0.25, False)):
        zt, et = dev(z).requires_grad_(True), dev(codebook).requires_grad_(True)
        latent, index, loss, vq, perplexity = F_hip.VQFn.apply(zt, et, None, cw, beta)
        assert not index.requires_grad and not vq.requires_grad and not perplexity.requires_grad and loss.requires_grad
        assert torch.equal(latent, et.detach()[index])
        assert abs(loss.item() - (cw + beta) * want['vq']) <= 3 * U32 * (cw + beta) * want['vq']
        scale = torch.full((), grad_loss, device=DEV)                                  # the upstream gradient lives on the device
        total = loss * scale + ((latent * dev(up)).sum() if with_latent else 0.0)
        total.backward()
        seen = float(np.float32(grad_loss))                                            # ... as a float32: 0.3 is not 0.3 there
        check_gradients(z, want, up if with_latent else None, seen, cw, beta, k, host(zt.grad), host(et.grad))


def test_codebook_weight_zero_skips_the_codebook_gradient():
    z, codebook = ref.case(64, 8, 16, seed=11)
    zt, et = dev(z).requires_grad_(True), dev(codebook).requires_grad_(True)
    calls = _lib.CALL_LOG = []
    try:
        latent, _, loss, _, _ = F_hip.VQFn.apply(zt, et, None, 0.0, 0.25)
        (loss + latent.sum()).backward()
    finally:
        _lib.CALL_LOG = None
    assert calls == ['mg_vq_assign_f32', 'mg_vq_bwd_f32'] and et.grad is None
    want = ref.assign(z, codebook)
    check_gradients(z, want, np.ones_like(z), 1.0, 0.0, 0.25, 8, host(zt.grad), np.zeros((8, 16)))
    dz, de = ops.vq_backward(None, torch.ones((), device=DEV), dev(z), dev(want['quantised']), dev(want['index']),
                             torch.tensor(64, device=DEV), 8, 1.0, 0.25, want_dz=False)
    assert dz is None
    check_gradients(z, want, None, 1.0, 1.0, 0.25, 8, ref.backward(z, want['quantised'], want['index'], 64, None, 1.0, 1.0, 0.25, 8)[0], host(de))


# --------------------------------------------------------------------------------------------------------------------------- 5. EMA
def check_ema(z, index, counts, before, after, decay):
    """One update from the float32 states ``before`` = (cluster_size, ema_sum, codebook) to ``after``, element by element: one float32
    rounding of each stored result; the float64 term of a sum over a code's members as for dE; the codebook is a quotient of two such
    results, so it inherits the sum's term divided by the smoothed size."""
    size, sums, codebook = ref.ema_update(z, index, counts, before[0], before[1], decay)
    members = np.asarray(counts, dtype=np.float64)
    dim = z.shape[-1]
    assert (np.abs(after[0] - size) <= (U32 + 4 * U64) * np.abs(size)).all()
    mass = np.zeros_like(sums)
    np.add.at(mass, index.reshape(-1)[index.reshape(-1) >= 0], np.abs(z.reshape(-1, dim).astype(np.float64))[index.reshape(-1) >= 0])
    term = 2 * (members[:, None] + 8) * U64 * (decay * np.abs(before[1].astype(np.float64)) + (1 - decay) * mass)
    assert (np.abs(after[1] - sums) <= U32 * np.abs(sums) + term).all()
    stored = size.astype(np.float32).astype(np.float64)
    smoothed = (stored + ref.EMA_EPS) / (stored.sum() + len(counts) * ref.EMA_EPS) * stored.sum()
    assert (np.abs(after[2] - codebook) <= (U32 + 16 * U64) * np.abs(codebook) + term / smoothed[:, None]).all()
    assert np.isfinite(after[2]).all()


def test_ema_one_update_and_three_chained_updates():
    k, d, decay = 9, 17, 0.9
    rng = np.random.RandomState(12)
    codebook = rng.standard_normal((k, d)).astype(np.float32)
    codebook[6] += 50.0                                                               # a code nothing is near: no members, ever
    state = [torch.ones(k, device=DEV), dev(codebook).clone(), dev(codebook).clone()]
    for step in range(3):
        near = codebook[rng.randint(0, 6, size=(4, 30))]
        z = (near + 0.3 * rng.standard_normal(near.shape)).astype(np.float32)
        seq_len = np.array([30, 11, 0, 25], dtype=np.int64)
        before = [host(t).copy() for t in state]
        index, _, _, counts, _, _ = ops.vq_assign(dev(z), state[2], dev(seq_len))
        assert counts[6].item() == 0 and counts.sum().item() == 66
        calls = _lib.CALL_LOG = []
        try:
            ops.vq_ema_update(dev(z), index, counts, state[0], state[1], state[2], decay)
        finally:
            _lib.CALL_LOG = None
        assert calls == ['mg_vq_ema_f32']
        after = [host(t) for t in state]
        zin = np.where(ref.valid_rows(z.shape, seq_len).reshape(4, 30, 1), z, 0)
        check_ema(zin, host(index), host(counts), before, after, decay)
        # the code without members decays in both states - its quotient stays put - and nothing divides by zero
        assert abs(after[0][6] - decay ** (step + 1)) <= 4 * U32 and np.abs(after[2][6] - codebook[6]).max() <= 1e-3 * np.abs(codebook[6]).max()
        assert not np.array_equal(after[2][:6], before[2][:6])
    empty = [torch.zeros(k, device=DEV), torch.zeros(k, d, device=DEV), dev(codebook).clone()]          # sizes that have decayed to nothing
    index, _, _, counts, _, _ = ops.vq_assign(dev(z), empty[2], dev(np.zeros(4, dtype=np.int64)))
    ops.vq_ema_update(dev(z), index, counts, empty[0], empty[1], empty[2], decay)
    assert torch.equal(empty[2], dev(codebook)) and not empty[0].any()                 # nothing assigned, nothing to divide by: left alone


def test_the_latent_of_an_ema_step_uses_the_codebook_from_before_its_update():
    """The node, then the EMA update in place, then the backward: the latent is the OLD codebook's rows bit for bit, and the backward
    reads what the node saved - not the codebook, which has moved by then."""
    torch.manual_seed(13)
    before = torch.empty(8, 4, device=DEV).uniform_(-0.125, 0.125)
    codebook, sizes, sums = before.clone(), torch.ones(8, device=DEV), before.clone()
    x = (0.1 * torch.randn(32, 4, device=DEV)).requires_grad_(True)
    counts = torch.full((8,), -1, dtype=torch.int32, device=DEV)
    latent, code, loss, vq, perplexity = F_hip.VQFn.apply(x, codebook, None, 0.0, 0.25, counts)
    want = ref.assign(host(x), host(before))
    assert np.array_equal(host(counts), want['counts'])                                # filled by the assignment kernel itself
    ops.vq_ema_update(x.detach(), code, counts, sizes, sums, codebook, 0.8)
    assert torch.equal(latent, before[code]) and not torch.equal(codebook, before)
    (loss + (latent ** 2).mean()).backward()
    up = 2.0 * want['quantised'] / (32 * 4)
    check_gradients(host(x), want, up, 1.0, 0.0, 0.25, 8, host(x.grad), np.zeros((8, 4)))


# ------------------------------------------------------------------------------------------------------ 6. determinism and capture
def test_two_calls_give_the_same_bits_and_a_captured_node_replays_on_new_inputs():
    n, k, d = 257, 65, 17
    rng = np.random.RandomState(14)
    z0, codebook = ref.case(n, k, d, seed=14)
    z = dev(z0).requires_grad_(True)
    e = dev(codebook).requires_grad_(True)
    up, scale = dev(rng.standard_normal((n, d)).astype(np.float32)), torch.full((), 1.3, device=DEV)
    state = [torch.ones(k, device=DEV), dev(codebook).clone()]

    def step(sizes, sums, book):
        latent, index, loss, vq, perplexity = F_hip.VQFn.apply(z, e, None, 1.0, 0.25)
        dz, de = torch.autograd.grad((latent * up).sum() + loss * scale, (z, e))
        counts = ops.vq_assign(z.detach(), e.detach())[3]
        ops.vq_ema_update(z.detach(), index, counts, sizes, sums, book, 0.9)
        return latent.detach(), index, loss.detach(), vq, perplexity, dz, de

    def fresh():
        return [state[0].clone(), state[1].clone(), state[1].clone()]

    first, second = step(*fresh()), step(*fresh())
    assert_same_bits(first, second)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*fresh())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    static = fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                      # a host read inside the node would end the capture
        captured = step(*static)
    for seed in (15, 16):
        z1, e1 = ref.case(n, k, d, seed=seed)
        with torch.no_grad():
            z.copy_(dev(z1))
            e.copy_(dev(e1))
            for t, src in zip(static, fresh()):
                t.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        eager_state = fresh()
        want = step(*eager_state)
        assert_same_bits(captured, want)
        assert_same_bits(static, eager_state)
        check_assignment(z1, e1, (captured[1], captured[0], captured[3], ops.vq_assign(z.detach(), e.detach())[3], captured[4],
                                  torch.tensor(n)))
