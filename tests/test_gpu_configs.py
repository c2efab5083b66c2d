"""GPU parity tests at the BASELINE configurations the first round left unexercised (run with ``-m gpu`` on an MI355X):

* C5  RNN_SPSS GRU-512, 600 -> 187, ragged 300-2000-frame utterances, seq_len masking  (morgana/utils.py:366-385, losses.py:37-39)
* C4  RNN_SPSS GRU-512, 600 -> 80 at its real chain length T = 1000: persistent recurrence == per-step kernels over 1000 dependent
      steps at the full (64, 1000, 512) shape, and the model against the oracle on a T = 1000 batch
* C3  the multi-rank code path of the graphed train step on a live RCCL process group (world size 1 on the one-GPU box)
plus the contracts the first review asked to be pinned: backward kernels never read ``saved`` past ``seq_len``, unsupported
recurrent layers raise instead of falling back to torch, the recurrent step is capturable (no host read of ``seq_len``).
Everything goes through the C ABI of libmorgana_hip.so and is compared with the oracle (oracle/ref_cpu.py).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from morgana_amd import _lib, data, models, ops, optim, synthetic, utils
from morgana_amd import functional as F_hip
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
RTOL = 1e-4           # fp32 parity bar (north star)
RTOL_BF16 = 2e-2      # bf16 throughput mode (8-bit mantissa)


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


from parity_report import rel_err          # noqa: E402,F401  max |got - want| / max |want|, recorded per test (gpurun_out/parity_report.json)


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)


def _load_state(model, state):
    own = model.state_dict()
    for key, value in state.items():
        own[key].copy_(torch.from_numpy(value))
    return model


# ------------------------------------------------------------------------------------------------------------ C5
@pytest.fixture(scope='module')
def c5_case():
    """BASELINE C5 at a reduced batch: 8 utterances of 300-2000 frames (P = T / 12.5 phones), 187-dim WORLD target, zero padded
    to the batch maximum as collate_fn pads (data.py:183-193); the oracle's loss / prediction / gradients (about 10 s of numpy)."""
    feats = synthetic.make_batch(8, (300, 2000), out_dim=187, target_name='world', seed=5)
    state = synthetic.rnn_spss_state(out_dim=187)
    want = ref_cpu.rnn_forward_backward(state, feats, target_key='normalised_world')
    return feats, state, want


@pytest.mark.parametrize('precision,packed', [('fp32', True), ('bf16', True), ('bf16', False), ('fp32', False)])
def test_c5_ragged_187_model_vs_oracle(c5_case, precision, packed):
    """RNNSPSS(output_dim=187) on the ragged batch against ``ref_cpu.rnn_forward_backward``: fp32 mode at the north star's 1e-4 on
    loss and prediction (1e-3 on gradients: 2000-step BPTT sums in another order), bf16 mode at 2e-2 / 5e-2 relative L2.  The batch is
    large enough for the persistent recurrence and the phone-rate GRU input to engage (asserted); ``packed`` runs the Linear stack
    behind the GRU and the loss on the sum(T_b) valid frame rows only (utils.PackedFrames) and must not change the result:
    predictions past an utterance's length are whatever the layers make of the GRU's zero rows in the reference, and are compared
    on the valid frames only in both forms (they are outside the loss mask)."""
    feats, state, (want_loss, want_pred, want_grads) = c5_case
    b, t = feats['normalised_world'].shape[:2]
    n_rows = feats['normalised_lab'].shape[0] * feats['normalised_lab'].shape[1]
    assert ops.phone_rate_gru_ok(n_rows, b * t, 512), 'C5 test batch misses the phone-rate GRU input'
    if precision == 'bf16':
        assert ops.gru_persist_ok(b, t, 512), 'C5 test batch misses the persistent recurrence'
    utils.set_packed_frames(packed, rows_min_padding=0.1)      # 0.1: the row-wise runs packed too
    try:
        model = _load_state(models.RNNSPSS(output_dim=187, target_name='world', precision=precision).to(DEV), state)
        loss, out = model(data.to_device(feats, DEV))
        loss.backward()
    finally:
        utils.set_packed_frames(True, rows_min_padding=0.75)
    pred = out['pred_norm_world'].detach().cpu().numpy()
    assert pred.shape == want_pred.shape
    valid = (np.arange(t)[None, :] < feats['n_frames'][:, None])[:, :, None]
    tol, gtol = (RTOL, 1e-3) if precision == 'fp32' else (RTOL_BF16, 5e-2)
    np.testing.assert_allclose(loss.item(), want_loss, rtol=tol)
    assert rel_err(np.where(valid, pred, 0), np.where(valid, want_pred, 0)) < tol
    for name, prm in model.named_parameters():
        err = rel_err(prm.grad.cpu().numpy(), want_grads[name]) if precision == 'fp32' else rel_l2(prm.grad.cpu().numpy(), want_grads[name])
        assert err < gtol, (name, err)


def test_c5_packed_rows_equal_padded_rows(c5_case):
    """The packed-frame form against the padded form of the same model and batch, bf16 mode: same kernels on fewer rows, so the
    loss and the valid predictions are EQUAL bit for bit; weight gradients sum the same terms in another split order (1e-5)."""
    feats, state, _ = c5_case
    t = feats['normalised_world'].shape[1]
    valid = torch.from_numpy((np.arange(t)[None, :] < feats['n_frames'][:, None])[:, :, None]).to(DEV)
    results = []
    for packed in (True, False):
        utils.set_packed_frames(packed, rows_min_padding=0.1)      # 0.1: the row-wise runs packed too
        try:
            model = _load_state(models.RNNSPSS(output_dim=187, target_name='world', precision='bf16').to(DEV), state)
            loss, out = model(data.to_device(feats, DEV))
            loss.backward()
        finally:
            utils.set_packed_frames(True, rows_min_padding=0.75)
        results.append((loss.detach().clone(), torch.where(valid, out['pred_norm_world'].detach(), torch.zeros((), device=DEV)),
                        {n: p.grad.detach().clone() for n, p in model.named_parameters()}))
    (loss_p, pred_p, grads_p), (loss_d, pred_d, grads_d) = results
    assert torch.equal(pred_p, pred_d)
    np.testing.assert_allclose(loss_p.item(), loss_d.item(), rtol=1e-6)
    for name in grads_d:
        assert rel_l2(grads_p[name].cpu().numpy(), grads_d[name].cpu().numpy()) < 1e-4, name


def test_c5_at_its_per_rank_size():
    """BASELINE C5 at the size ONE RANK runs it (64 utterances of 300-2000 frames, 187 outputs), bf16 mode,
    through properties that do not need 80 s of oracle time:
      * the phone-rate GRU input and the persistent recurrence engage, the persistent status word stays clean;
      * packed frame rows == padded rows: valid predictions bit for bit, loss to 1e-6, gradients to 1e-4 (another split order);
      * utterances are independent (morgana/losses.py:37-42: a mean over utterances of per-utterance means): the two half batches
        give the SAME valid predictions bit for bit, the mean of their losses is the loss, the mean of their gradients the gradient;
      * the first 8 utterances' predictions against the oracle (the only part that costs oracle time: 8 utterances)."""
    feats = synthetic.make_batch(64, (300, 2000), out_dim=187, target_name='world', seed=5)
    state = synthetic.rnn_spss_state(out_dim=187)
    b, t = feats['normalised_world'].shape[:2]
    assert ops.phone_rate_gru_ok(feats['normalised_lab'].shape[0] * feats['normalised_lab'].shape[1], b * t, 512)
    assert ops.gru_persist_ok(b, t, 512)

    def run(batch, packed=True):
        utils.set_packed_frames(packed, rows_min_padding=0.1)      # 0.1: the row-wise runs packed too
        try:
            model = _load_state(models.RNNSPSS(output_dim=187, target_name='world', precision='bf16').to(DEV), state)
            loss, out = model(data.to_device(batch, DEV))
            loss.backward()
            ops.check_persistent_status()              # raises if a persistent launch gave up on a peer
        finally:
            utils.set_packed_frames(True, rows_min_padding=0.75)
        tt = batch['normalised_world'].shape[1]
        valid = torch.from_numpy((np.arange(tt)[None, :] < batch['n_frames'][:, None])[:, :, None]).to(DEV)
        pred = torch.where(valid, out['pred_norm_world'].detach(), torch.zeros((), device=DEV))
        return loss.item(), pred, {n: p.grad.detach().cpu().numpy().astype(np.float64) for n, p in model.named_parameters()}

    loss_p, pred_p, grads_p = run(feats, packed=True)
    loss_d, pred_d, grads_d = run(feats, packed=False)
    assert torch.equal(pred_p, pred_d)
    np.testing.assert_allclose(loss_p, loss_d, rtol=1e-6)
    for name in grads_d:
        assert rel_l2(grads_p[name], grads_d[name]) < 1e-4, name

    halves = [run(synthetic.shard_batch(feats, r, 2)) for r in range(2)]
    for r, (_, pred_h, _) in enumerate(halves):
        th = pred_h.shape[1]
        assert torch.equal(pred_h, pred_p[32 * r:32 * (r + 1), :th]), r
        assert not bool(pred_p[32 * r:32 * (r + 1), th:].any())            # nothing valid beyond the half's own longest utterance
    np.testing.assert_allclose(0.5 * (halves[0][0] + halves[1][0]), loss_p, rtol=1e-5)
    for name in grads_p:
        assert rel_l2(0.5 * (halves[0][2][name] + halves[1][2][name]), grads_p[name]) < 1e-4, name

    sub = synthetic.shard_batch(feats, 0, 8)
    _, want_pred, _ = ref_cpu.rnn_forward_backward(state, sub, target_key='normalised_world')
    t8 = want_pred.shape[1]
    valid8 = (np.arange(t8)[None, :] < sub['n_frames'][:, None])[:, :, None]
    assert rel_err(pred_p[:8, :t8].cpu().numpy(), np.where(valid8, want_pred, 0)) < RTOL_BF16


# ------------------------------------------------------------------------------------------------------------ C4
def test_c4_persistent_recurrence_equals_step_kernels_at_t1000():
    """mg_gru_fwd_persist_bf16 / mg_gru_bwd_persist_bf16 at the full C4 shape (64, 1000, 512) against the per-step kernels that
    share their cell code: 1000 dependent hand-offs per direction, results EQUAL bit for bit (outputs, states, saved gates, gate
    gradients, dh0).  Lengths: mostly full (C4 is fixed length) with a few shorter items, so frozen states ride along."""
    b, t, hid = 64, 1000, 512
    rng = np.random.RandomState(1000)
    xproj = dev(rng.standard_normal((b, t, 3 * hid)).astype(np.float32))
    w_hh = dev((rng.uniform(-1, 1, (3 * hid, hid)) / np.sqrt(hid)).astype(np.float32))
    b_hh = dev(rng.uniform(-0.1, 0.1, 3 * hid).astype(np.float32))
    sl_np = np.full(b, t, dtype=np.int64)
    sl_np[[3, 17, 40]] = [1, 500, 999]
    sl = dev(sl_np)
    assert ops.gru_persist_ok(b, t, hid)
    out_s, hs_s, sv_s, hsbf_s = ops.gru_fwd_bf16(xproj, w_hh, b_hh, sl, None, b, t, hid, persistent=False)
    out_p, hs_p, sv_p, hsbf_p = ops.gru_fwd_bf16(xproj, w_hh, b_hh, sl, None, b, t, hid, persistent=True)
    assert torch.equal(out_p, out_s) and torch.equal(hs_p, hs_s) and torch.equal(hsbf_p, hsbf_s)
    valid = dev((np.arange(t)[None, :] < sl_np[:, None])[:, :, None])
    zero = torch.zeros((), device=DEV)
    assert torch.equal(torch.where(valid, sv_p, zero), torch.where(valid, sv_s, zero))
    g_out = dev(rng.standard_normal((b, t, hid)).astype(np.float32) * 0.1)
    g_hn = dev(rng.standard_normal((b, hid)).astype(np.float32) * 0.1)
    dx_s, dh_s, d0_s, dhbf_s = ops.gru_bwd_bf16(g_out, g_hn, hs_s, sv_s, w_hh, sl, b, t, hid, persistent=False)
    dx_p, dh_p, d0_p, dhbf_p = ops.gru_bwd_bf16(g_out, g_hn, hs_s, sv_s, w_hh, sl, b, t, hid, persistent=True)
    assert torch.equal(dx_p, dx_s) and torch.equal(dh_p, dh_s) and torch.equal(d0_p, d0_s) and torch.equal(dhbf_p, dhbf_s)
    assert torch.isfinite(dx_p).all()


def test_persistent_gru_reads_its_input_projections_through_a_row_map():
    """mg_gru_fwd_persist_rows_bf16 (the recurrence takes frame (b, t)'s input projection from row xrows[b, t] of a phone-level table:
    upsample_to_repetitions applied inside the launch) against the same launch on the explicitly repeated rows: EQUAL in every output.
    Ragged lengths, a table with runs of 1-30 frames per row and a shared zero row for the padding frames."""
    b, t, hid = 24, 300, 512
    rng = np.random.RandomState(7)
    n_rows = 700
    table = dev(rng.standard_normal((n_rows + 1, 3 * hid)).astype(np.float32))
    table[n_rows].zero_()
    lens = rng.randint(1, t + 1, size=b)
    lens[0] = t
    rows_np = np.full((b, t), n_rows, dtype=np.int32)
    for i in range(b):
        reps = rng.randint(1, 31, size=t)
        ids = np.repeat(rng.randint(0, n_rows, size=t), reps)[:lens[i]]
        rows_np[i, :lens[i]] = ids
    rows, sl = dev(rows_np), dev(lens.astype(np.int64))
    w_hh = dev((rng.uniform(-1, 1, (3 * hid, hid)) / np.sqrt(hid)).astype(np.float32))
    b_hh = dev(rng.uniform(-0.1, 0.1, 3 * hid).astype(np.float32))
    assert ops.gru_persist_ok(b, t, hid)
    dense = table[rows.reshape(-1).long()].view(b, t, 3 * hid).contiguous()
    want = ops.gru_fwd_bf16(dense, w_hh, b_hh, sl, None, b, t, hid, persistent=True)
    got = ops.gru_fwd_bf16(table, w_hh, b_hh, sl, None, b, t, hid, persistent=True, xrows=rows)
    ops.check_persistent_status()
    valid = dev((np.arange(t)[None, :] < lens[:, None])[:, :, None])
    zero = torch.zeros((), device=DEV)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[3], want[3])
    assert torch.equal(torch.where(valid, got[2], zero), torch.where(valid, want[2], zero))


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16'])
def test_c4_model_t1000_vs_oracle(precision):
    """The C4 model (600 -> 512 -> GRU-512 -> 256 -> 80) on 8 fixed-length 1000-frame utterances (C4's chain length; a smaller batch
    keeps the numpy oracle at seconds) against the oracle, fp32 at 1e-4 / 1e-3, bf16 at 2e-2 / 5e-2 (relative L2 on gradients)."""
    feats = synthetic.make_batch(8, 1000, out_dim=80, target_name='mcep', seed=1004)
    state = synthetic.rnn_spss_state()
    want_loss, want_pred, want_grads = ref_cpu.rnn_forward_backward(state, feats)
    model = _load_state(models.RNNSPSS(precision=precision).to(DEV), state)
    loss, out = model(data.to_device(feats, DEV))
    loss.backward()
    # 'bf16x3' (split-bf16 row-wise layers, exact-fp32 recurrence) is held to fp32 mode's bars
    exact = precision in ('fp32', 'bf16x3')
    tol, gtol = (RTOL, 1e-3) if exact else (RTOL_BF16, 5e-2)
    np.testing.assert_allclose(loss.item(), want_loss, rtol=tol)
    assert rel_err(out['pred_norm_mcep'].detach().cpu().numpy(), want_pred) < tol
    for name, prm in model.named_parameters():
        err = rel_err(prm.grad.cpu().numpy(), want_grads[name]) if exact else rel_l2(prm.grad.cpu().numpy(), want_grads[name])
        assert err < gtol, (name, err)


def test_recurrent_step_graph_replay_equals_eager():
    """With ``max_len`` handed down (models.RNNSPSS does) the GRU wrapper reads nothing back from the device, so the whole
    recurrent training step - persistent recurrences included - is captured as one HIP graph: replays against eager steps on the
    same batch, parameters and losses EQUAL bit for bit."""
    from morgana_amd import graphs
    feats = data.to_device(synthetic.make_batch(16, (150, 260), out_dim=80, target_name='mcep', seed=21), DEV)

    def fresh():
        model = _load_state(models.RNNSPSS(precision='bf16').to(DEV), synthetic.rnn_spss_state())
        return model, optim.Adam(model.parameters(), lr=0.002)

    model_e, opt_e = fresh()
    losses_e = []
    for _ in range(6):
        opt_e.zero_grad()
        loss, _ = model_e(feats)
        F_hip.backward(loss)
        opt_e.step()
        losses_e.append(loss.item())
    model_g, opt_g = fresh()
    step = graphs.GraphedTrainStep(model_g, opt_g, feats, warmup=2)
    losses_g = [step().clone() for _ in range(4)]
    assert [v.item() for v in losses_g] == losses_e[2:]
    for key in ('param', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(opt_e.flat_buffers()[key], opt_g.flat_buffers()[key]), key


# ------------------------------------------------------------------------------------------------------------ C3
def test_rccl_world1_graphed_step_equals_single_rank():
    """First contact with RCCL: a world-size-1 ``nccl`` process group on the one GPU.  ``GraphedTrainStep`` is forced onto its
    multi-rank path (forward + backward + early bucket exchange captured while the process group's watchdog thread is alive, the
    gradient all-reduce through RCCL, the Adam kernel behind it) and must reproduce the single-rank graphed step bit for bit: an
    all-reduce over one rank is the identity and 1/world = 1.  Two batches: a small one (generic kernels) and C2's 256 x 1000 frames,
    where the single-rank step leaves its weight-gradient slabs to the update kernel and the multi-rank step sums the same slabs with
    one reduce launch per layer in front of the exchange (mg_slab_reduce_f32) - the same sums in the same order."""
    import torch.distributed as dist
    from morgana_amd import graphs
    batches = [data.to_device(synthetic.make_batch(32, 200, seed=8), DEV), data.to_device(synthetic.make_batch(256, 1000, seed=9), DEV)]
    data.add_bf16_table(batches[1])

    def fresh(**kw):
        model = _load_state(models.F0Model(precision='bf16').to(DEV), synthetic.f0_model_state())
        return model, optim.Adam(model.parameters(), lr=0.01, **kw)

    losses_s = []
    for feats in batches:
        model_s, opt_s = fresh()
        single = graphs.GraphedTrainStep(model_s, opt_s, feats, warmup=2)
        losses_s.append([single().clone() for _ in range(5)])

    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29531')
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    torch.cuda.set_device(0)
    dist.init_process_group(backend='nccl', rank=0, world_size=1)
    try:
        probe = torch.arange(8, dtype=torch.float32, device=DEV)
        dist.all_reduce(probe)                                   # RCCL communicator creation + one real collective
        assert torch.equal(probe, torch.arange(8, dtype=torch.float32, device=DEV))
        losses_m = []
        for feats in batches:
            model_m, opt_m = fresh(exchange_always=True)
            multi = graphs.GraphedTrainStep(model_m, opt_m, feats, warmup=2)
            assert multi._multi, 'the multi-rank path was not taken'
            losses_m.append([multi().clone() for _ in range(5)])
        torch.cuda.synchronize()
        mode = multi.exchange_mode
        feats = batches[0]
        # two steps per graph launch on the multi-rank path (bench.py's form when the exchange is captured): 2 + 2 x 2 steps against the
        # first 6 of the single-rank run above; with an eager exchange the object falls back to one step per replay
        model_k, opt_k = fresh(exchange_always=True)
        losses_k = []
        multi_k = graphs.GraphedTrainStep(model_k, opt_k, feats, warmup=2, steps_per_replay=2)
        assert multi_k.steps_per_replay == (1 if mode == 'eager' else 2)     # an eager exchange sits between graph launches
        for _ in range(4 // multi_k.steps_per_replay):
            multi_k()
            losses_k += [v.clone() for v in multi_k.losses]
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert [v.item() for v in losses_k] == [v.item() for v in losses_s[0][:4]]
    assert mode in ('captured', 'eager')
    for got, want in zip(losses_m, losses_s):
        assert [v.item() for v in got] == [v.item() for v in want]
    for key in ('param', 'exp_avg', 'exp_avg_sq'):               # the C2 batch's optimisers (the last of each loop)
        assert torch.equal(opt_m.flat_buffers()[key], opt_s.flat_buffers()[key]), key
    print('RCCL world-1 graphed step: exchange mode = %s' % mode)


@pytest.mark.parametrize('precision,form,ragged,which', [('fp32', 'eager', True, 'f0'), ('fp32', 'graph', False, 'f0'), ('bf16', 'graph', True, 'f0'),
                                                         ('bf16x3', 'graph', False, 'f0'),
                                                         ('bf16', 'eager', True, 'rnn187'), ('fp32', 'eager', True, 'rnn187'),
                                                         ('bf16', 'eager', True, 'lstm')])
def test_two_ranks_on_one_gpu_equal_the_global_batch(tmp_path, precision, form, ragged, which):
    """The N > 1 leg of C3 / C5 with device tensors: two ranks share the box's one GPU (gloo process group - RCCL refuses two ranks on
    one device), each runs the PRODUCT step on its contiguous shard of 16 utterances (HIP kernels, flat fp32 gradient bucket on the
    device, the eager all-reduce of optim.Adam / GraphedTrainStep between the backward graph and the update kernel, 1 / world folded
    into the update) and must reproduce the one-rank run on the global batch: replicas bit-identical to each other, parameters and
    losses equal to the single run up to the order of the fp32 sums (L = mean_r L_r for equal shard sizes).
    ``which``: the README F0Model; 'rnn187' = BASELINE config C5's model (RNN_SPSS GRU-512, 187 outputs, ragged shards) and 'lstm' = the
    shipped LSTM acoustic model - the recurrent layers' DIRECT gradients (GRUFn / LSTMStackPersistFn add into the flat bucket inside
    functional.backward) meet the exchange here (/root/reference/morgana/losses.py:37-42)."""
    import subprocess
    import sys
    import _dist_gpu_worker as worker
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rendezvous = 'file://' + str(tmp_path / 'rendezvous')   # a file the ranks meet at: no port to lose to another process before they start
    out = str(tmp_path / 'dp_gpu.npz')
    n_steps = 4
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MG_TEST_RENDEZVOUS=rendezvous,
                   OMP_NUM_THREADS='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
        log = open(str(tmp_path / ('rank%d.log' % rank)), 'w')
        procs.append((subprocess.Popen([sys.executable, os.path.join(repo, 'tests', '_dist_gpu_worker.py'), out, str(n_steps), precision, form,
                                        '1' if ragged else '0', which], env=env, cwd=repo, stdout=log, stderr=subprocess.STDOUT), log))
    codes = []
    for p, log in procs:
        codes.append(p.wait(timeout=600))
        log.close()
    # a rank that died says why (one failure of this test in round 5 left no trace: the workers' output went to the terminal)
    assert codes == [0, 0], '\n'.join('--- rank %d (exit %s)\n%s' % (r, codes[r], open(str(tmp_path / ('rank%d.log' % r))).read()[-3000:])
                                      for r in range(2))
    got = np.load(out)
    assert np.array_equal(got['replicas'][0], got['replicas'][1])            # the ranks hold identical parameters after every update
    assert str(got['mode']) == ('eager' if form == 'graph' else 'eager loop')  # gloo is never captured into the graph
    batch = worker.global_batch(which, ragged)
    want_flat, want_losses, _ = worker.run_steps(batch, n_steps, precision, form, torch.device(DEV), which)
    # the exact modes to 1e-4 (F0Model) / 1e-3 (the recurrent model: BPTT sums in another order per shard), bf16 to 2e-3 / 5e-3
    tol = {'fp32': RTOL, 'bf16x3': RTOL}.get(precision, 2e-3) * (1.0 if which == 'f0' else (10.0 if precision == 'fp32' else 2.5))
    err = rel_l2(got['replicas'][0], want_flat.cpu().numpy())
    assert err < tol, (err, tol, got['losses'], want_losses)
    np.testing.assert_allclose(got['losses'], want_losses, rtol=tol)


@pytest.mark.parametrize('ragged', [False, True])
def test_recurrence_output_shadow_equals_the_cast_pass(ragged, monkeypatch):
    """utils.OUT_SHADOW (default on): the persistent GRU forward writes the bf16 copy of its output itself
    (mg_gru_fwd_persist_out_bf16) and the Linear run behind the wrapper takes it as its operand instead of casting [B, T, H] in a
    pass of its own.  The copy is bf16(out) element for element, so the loss, the prediction and every gradient are EQUAL."""
    feats = synthetic.make_batch(16, (150, 400) if ragged else 300, out_dim=80, target_name='mcep', seed=11)
    state = synthetic.rnn_spss_state()
    results = []
    for shadow in (True, False):
        monkeypatch.setattr(utils, 'OUT_SHADOW', shadow)
        model = _load_state(models.RNNSPSS(precision='bf16').to(DEV), state)
        loss, out = model(data.to_device(feats, DEV))
        loss.backward()
        ops.check_persistent_status()
        results.append((loss.detach().clone(), out['pred_norm_mcep'].detach().clone(),
                        {n: p.grad.detach().clone() for n, p in model.named_parameters()}))
    (loss_s, pred_s, grads_s), (loss_c, pred_c, grads_c) = results
    assert torch.equal(loss_s, loss_c) and torch.equal(pred_s, pred_c)
    for name in grads_c:
        assert torch.equal(grads_s[name], grads_c[name]), name


@pytest.mark.parametrize('which', ['rnn_spss', 'rnn_spss_ragged', 'lstm'])
def test_direct_gradients_equal_autograd_accumulation(which):
    """Inside functional.backward the row-wise, GRU and LSTM-stack layers outside the fused stack add their weight gradients and bias
    sums straight into morgana_amd.optim.Adam's flat gradient and hand autograd None (functional._direct_params; weight operands from
    the parameters' shadows) - against a plain ``loss.backward()`` on a twin model, where autograd accumulates returned tensors:
    the same kernels on the same data, every parameter's gradient EQUAL bit for bit, and so are the parameters after an update."""
    if which == 'lstm':
        feats = data.to_device(synthetic.make_acoustic_batch(64, 120, seed=11, with_raw=True), DEV)
        make = lambda: _load_state(models.LSTMAcousticModel(precision='bf16', generate=False).to(DEV), synthetic.lstm_acoustic_state())
    else:
        frames = (60, 150) if which == 'rnn_spss_ragged' else 120
        feats = data.to_device(synthetic.make_batch(64, frames, out_dim=80, target_name='mcep', seed=11), DEV)
        make = lambda: _load_state(models.RNNSPSS(precision='bf16').to(DEV), synthetic.rnn_spss_state())
    grads, params = {}, {}
    for mode in ('autograd', 'direct'):
        model = make()
        if which == 'lstm':
            synthetic.acoustic_normalisers(model, device=DEV)
            model.mode = 'train'
            model.metrics.reset_state('train')
        opt = optim.Adam(model.parameters(), lr=0.01)
        for _ in range(2):                                            # the second step runs on shadows the update kernel refreshed
            opt.zero_grad()
            loss, _ = model(feats)
            if mode == 'direct':
                F_hip.backward(loss)
            else:
                loss.backward()
            g = opt.flat_buffers()['grad'].clone()
            opt.step()
        ops.check_persistent_status()
        grads[mode], params[mode] = g, opt.flat_buffers()['param'].clone()
    assert torch.equal(grads['direct'], grads['autograd'])
    assert torch.equal(params['direct'], params['autograd'])


# ------------------------------------------------------------------------------------------------------------ contracts
@pytest.mark.parametrize('b,t,hid,form', [(16, 50, 512, 'step_bf16'), (16, 50, 512, 'persist_bf16'), (16, 50, 512, 'step_f32'),
                                          (16, 50, 256, 'persist_f32'), (12, 40, 64, 'small_f32'), (12, 40, 128, 'small_f32')])
def test_gru_backward_never_reads_saved_past_seq_len(b, t, hid, form):
    """Contract of include/morgana_hip.h (K3): ``saved[b, t, :]`` for t >= seq_len[b] is unspecified - the forward kernels differ in
    what they leave there - and no backward entry point lets it reach a result.  Poison exactly those elements (and the matching
    ``grad_out`` rows, which the reference's pad_packed_sequence backward drops as well) with NaN: every gradient must come out
    bit-identical to the unpoisoned run, and finite."""
    rng = np.random.RandomState(hid + t)
    xproj = dev(rng.standard_normal((b, t, 3 * hid)).astype(np.float32))
    w_hh = dev((rng.uniform(-1, 1, (3 * hid, hid)) / np.sqrt(hid)).astype(np.float32))
    b_hh = dev(rng.uniform(-0.1, 0.1, 3 * hid).astype(np.float32))
    sl_np = rng.randint(1, t + 1, size=b).astype(np.int64)
    sl_np[0], sl_np[-1] = t, 1
    sl = dev(sl_np)
    out, hs, sv = ops.gru_fwd(xproj, w_hh, b_hh, sl, None, b, t, hid)
    g_out = dev(rng.standard_normal((b, t, hid)).astype(np.float32))
    g_hn = dev(rng.standard_normal((b, hid)).astype(np.float32))
    past = dev((np.arange(t)[None, :] >= sl_np[:, None])[:, :, None])
    nan = torch.full((), float('nan'), device=DEV)
    sv_bad, g_bad = torch.where(past, nan, sv), torch.where(past, nan, g_out)

    def run(saved, grad):
        if form == 'step_bf16':
            return ops.gru_bwd_bf16(grad, g_hn, hs, saved, w_hh, sl, b, t, hid, persistent=False)
        if form == 'persist_bf16':
            assert ops.gru_persist_ok(b, t, hid)
            return ops.gru_bwd_bf16(grad, g_hn, hs, saved, w_hh, sl, b, t, hid, persistent=True)
        if form == 'persist_f32':
            assert ops.gru_persist_f32_ok(b, t, hid)
            return ops.gru_bwd(grad, g_hn, hs, saved, w_hh, sl, b, t, hid)
        if form == 'step_f32':
            return ops.gru_bwd(grad, g_hn, hs, saved, w_hh, sl, b, t, hid, persistent=False)
        return ops.gru_bwd(grad, g_hn, hs, saved, w_hh, sl, b, t, hid)

    clean, dirty = run(sv, g_out), run(sv_bad, g_bad)
    for got, want in zip(dirty, clean):
        assert torch.isfinite(got.float()).all()
        assert torch.equal(got, want)


def test_unsupported_recurrent_layers_raise():
    """No torch / MIOpen fallback: layer types without a HIP recurrence raise MorganaHipError."""
    x = torch.zeros(2, 5, 16, device=DEV)
    sl = torch.tensor([5, 3], device=DEV)
    for layer in (nn.GRU(16, 8), nn.LSTM(16, 8, batch_first=True, proj_size=4), nn.GRU(16, 8, batch_first=True, bias=False),
                  nn.RNN(16, 8, batch_first=True)):
        with pytest.raises(_lib.MorganaHipError, match='no HIP recurrence'):
            utils.RecurrentCuDNNWrapper(layer.to(DEV))(x, None, sl)


@pytest.mark.parametrize('kind,num_layers,bidirectional,hid', [('gru', 2, False, 128), ('gru', 1, True, 128), ('gru', 2, True, 64), ('lstm', 1, True, 128),
                                                             ('lstm', 2, True, 64)])
def test_multi_layer_and_bidirectional_wrappers_vs_torch(kind, num_layers, bidirectional, hid):
    """The reference's wrapper takes any nn.RNNBase (/root/reference/morgana/utils.py:333-343): multi-layer and bidirectional nn.GRU /
    nn.LSTM run layer by layer and direction by direction on the single-layer HIP recurrences (RecurrentCuDNNWrapper._run_general; the
    backward direction on every item's frames reversed within its own length).  fp32 mode against torch's CPU layer behind
    pack_padded_sequence / pad_packed_sequence - the reference's own call sequence (utils.py:366-385): outputs, final states and every
    gradient to 1e-4 of the largest element; ragged lengths, initial states given."""
    rng = np.random.RandomState(11)
    b, t, f = 5, 17, 24
    make = nn.GRU if kind == 'gru' else nn.LSTM
    torch.manual_seed(7)
    ref = make(f, hid, num_layers=num_layers, batch_first=True, bidirectional=bidirectional)
    own = make(f, hid, num_layers=num_layers, batch_first=True, bidirectional=bidirectional).to(DEV)
    own.load_state_dict(ref.state_dict())
    x_np = rng.standard_normal((b, t, f)).astype(np.float32)
    lens = np.array([17, 9, 1, 12, 17], dtype=np.int64)
    for i, n in enumerate(lens):
        x_np[i, n:] = 0.0
    n_state = num_layers * (2 if bidirectional else 1)
    h0_np = (rng.standard_normal((n_state, b, hid)) * 0.3).astype(np.float32)
    c0_np = (rng.standard_normal((n_state, b, hid)) * 0.3).astype(np.float32)
    g_np = rng.standard_normal((b, t, hid * (2 if bidirectional else 1))).astype(np.float32)

    # the reference's call sequence on CPU
    x_r = torch.from_numpy(x_np).requires_grad_(True)
    hid_r = (torch.from_numpy(h0_np), torch.from_numpy(c0_np)) if kind == 'lstm' else torch.from_numpy(h0_np)
    packed = nn.utils.rnn.pack_padded_sequence(x_r, torch.from_numpy(lens), batch_first=True, enforce_sorted=False)
    out_p, hn_r = ref(packed, hid_r)
    out_r, _ = nn.utils.rnn.pad_packed_sequence(out_p, batch_first=True, total_length=t)
    (out_r * torch.from_numpy(g_np)).sum().backward()

    wrapper = utils.RecurrentCuDNNWrapper(own, precision='fp32')
    x_o = dev(x_np).requires_grad_(True)
    hid_o = (dev(h0_np), dev(c0_np)) if kind == 'lstm' else dev(h0_np)
    out_o, hn_o = wrapper(x_o, hid_o, dev(lens))
    (out_o * dev(g_np)).sum().backward()
    assert rel_err(out_o.detach().cpu().numpy(), out_r.detach().numpy(), 'output') < RTOL
    for got, want in zip(hn_o if kind == 'lstm' else (hn_o,), hn_r if kind == 'lstm' else (hn_r,)):
        assert rel_err(got.detach().cpu().numpy(), want.detach().numpy(), 'final state') < RTOL
    assert rel_err(x_o.grad.cpu().numpy(), x_r.grad.numpy(), 'input gradient') < RTOL
    for (name, p_o), (_, p_r) in zip(own.named_parameters(), ref.named_parameters()):
        assert rel_err(p_o.grad.cpu().numpy(), p_r.grad.numpy(), name) < RTOL, name


def test_wrapper_accepts_packed_sequences():
    """``seq_len=None`` with an already packed input (morgana/utils.py:347-349) runs the HIP recurrence and returns a packed
    result equal to the padded call's."""
    rng = np.random.RandomState(4)
    gru = nn.GRU(12, 128, batch_first=True).to(DEV)
    wrapper = utils.RecurrentCuDNNWrapper(gru, precision='fp32')
    x = dev(rng.standard_normal((4, 9, 12)).astype(np.float32))
    sl = torch.tensor([6, 9, 1, 4], device=DEV)
    want, want_h = wrapper(x, None, sl)
    packed = nn.utils.rnn.pack_padded_sequence(x, sl.cpu(), batch_first=True, enforce_sorted=False)
    got, got_h = wrapper(packed)
    assert isinstance(got, nn.utils.rnn.PackedSequence)
    got_padded, lens = nn.utils.rnn.pad_packed_sequence(got, batch_first=True)
    assert torch.equal(lens, sl.cpu()) and torch.equal(got_padded, want) and torch.equal(got_h, want_h)


# ------------------------------------------------------------------------------------------------------------ fused update
@pytest.mark.parametrize('n_slabs,aligned', [(48, True), (96, True), (5, False), (1, False)])
def test_adam_plan_kernel_equals_reduce_then_adam(n_slabs, aligned):
    """mg_adam_step_plan_f32 (split-M slabs summed inside the update, bf16 operand copies refreshed, gradient zeroed behind the read)
    against the separate launches it replaces - slab reduce (mg_linear_wgrad_bf16's) into the gradient, mg_adam_step_dev_f32, a cast:
    parameters, both moments and the bf16 copies EQUAL bit for bit; the gradient buffer is zero afterwards.  Ranges that are not
    16-byte aligned take the element-wise path."""
    rng = np.random.RandomState(n_slabs)
    rows, cols = 24, 40
    n_mat = rows * cols
    begin = 64 if aligned else 37
    count = n_mat + rows if aligned else n_mat + rows - 3
    n = begin + count + 29
    stride = count + (0 if aligned else 1)
    param = dev(rng.standard_normal(n).astype(np.float32))
    grad = dev(rng.standard_normal(n).astype(np.float32) * 0.1)
    m0 = dev(rng.standard_normal(n).astype(np.float32) * 0.01)
    v0 = dev(np.abs(rng.standard_normal(n)).astype(np.float32) * 0.01)
    slabs = dev(rng.standard_normal((n_slabs, stride)).astype(np.float32) * 0.05)
    scalars = torch.tensor(ops.adam_scalars(0.01, (0.9, 0.999), 3), dtype=torch.float32, device=DEV)
    # reference: the slab reduce's order (16 interleaved partitions, ascending, then ascending over partitions) on the host in fp32
    want_grad = grad.clone()
    acc = want_grad[begin:begin + count].clone()
    parts = []
    for p in range(min(16, n_slabs)):
        t = torch.zeros(count, device=DEV)
        for s in range(p, n_slabs, 16):
            t = t + slabs[s, :count]
        parts.append(t)
    for t in parts:
        acc = acc + t
    want_grad[begin:begin + count] = acc
    p_ref, m_ref, v_ref = param.clone(), m0.clone(), v0.clone()
    ops.adam_step_dev(p_ref, want_grad, m_ref, v_ref, (0.9, 0.999), 1e-8, 0.01, scalars, 0.5)
    plain = torch.zeros((rows, 64), dtype=torch.bfloat16, device=DEV)
    trans = torch.zeros((cols, 64), dtype=torch.bfloat16, device=DEV)
    p_got, g_got, m_got, v_got = param.clone(), grad.clone(), m0.clone(), v0.clone()
    ops.adam_step_plan(p_got, g_got, m_got, v_got, (0.9, 0.999), 1e-8, 0.01, scalars, 0.5,
                       slab_srcs=[(begin, count, slabs, n_slabs, stride)], shadows=[(begin, rows, cols, plain, trans)], clear_grad=True)
    assert torch.equal(p_got, p_ref) and torch.equal(m_got, m_ref) and torch.equal(v_got, v_ref)
    assert torch.count_nonzero(g_got) == 0
    w = p_ref[begin:begin + n_mat].view(rows, cols)
    assert torch.equal(plain[:, :cols], w.to(torch.bfloat16)) and torch.count_nonzero(plain[:, cols:]) == 0
    assert torch.equal(trans[:, :rows], w.t().to(torch.bfloat16)) and torch.count_nonzero(trans[:, rows:]) == 0
    with pytest.raises(ValueError):
        ops.adam_step_plan(p_got, g_got, m_got, v_got, (0.9, 0.999), 1e-8, 0.0, scalars, 1.0, slab_srcs=[(n - 4, 16, slabs, 1, stride)])


def test_fused_loop_step_equals_plain_loop():
    """The reference's loop body with ``optim.Adam(fused_loop=True)`` (weight-gradient slabs left to the update kernel, bf16 weight copies
    refreshed by it, zero_grad free, the loader's bf16 phone table) against the same loop with the default optimiser (every gradient
    reduced into .grad by the backward pass, weights re-cast per step, memset per step, table cast per step): losses, parameters and
    moments EQUAL bit for bit over several steps, at the phone-rate and at the frame-rate order of operations."""
    for phone_rate in (True, False):
        results = []
        for fused in (False, True):
            ops.PHONE_RATE = phone_rate
            try:
                feats = data.to_device(synthetic.make_batch(48, (200, 240), seed=4, frames_per_phone=5.0), DEV)
                if fused:
                    data.add_bf16_table(feats)
                model = _load_state(models.F0Model(precision='bf16').to(DEV), synthetic.f0_model_state())
                opt = optim.Adam(model.parameters(), lr=0.01, fused_loop=fused)
                losses = []
                for _ in range(5):
                    opt.zero_grad()
                    loss, _ = model(feats)
                    F_hip.backward(loss)
                    opt.step()
                    losses.append(loss.item())
            finally:
                ops.PHONE_RATE = True
            flat = opt.flat_buffers()
            results.append((losses, flat['param'].clone(), flat['exp_avg'].clone(), flat['exp_avg_sq'].clone()))
        (l0, p0, m0, v0), (l1, p1, m1, v1) = results
        assert l0 == l1, phone_rate
        assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1), phone_rate


# ------------------------------------------------------------------------------------------------------------ fp32 persistent LSTM
@pytest.mark.parametrize('b,t,hid', [(16, 50, 512), (33, 23, 256), (5, 70, 384), (128, 9, 320), (1, 1, 512)])
@pytest.mark.parametrize('handoff', [0, 1])
def test_lstm_persistent_fp32_equals_step_kernels(b, t, hid, handoff):
    """mg_lstm_fwd_persist_f32 / mg_lstm_bwd_persist_f32 (one launch per direction, W_hh resident in registers, fp32 hand-off tiles
    between workgroups) against the launch-per-step kernels mg_lstm_fwd_f32 / mg_lstm_bwd_f32, which share their block order and
    cell code (csrc/lstm_cell.h): outputs, both states, gate gradients, dh0 / dc0 EQUAL bit for bit on ragged batches with an
    initial state, gradients on outputs and on the final states, in the same-XCD and in the forced write-through hand-off form;
    saved gates compared on the live steps (past an item's length they are unspecified by contract)."""
    lib = _lib.load()
    rng = np.random.RandomState(hid + b + t)
    xproj = dev(rng.standard_normal((b, t, 4 * hid)).astype(np.float32))
    w_hh = dev((rng.uniform(-1, 1, (4 * hid, hid)) / np.sqrt(hid)).astype(np.float32))
    b_hh = dev(rng.uniform(-0.1, 0.1, 4 * hid).astype(np.float32))
    h0 = dev(rng.standard_normal((b, hid)).astype(np.float32) * 0.5)
    c0 = dev(rng.standard_normal((b, hid)).astype(np.float32) * 0.5)
    sl_np = rng.randint(1, t + 1, size=b).astype(np.int64)
    sl_np[0] = t
    if b > 2:
        sl_np[-1] = 1
    sl = dev(sl_np)
    assert ops.lstm_persist_f32_ok(b, t, hid)
    lib.mg_set_tuning(2, handoff)
    try:
        out_s, hs_s, cs_s, sv_s = ops.lstm_fwd(xproj, w_hh, b_hh, sl, h0, c0, b, t, hid, persistent=False)
        out_p, hs_p, cs_p, sv_p = ops.lstm_fwd(xproj, w_hh, b_hh, sl, h0, c0, b, t, hid, persistent=True)
        assert torch.equal(out_p, out_s) and torch.equal(hs_p, hs_s) and torch.equal(cs_p, cs_s)
        valid = dev((np.arange(t)[None, :] < sl_np[:, None])[:, :, None])
        zero = torch.zeros((), device=DEV)
        assert torch.equal(torch.where(valid, sv_p, zero), torch.where(valid, sv_s, zero))
        g_out = dev(rng.standard_normal((b, t, hid)).astype(np.float32))
        g_hn = dev(rng.standard_normal((b, hid)).astype(np.float32))
        g_cn = dev(rng.standard_normal((b, hid)).astype(np.float32))
        # the contract's other half: gate values and output gradients past an item's length never reach a result
        nan = torch.full((), float('nan'), device=DEV)
        sv_bad, g_bad = torch.where(valid, sv_s, nan), torch.where(valid, g_out, nan)
        dg_s, dh_s, dc_s = ops.lstm_bwd(g_out, g_hn, g_cn, cs_s, sv_s, w_hh, sl, b, t, hid, persistent=False)
        dg_p, dh_p, dc_p = ops.lstm_bwd(g_bad, g_hn, g_cn, cs_s, sv_bad, w_hh, sl, b, t, hid, persistent=True)
        dg_q, dh_q, dc_q = ops.lstm_bwd(g_bad, g_hn, g_cn, cs_s, sv_bad, w_hh, sl, b, t, hid, persistent=False)
    finally:
        lib.mg_set_tuning(2, 0)
    for got in ((dg_p, dh_p, dc_p), (dg_q, dh_q, dc_q)):
        for g, w in zip(got, (dg_s, dh_s, dc_s)):
            assert torch.isfinite(g).all() and torch.equal(g, w)


def test_lstm_fp32_model_runs_on_persistent_recurrence_vs_oracle():
    """Two stacked LSTM-512 wrappers in fp32 parity mode now run layer by layer on the persistent recurrence (functional.lstm_layerwise)
    instead of the time-skewed stack of per-step launches: against the numpy oracle at the north star's 1e-4."""
    rng = np.random.RandomState(3)
    b, t, hid = 6, 40, 512
    lstm = nn.LSTM(64, hid, num_layers=2, batch_first=True).to(DEV)
    x_np = rng.standard_normal((b, t, 64)).astype(np.float32)
    sl_np = np.array([40, 13, 27, 1, 40, 33], dtype=np.int64)
    assert F_hip.lstm_layerwise('fp32', b, t, hid)
    params = [[getattr(lstm, '%s_l%d' % (n, k)).detach().cpu().numpy() for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')] for k in range(2)]
    want = x_np
    for k in range(2):
        want, hn, cn, _ = ref_cpu.lstm_forward(want, sl_np, *params[k])
    out, (h, c) = utils.RecurrentCuDNNWrapper(lstm, precision='fp32')(dev(x_np), None, dev(sl_np))
    assert rel_err(out.detach().cpu().numpy(), want) < RTOL
    assert rel_err(h[1].detach().cpu().numpy(), hn[0]) < RTOL and rel_err(c[1].detach().cpu().numpy(), cn[0]) < RTOL


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The LSTM stack's backward as one wavefront launch (csrc/lstm_persist.hip, mg_lstm_pstack_bwd_bf16)
@pytest.mark.gpu
@pytest.mark.parametrize('b,t,i_dim,hid,n_layers', [(64, 70, 512, 512, 8), (64, 40, 96, 512, 3), (20, 30, 24, 128, 3), (9, 33, 40, 128, 2),
                                                    (40, 25, 64, 384, 4)])
def test_lstm_stack_backward_wavefront_vs_layer_by_layer(b, t, i_dim, hid, n_layers):
    """The same forward (one wavefront launch), then the backward twice: as ONE wavefront launch over (layer, time) with the gradient a
    layer hands to the layer below computed inside the step, and layer by layer (one persistent launch + the input-gradient GEMM per
    layer).  bf16 operands and fp32 accumulation in both; the in-step products are summed in a different order than the GEMM's, so the
    gradients agree to 5e-3 relative (measured ~1e-3), not bit for bit.  Ragged lengths with a full and a 1-step item, gradients on
    the outputs and on every layer's final states, initial states given.  Both slot widths (32 units: one workgroup per CU, 16: two)
    and both hand-off forms must give identical bits, run after run."""
    assert ops.lstm_pstack_bwd_ok(b, t, hid, n_layers)
    torch.manual_seed(3 * hid + n_layers)
    x = torch.randn(b, t, i_dim, device=DEV, requires_grad=True)
    sl_np = np.random.RandomState(b + t).randint(1, t + 1, size=b).astype(np.int64)
    sl_np[0], sl_np[-1] = t, 1
    seq_len = dev(sl_np)
    params = []
    for l in range(n_layers):
        k = i_dim if l == 0 else hid
        params += [torch.randn(4 * hid, k, device=DEV) / k ** 0.5, torch.randn(4 * hid, hid, device=DEV) / hid ** 0.5,
                   torch.randn(4 * hid, device=DEV) * 0.1, torch.randn(4 * hid, device=DEV) * 0.1]
    params = [p.requires_grad_(True) for p in params]
    h0s = (torch.randn(n_layers, b, hid, device=DEV) * 0.5).requires_grad_(True)
    c0s = (torch.randn(n_layers, b, hid, device=DEV) * 0.5).requires_grad_(True)
    g_out = torch.randn(b, t, hid, device=DEV)
    g_hn, g_cn = torch.randn(n_layers, b, hid, device=DEV), torch.randn(n_layers, b, hid, device=DEV)
    leaves = [x, h0s, c0s] + params

    def run(stack_backward):
        for p in leaves:
            p.grad = None
        F_hip.LSTM_STACK_BACKWARD = stack_backward
        try:
            out, hn, cn = F_hip.LSTMStackPersistFn.apply(x, seq_len, h0s, c0s, *params)
            ((out * g_out).sum() + (hn * g_hn).sum() + (cn * g_cn).sum()).backward()
        finally:
            F_hip.LSTM_STACK_BACKWARD = True
        ops.check_persistent_status()
        return [p.grad.detach().cpu().numpy().copy() for p in leaves]

    want = run(False)
    lib = _lib.load()
    first = None
    try:
        for width, handoff in ((0, 0), (1, 0), (0, 1), (0, 0)):
            lib.mg_set_tuning(6, width)
            lib.mg_set_tuning(2, handoff)
            got = run(True)
            if first is None:
                first = got
                for k, (g, w) in enumerate(zip(got, want)):
                    assert np.all(np.isfinite(g)), k
                    assert rel_err(g, w) < 5e-3, (k, rel_err(g, w))
            else:
                for k, (g, w) in enumerate(zip(got, first)):
                    np.testing.assert_array_equal(g, w, err_msg='gradient %d, slot width %d, hand-off %d' % (k, width, handoff))
    finally:
        lib.mg_set_tuning(6, 0)
        lib.mg_set_tuning(2, 0)


@pytest.mark.gpu
def test_lstm_stack_backward_gate_gradients_and_fp32_copy():
    """ops.lstm_pstack_bwd itself: per layer the bf16 gate gradients against ops.lstm_bwd_bf16 fed with the gradient the layer above hands
    down (its gate gradients through W_ih), the optional fp32 copy rounds to the bf16 shadow, padded steps are exactly zero, no
    final-state gradients (NULL pointers), groups whose items are all shorter than T, and NaN in `saved` / `grad_out` past an item's
    length reaching nothing."""
    b, t, hid, n_layers = 24, 21, 256, 3
    assert ops.lstm_pstack_bwd_ok(b, t, hid, n_layers)
    torch.manual_seed(11)
    sl_np = np.random.RandomState(5).randint(1, t - 2, size=b).astype(np.int64)
    sl_np[3] = t
    seq_len = dev(sl_np)
    w_ih = [torch.randn(4 * hid, hid, device=DEV) / hid ** 0.5 for _ in range(n_layers)]
    w_hh = [torch.randn(4 * hid, hid, device=DEV) / hid ** 0.5 for _ in range(n_layers)]
    b_ih = [torch.randn(4 * hid, device=DEV) * 0.1 for _ in range(n_layers)]
    b_hh = [torch.randn(4 * hid, device=DEV) * 0.1 for _ in range(n_layers)]
    xproj0 = torch.randn(b, t, 4 * hid, device=DEV)
    _, _, cstate, saved, _ = ops.lstm_pstack_fwd(xproj0, w_ih, w_hh, b_ih, b_hh, seq_len, None, None, b, t, hid)
    g_out = torch.randn(b, t, hid, device=DEV)
    dgates, dgates_bf, dh0, dc0 = ops.lstm_pstack_bwd(g_out, None, None, cstate, saved, w_ih, w_hh, seq_len, b, t, hid, want_f32=True)
    ops.check_persistent_status()
    m = b * t
    g = g_out
    for l in range(n_layers - 1, -1, -1):
        _, dh0_l, dc0_l, want_bf = ops.lstm_bwd_bf16(g, None, None, cstate[l], saved[l], w_hh[l], seq_len, b, t, hid, want_f32=False)
        got, want = dgates_bf[l].float().cpu().numpy(), want_bf.float().cpu().numpy()
        assert rel_err(got, want) < 1e-2, (l, rel_err(got, want))
        assert rel_err(dh0[l].cpu().numpy(), dh0_l.cpu().numpy()) < 1e-2 and rel_err(dc0[l].cpu().numpy(), dc0_l.cpu().numpy()) < 1e-2
        np.testing.assert_array_equal(dgates[l].to(torch.bfloat16).float().cpu().numpy(), got)
        for i, n in enumerate(sl_np):
            assert np.all(got[i, n:] == 0)
        if l > 0:
            # what the layer hands down, from the WAVEFRONT's gate gradients (so that errors do not compound over the layers)
            g = ops.linear_dgrad_bf16(dgates_bf[l].view(m, 4 * hid), m, 4 * hid, ops.cast_transpose_bf16(w_ih[l]), hid, None,
                                      out_f32=True)[:, :hid].contiguous().view(b, t, hid)
    # the contract of include/morgana_hip.h: saved[b, t, :] past an item's length is unspecified and must not reach any result
    past = (torch.arange(t, device=DEV)[None, :] >= seq_len[:, None])[:, :, None]
    nan = torch.full((), float('nan'), device=DEV)
    bad = [torch.where(past, nan, s) for s in saved]
    _, dgates_bf2, dh02, dc02 = ops.lstm_pstack_bwd(torch.where(past, nan, g_out), None, None, cstate, bad, w_ih, w_hh, seq_len, b, t, hid)
    ops.check_persistent_status()
    for l in range(n_layers):
        assert torch.equal(dgates_bf2[l], dgates_bf[l]), l
    assert torch.equal(dh02, dh0) and torch.equal(dc02, dc0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The stack of small GRU layers as one wavefront launch per direction (csrc/gru_small_stack.hip)
@pytest.mark.gpu
@pytest.mark.parametrize('b,t,i_dim,n_layers,precision', [(64, 120, 256, 3, 'fp32'), (13, 57, 40, 2, 'fp32'), (5, 1, 24, 3, 'fp32'),
                                                         (30, 64, 96, 4, 'fp32'), (64, 90, 256, 3, 'bf16')])
def test_gru_small_stack_wavefront_vs_chained_layers(b, t, i_dim, n_layers, precision):
    """functional.GRUStackSmallFn (the GRU-64 layers of models/f0_test_model.py:31-37 as ONE launch per direction: a wavefront over layer
    and time, the upper layers' input projections and the gradients between the layers computed inside the step) against the same
    layers chained through functional.GRUFn.  fp32 mode: exact fp32 on both sides, only the summation order of those in-step products
    differs - 1e-4 relative on outputs, final states and every gradient (measured ~1e-6).  bf16 mode: the chain rounds the upper
    layers' inputs and gate gradients to bf16 for its GEMMs, the wavefront keeps them in fp32 - 2e-2.  Ragged lengths with a full and
    a 1-step item, gradients on outputs and final states; odd and even T, T = 1; run twice: identical bits."""
    hid = 64
    assert F_hip.gru_stack_small(b, t, hid, n_layers)
    torch.manual_seed(7 * b + n_layers)
    x = torch.randn(b, t, i_dim, device=DEV, requires_grad=True)
    sl_np = np.random.RandomState(b + t).randint(1, t + 1, size=b).astype(np.int64)
    sl_np[0], sl_np[-1] = t, 1
    seq_len = dev(sl_np)
    params = []
    for l in range(n_layers):
        k = i_dim if l == 0 else hid
        params += [torch.randn(3 * hid, k, device=DEV) / k ** 0.5, torch.randn(3 * hid, hid, device=DEV) / hid ** 0.5,
                   torch.randn(3 * hid, device=DEV) * 0.1, torch.randn(3 * hid, device=DEV) * 0.1]
    params = [p.requires_grad_(True) for p in params]
    g_out = torch.randn(b, t, hid, device=DEV)
    g_hn = torch.randn(n_layers, b, hid, device=DEV)
    leaves = [x] + params

    def run(kind):
        for p in leaves:
            p.grad = None
        if kind == 'wavefront':
            out, hn = F_hip.GRUStackSmallFn.apply(precision, x, seq_len, None, *params)
        else:
            out, hns = x, []
            for l in range(n_layers):
                out, h = F_hip.GRUFn.apply(precision, out.contiguous(), None, seq_len, *params[4 * l:4 * l + 4])
                hns.append(h)
            hn = torch.cat(hns, 0)
        ((out * g_out).sum() + (hn * g_hn).sum()).backward()
        ops.check_persistent_status()
        return [v.detach().cpu().numpy().copy() for v in (out, hn, *[p.grad for p in leaves])]

    want = run('chain')
    got = run('wavefront')
    tol = 1e-4 if precision == 'fp32' else 2e-2
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.all(np.isfinite(g)), k
        assert rel_err(g, w) < tol, (k, rel_err(g, w))
    for i, n in enumerate(sl_np):
        assert np.all(got[0][i, n:] == 0)
    again = run('wavefront')
    for k, (g, w) in enumerate(zip(again, got)):
        np.testing.assert_array_equal(g, w, err_msg='output %d of the second run' % k)


@pytest.mark.gpu
def test_gru_f0_model_runs_on_the_stack_wavefront():
    """models.GRUF0Model (the shipped F0 model) takes the wavefront for its three GRU-64 wrappers: loss and every parameter gradient
    against the same model with the wavefront switched off (fp32 mode, 1e-4)."""
    torch.manual_seed(0)
    feats = data.to_device(synthetic.make_acoustic_batch(6, (60, 150), streams=(('lf0', 3, 'mse'),), seed=5), DEV)
    grads = {}
    try:
        for flag in (False, True):
            F_hip.GRU_STACK_WAVEFRONT = flag
            torch.manual_seed(1)
            model = models.GRUF0Model(precision='fp32', generate=False).to(DEV)
            loss, _ = model(feats)
            loss.backward()
            ops.check_persistent_status()
            grads[flag] = [float(loss.detach())] + [p.grad.detach().cpu().numpy().copy() for p in model.parameters()]
    finally:
        F_hip.GRU_STACK_WAVEFRONT = True
    assert abs(grads[True][0] - grads[False][0]) < 1e-5 * max(1.0, abs(grads[False][0]))
    for k, (g, w) in enumerate(zip(grads[True][1:], grads[False][1:])):
        assert rel_err(g, w) < 1e-4, (k, rel_err(g, w))


@pytest.mark.parametrize('which', ['gru_f0', 'lstm'])
def test_shipped_models_in_bf16x3_track_fp32(which):
    """The reference's two shipped models (models/f0_test_model.py, models/RNN_SPSS.py: 609-dim input with frame-level counters,
    recurrent stacks, multi-stream loss) in precision 'bf16x3' - split-bf16 row-wise layers, exact-fp32 recurrences - against fp32
    mode on a ragged batch: loss to 1e-4, every parameter gradient to 1e-3 of its largest element (fp32 mode's own bars vs the oracle)."""
    if which == 'gru_f0':
        feats_np = synthetic.make_acoustic_batch(6, (60, 150), streams=(('lf0', 3, 'mse'),), seed=5)
        make = lambda prec: models.GRUF0Model(precision=prec, generate=False)
    else:
        feats_np = synthetic.make_acoustic_batch(4, (40, 90), seed=6)
        make = lambda prec: models.LSTMAcousticModel(precision=prec, num_layers=2, generate=False)
    feats = data.to_device(feats_np, DEV)
    got = {}
    for prec in ('fp32', 'bf16x3'):
        torch.manual_seed(2)
        model = make(prec).to(DEV)
        loss, _ = model(feats)
        loss.backward()
        ops.check_persistent_status()
        got[prec] = (float(loss.detach()), {n: p.grad.detach().cpu().numpy().copy() for n, p in model.named_parameters()})
    np.testing.assert_allclose(got['bf16x3'][0], got['fp32'][0], rtol=RTOL)
    for name, want in got['fp32'][1].items():
        assert rel_err(got['bf16x3'][1][name], want) < 1e-3, name


def test_frame_layout_with_a_host_total_that_disagrees_with_the_lengths():
    """mg_frame_layout with a host-side frame total above / below what the device lengths (clipped to T) add up to: surplus packed
    rows must gather the zero row (-1), never whatever the allocation held (rows[sum .. total-1] were left
    uninitialised and used as gather indices); surplus frames count as padding."""
    seq = torch.tensor([5, 9, 3, 12], dtype=torch.int64, device=DEV)
    t = 8                                                  # clips 9 and 12: the device sum is 5 + 8 + 3 + 8 = 24
    for total in (24, 29, 20):
        rows = None
        for fill in (0x7fffffff, -7):                      # two poisons: whatever the allocator hands out must not show
            torch.full((total + 64,), fill, dtype=torch.int32, device=DEV)
            offsets, rows, inverse = ops.frame_layout(seq, t, total)
            r, inv, off = rows.cpu().numpy(), inverse.cpu().numpy().reshape(4, t), offsets.cpu().numpy()
            assert off.tolist() == [0, 5, 13, 16, 24]
            assert r[total] == -1
            valid = min(total, 24)
            want = [b * t + f for b in range(4) for f in range(min(int(seq[b]), t))][:valid]
            assert r[:valid].tolist() == want
            assert (r[valid:total] == -1).all(), (total, r[valid:total])
            for b in range(4):
                for f in range(t):
                    i = off[b] + f
                    assert inv[b, f] == (i if f < int(seq[b]) and i < total else total)


@pytest.mark.parametrize('n,act,out_f32', [(512, ops.ACT_SIGMOID, False), (256, ops.ACT_SIGMOID, True), (100, ops.ACT_NONE, False),
                                           (20, ops.ACT_NONE, True)])
def test_phone_concat_layer_kernel(n, act, out_f32):
    """mg_phone_concat_layer_bf16 (csrc/phone_rate.hip): act(P[rows] + counters W_cnt^T + b) with P = table W_lab^T at phone rate, against
    the same arithmetic in torch (bf16-rounded table and lab weights, fp32 counters and their weights, fp32 accumulation): fp32
    output to 1e-5 of the largest value, bf16 output to one bf16 step; padding columns zero; padding frames (row -1 -> the zero
    row behind the table) see the bias and their counters only."""
    rng = np.random.RandomState(n)
    r, k_lab, c, extra = 37, 600, 9, 5
    counts = rng.randint(1, 9, size=r)
    rows_np = np.concatenate([np.repeat(np.arange(r), counts), -np.ones(11)]).astype(np.int32)
    m = rows_np.size
    table = dev(rng.uniform(0, 1, (r, k_lab)).astype(np.float32))
    feat = dev(rng.uniform(0, 1, (m, c)).astype(np.float32))
    w = dev((rng.standard_normal((n, k_lab + c)) * 0.05).astype(np.float32))
    b = dev((rng.standard_normal(n) * 0.1).astype(np.float32))
    rows = torch.from_numpy(rows_np).to(DEV)
    seg, mapped = ops.segment_bounds(rows, r, pad_row=r)
    table_bf = ops.cast_pad_bf16(table, extra_rows=extra)
    w_bf = ops.cast_pad_bf16(w)
    got = ops.phone_concat_layer(table_bf, k_lab, mapped, feat, w, w_bf, b, n, act, out_f32=out_f32)
    assert got.dtype == (torch.float32 if out_f32 else torch.bfloat16)
    assert got.shape[1] == ((n + 7) // 8 * 8 if out_f32 else ops.pad8(n)) and not bool(got[:, n:].any())
    lab = torch.cat((table.to(torch.bfloat16).double(), torch.zeros((1, k_lab), dtype=torch.float64, device=DEV)))[mapped.long()]
    z = lab @ w[:, :k_lab].to(torch.bfloat16).double().t() + feat.double() @ w[:, k_lab:].double().t() + b.double()
    want = torch.sigmoid(z) if act == ops.ACT_SIGMOID else z
    err = float((got[:, :n].double() - want).abs().max() / want.abs().max())
    assert err < (1e-5 if out_f32 else 2.0 ** -8), err
    pad = rows_np < 0
    z_pad = feat.double()[torch.from_numpy(pad).to(DEV)] @ w[:, k_lab:].double().t() + b.double()
    want_pad = torch.sigmoid(z_pad) if act == ops.ACT_SIGMOID else z_pad
    assert float((got[torch.from_numpy(pad).to(DEV), :n].double() - want_pad).abs().max()) < (1e-5 if out_f32 else 2.0 ** -7)


@pytest.mark.parametrize('which', ['gru_f0', 'lstm'])
def test_first_layer_of_the_609_input_models_at_phone_rate(which, monkeypatch):
    """cat(upsampled labels, frame counters) -> Linear (models/RNN_SPSS.py:76-81, models/f0_test_model.py:78-79) in bf16 mode at both
    orders of operations: phone rate = the labels' 600 columns multiplied once per phone (mg_phone_concat_layer_bf16 adds the counters'
    9 columns per frame; backward: per-phone sums of the gradient), frame rate = one gather + concat pass and the 609-column GEMM per
    frame.  Same loss and gradients to bf16 tolerance, both tracking fp32 mode; also with active dropout behind the layer."""
    if which == 'gru_f0':
        feats_np = synthetic.make_acoustic_batch(16, (300, 400), streams=(('lf0', 3, 'mse'),), seed=5)
        make = lambda prec, p=0.: models.GRUF0Model(precision=prec, dropout_prob=p, generate=False)
    else:
        feats_np = synthetic.make_acoustic_batch(16, (300, 400), seed=6)
        make = lambda prec, p=0.: models.LSTMAcousticModel(precision=prec, num_layers=2, dropout_prob=p, generate=False)
    feats = data.to_device(feats_np, DEV)
    got = {}
    monkeypatch.setattr(utils, 'CONCAT_PHONE_RATE', True)             # measured and off by default (utils.CONCAT_PHONE_RATE)
    for tag, prec, choice in (('fp32', 'fp32', None), ('phone', 'bf16', True), ('frame', 'bf16', False)):
        torch.manual_seed(2)
        model = make(prec).to(DEV)
        model.phone_rate = choice
        calls = []
        _lib.CALL_LOG = calls
        try:
            loss, _ = model(feats)
            F_hip.backward(loss)
        finally:
            _lib.CALL_LOG = None
        ops.check_persistent_status()
        assert (calls.count('mg_phone_concat_layer_bf16') == 1) == (tag == 'phone'), (tag, calls.count('mg_phone_concat_layer_bf16'))
        assert (calls.count('mg_segment_sum_feat_bf16') == 1) == (tag == 'phone') == (calls.count('mg_feat_wgrad_reduce') == 1)
        assert (calls.count('mg_gather_concat_bf16') == 1) == (tag == 'frame')
        got[tag] = (float(loss.detach()), {n: p.grad.detach().cpu().numpy().copy() for n, p in model.named_parameters()})
    for tag in ('phone', 'frame'):
        np.testing.assert_allclose(got[tag][0], got['fp32'][0], rtol=RTOL_BF16)
        for name, want in got['fp32'][1].items():
            assert rel_err(got[tag][1][name], want) < 5e-2, (tag, name, rel_err(got[tag][1][name], want))
    for name, want in got['frame'][1].items():
        assert rel_err(got['phone'][1][name], want) < 3e-2, (name, rel_err(got['phone'][1][name], want))
    # active dropout behind the first layer: the mask is per frame, drawn over the layer's frame-rate output either way
    torch.manual_seed(2)
    model = make('bf16', 0.2).to(DEV)
    model.phone_rate = True
    model.train()
    calls = []
    _lib.CALL_LOG = calls
    try:
        loss, _ = model(feats)
        F_hip.backward(loss)
    finally:
        _lib.CALL_LOG = None
    assert calls.count('mg_phone_concat_layer_bf16') == 1 and calls.count('mg_dropout') >= 2
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in model.parameters())


@pytest.mark.parametrize('n,c', [(512, 9), (256, 9), (104, 3), (1024, 16)])
def test_segment_sum_with_frame_feature_gradients(n, c):
    """mg_segment_sum_feat_bf16 + mg_feat_wgrad_reduce (csrc/phone_rate.hip): the per-phone sums of a bf16 gradient - bit for bit
    mg_segment_sum's - and from the same pass dW[:, col0:col0+C] = g^T feat (fp32 sums of bf16 g times fp32 features: 1e-5 of the
    largest element against float64), overwriting or accumulating; padding frames (row -1) count; run twice: the same bits."""
    rng = np.random.RandomState(n + c)
    r, extra, col0 = 700, 1024, 600
    counts = rng.randint(0, 24, size=r)
    pieces = []
    for i, k in enumerate(counts):
        pieces.append(np.full(k, i))
        if i % 97 == 96:
            pieces.append(-np.ones(rng.randint(1, 40)))
    rows_np = np.concatenate(pieces).astype(np.int32)
    m = rows_np.size
    rows = torch.from_numpy(rows_np).to(DEV)
    seg, mapped = ops.segment_bounds(rows, r, pad_row=r)
    g = ops.cast_pad_bf16(dev(rng.standard_normal((m, n)).astype(np.float32)))
    feat = dev(rng.uniform(0, 1, (m, c)).astype(np.float32))
    want_sums = ops.segment_sum(g, mapped, seg, r, g.shape[1], extra=extra)
    sums, slabs = ops.segment_sum_feat(g, mapped, seg, r, g.shape[1], feat, extra=extra)
    assert torch.equal(sums, want_sums)
    dw = torch.full((n, col0 + c + 2), 7.0, device=DEV)
    ops.feat_wgrad_reduce(slabs, c, sums.shape[1], n, dw, col0, accumulate=False)
    want = (g[:, :n].double().t() @ feat.double())
    got = dw[:, col0:col0 + c].double()
    assert float((got - want).abs().max() / want.abs().max()) < 1e-5
    assert bool((dw[:, :col0] == 7.0).all()) and bool((dw[:, col0 + c:] == 7.0).all())
    ops.feat_wgrad_reduce(slabs, c, sums.shape[1], n, dw, col0, accumulate=True)
    assert torch.allclose(dw[:, col0:col0 + c].double(), 2 * got, rtol=1e-6)
    sums2, slabs2 = ops.segment_sum_feat(g, mapped, seg, r, g.shape[1], feat, extra=extra)
    assert torch.equal(slabs2, slabs) and torch.equal(sums2, sums)
