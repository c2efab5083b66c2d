"""utils.pool_segments on the GPU (csrc/segpool.hip): every expectation comes from the long-double restatement tests/segpool_ref64.py
and its derived bounds.  The C entry points write into guarded allocations; every frame that belongs to no segment holds NaN."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import segpool_ref64 as ref
from morgana_amd import _lib, data, experiment_builder, models, ops, utils
from morgana_amd import functional as F_hip

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = np.float32(7.5e33)
IGUARD = np.int32(-77777)
CHUNK = _lib.load().mg_segment_pool_chunk()
T = 2 * CHUNK + 5
WIDTHS = (1, 3, 4, 64, 65, 130)
SHARES = {}                           # the largest measured share of a derived bound, by kind


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the shared cases are read-only


def _tables():
    """name -> (segment lengths (3, S) int64, seq_len (3,) int64 or None)."""
    main = np.array([
        # starts 0 0 1 3 3 5 | CHUNK + 13 | CHUNK + 28 | past.  n_b = T - 3 cuts the segment of 50, the last one lies wholly past it
        [0, 1, 2, -3, 2, CHUNK + 8, 15, 50, 4],
        # the lengths end at CHUNK + 10 < n_b = T - 9: the frames behind them are valid, belong to no segment and get a +0 gradient
        [5, 2, 1, CHUNK + 1, 0, 1, 0, 0, 0],
        [3, 4, 5, 0, 1, 2, 3, 0, 0],                          # seq_len = 0: nothing is read
    ], dtype=np.int64)
    return {'main': (main, np.array([T - 3, T - 9, 0], dtype=np.int64)),
            'whole': (np.array([[T], [CHUNK + 1], [1]], dtype=np.int64), np.array([T, CHUNK + 1, 1], dtype=np.int64)),
            'ones': (np.ones((3, T), dtype=np.int64), None)}


TABLES = _tables()


@functools.lru_cache(maxsize=None)
def _case(table, f, mode):
    """(x with NaN on every never-read frame, grad_out, restated forward, restated backward) - computed once, read-only."""
    lens, seq_len = TABLES[table]
    rng = np.random.RandomState(1000 + 7 * f + len(table))
    x = rng.standard_normal((3, T, f)).astype(np.float32)
    x[~ref.frames_read(lens, seq_len, T)] = np.nan
    g = rng.standard_normal((3, lens.shape[1], f)).astype(np.float32)
    fwd = ref.pool(x, lens, mode, seq_len)
    bwd = ref.pool_grad(g, lens, mode, T, seq_len, fwd['index'])
    for a in (x, g):
        a.setflags(write=False)
    return x, g, fwd, bwd


def _guarded(n, lead, dtype=np.float32):
    whole = np.full(lead + n + 5, GUARD if dtype == np.float32 else IGUARD, dtype=dtype)
    buf = torch.from_numpy(whole).to(DEV)
    return buf, buf.data_ptr() + 4 * lead


def _inside(buf, lead, n, dtype=np.float32):
    host = buf.cpu().numpy()
    canary = GUARD if dtype == np.float32 else IGUARD
    assert np.all(host[:lead] == canary) and np.all(host[lead + n:] == canary), 'the kernel wrote outside an output'
    return host[lead:lead + n]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def run_forward(x, lens, seq_len, mode, lead):
    """mg_segment_pool_f32 on the device tensor ``x`` (any strides) into guarded outputs -> (out, arg or None) on the host."""
    lib = _lib.load()
    b, t, f = x.shape
    s = lens.shape[1]
    d_lens, d_seq = dev(lens), (dev(seq_len) if seq_len is not None else None)
    out, out_ptr = _guarded(b * s * f, lead)
    arg, arg_ptr = _guarded(b * s * f, lead, np.int32) if mode in ('max', 'min') else (None, None)
    rc = lib.mg_segment_pool_f32(_ptr(x), x.stride(0), x.stride(1), x.stride(2), _ptr(d_lens), _ptr(d_seq), b, s, t, f,
                                 ops.POOL_MODES[mode], ctypes.c_void_p(out_ptr), ctypes.c_void_p(arg_ptr) if arg is not None else None, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    got = _inside(out, lead, b * s * f).reshape(b, s, f)
    return got, (_inside(arg, lead, b * s * f, np.int32).reshape(b, s, f) if arg is not None else None)


def run_backward(g, lens, seq_len, index, mode, t, lead):
    lib = _lib.load()
    b, s, f = g.shape
    d_g, d_lens, d_seq = dev(g), dev(lens), (dev(seq_len) if seq_len is not None else None)
    d_arg = dev(index) if mode in ('max', 'min') else None
    grad, grad_ptr = _guarded(b * t * f, lead)
    rc = lib.mg_segment_pool_bwd_f32(_ptr(d_g), _ptr(d_lens), _ptr(d_seq), _ptr(d_arg), b, s, t, f, ops.POOL_MODES[mode],
                                     ctypes.c_void_p(grad_ptr), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return _inside(grad, lead, b * t * f).reshape(b, t, f)


def _hold(kind, got, want, bound):
    """``got`` float32 against the restatement: bit equality where the bound is 0, else inside the bound; no NaN, every zero a +0."""
    assert not np.isnan(got).any(), 'a NaN of a never-read frame reached %s' % kind
    if want.dtype == np.float32:
        assert ref.same_bits(got, want), kind
        return
    zero = want == 0
    assert not got[zero].any() and not np.signbit(got[zero]).any(), kind
    share = ref.bound_share(got, want, bound)
    SHARES[kind] = max(SHARES.get(kind, 0.0), share)
    print('%s: largest share of its bound %.4f' % (kind, share))
    assert share <= 1.0, (kind, share)


# ------------------------------------------------------------------------------------------------- values, indices, gradients
@pytest.mark.parametrize('mode', ref.MODES)
@pytest.mark.parametrize('f', WIDTHS)
@pytest.mark.parametrize('table', sorted(TABLES))
def test_forward_and_backward_against_the_restatement(table, f, mode):
    lens, seq_len = TABLES[table]
    x, g, fwd, bwd = _case(table, f, mode)
    lead = 4 if f % 2 == 0 else 3                           # outputs at and off a 16-byte boundary
    out, arg = run_forward(dev(x), lens, seq_len, mode, lead)
    _hold('%s value' % mode, out, fwd['value'], fwd['bound'])
    if mode in ('max', 'min'):
        assert ref.same_bits(arg, fwd['index'])
    if table == 'ones':
        assert ref.same_bits(out, x)                        # S = T segments of one frame: the identity
    empty = fwd['m'] == 0
    assert not out[empty].any() and not np.signbit(out[empty]).any()
    grad = run_backward(g, lens, seq_len, fwd['index'], mode, T, lead)
    _hold('%s gradient' % mode, grad, bwd['grad'], bwd['bound'])
    outside = ~ref.frames_read(lens, seq_len, T)
    assert not grad[outside].any() and not np.signbit(grad[outside]).any()


def test_long_segments_cross_every_round_of_chunks():
    """One segment of more than 256 chunks beside a short one: at every width the chunk results of the long segment pass through the
    carry from one round of slots to the next (a round holds at most 256 chunks), on the 16-byte and on the 4-byte path."""
    t = 257 * CHUNK + 3
    lens = np.array([[t, 0], [CHUNK - 1, t - CHUNK - 50]], dtype=np.int64)
    seq_len = np.array([t, t - 20], dtype=np.int64)
    rng = np.random.RandomState(77)
    for f in (1, 4, 64):
        x = rng.standard_normal((2, t, f)).astype(np.float32)
        x[~ref.frames_read(lens, seq_len, t)] = np.nan
        off = torch.full((x.size + 1,), float('nan'), device=DEV)
        off[1:].copy_(dev(x).reshape(-1))
        for mode in ('mean', 'max'):
            want = ref.pool(x, lens, mode, seq_len)
            for name, operand in (('aligned', dev(x)), ('one float past', off[1:].view(2, t, f))):
                out, arg = run_forward(operand, lens, seq_len, mode, 4)
                _hold('%s value, long segments' % mode, out, want['value'], want['bound'])
                if mode == 'max':
                    assert ref.same_bits(arg, want['index']), name


@pytest.mark.parametrize('f, slots', [(1, 256), (4, 256), (64, 16), (65, 4), (130, 4)])
def test_a_segment_ends_in_the_round_in_which_the_next_one_crosses_its_end(f, slots):
    """Two neighbours of 1.25 rounds of chunks each (``slots``: the chunks a round holds at this width on an aligned base): in the
    round in which the first one ends, slot 0 takes the carry of the first while a later slot - another wave at the wide rows -
    leaves the carry of the second.  The one-float-misaligned base runs the same table on the 4-byte path, with other round sizes."""
    n = (slots + slots // 4) * CHUNK + 3
    t = 2 * n + 10
    lens = np.array([[n, n, 7], [3, n, n]], dtype=np.int64)
    seq_len = np.array([t, t - 5], dtype=np.int64)
    rng = np.random.RandomState(78 + f)
    x = rng.standard_normal((2, t, f)).astype(np.float32)
    x[~ref.frames_read(lens, seq_len, t)] = np.nan
    off = torch.full((x.size + 1,), float('nan'), device=DEV)
    off[1:].copy_(dev(x).reshape(-1))
    for mode in ('sum', 'max'):
        want = ref.pool(x, lens, mode, seq_len)
        for name, operand in (('aligned', dev(x)), ('one float past', off[1:].view(2, t, f))):
            out, arg = run_forward(operand, lens, seq_len, mode, 4)
            _hold('%s value, neighbours across a round' % mode, out, want['value'], want['bound'])
            if mode == 'max':
                assert ref.same_bits(arg, want['index']), name


# ---------------------------------------------------------------------------------------------------------- extremum edge cases
def _edge_case():
    lens = np.array([[5, 6, CHUNK + 8, 7, 4]], dtype=np.int64)          # starts 0 5 11 CHUNK+19 CHUNK+26; the rest belongs to no segment
    rng = np.random.RandomState(21)
    x = rng.standard_normal((1, T, 4)).astype(np.float32)
    x[0, 1, 0] = x[0, 3, 0] = 9.0                                       # duplicated maximum, duplicated minimum
    x[0, 2, 1] = x[0, 4, 1] = -9.0
    x[0, 0:5, 2] = [0.0, -0.0, 0.0, -0.0, -0.0]                         # -0 against +0: equal, the lowest frame wins
    x[0, 0:5, 3] = [-0.0, 0.0, -0.0, 0.0, 0.0]
    x[0, 6, 0], x[0, 8, 0] = np.inf, -np.inf                            # +-inf
    x[0, 7, 1], x[0, 9, 1], x[0, 10, 1] = -np.inf, np.inf, np.inf
    x[0, 5:11, 2] = [1.0, np.nan, 5.0, np.nan, -5.0, 2.0]               # NaN in a segment: the first NaN frame, whatever follows
    x[0, 5:11, 3] = -np.abs(x[0, 5:11, 3]) - 1.0                        # all negative: a zero-padded block would answer 0 under max
    x[0, 11 + CHUNK + 2, 0] = np.nan                                    # a NaN in the second chunk of the long segment
    x[0, 13, 1] = x[0, 11 + CHUNK + 1, 1] = 11.0                        # equal maxima in two chunks: the first chunk's frame
    x[0, 12, 2] = x[0, 11 + CHUNK, 2] = -11.0
    x[0, 11:11 + CHUNK + 8, 3] = 3.25                                   # a constant segment
    x[0, CHUNK + 19:CHUNK + 26, :] = -np.abs(x[0, CHUNK + 19:CHUNK + 26, :]) - 0.5
    x[~ref.frames_read(lens, None, T)] = np.nan
    return x, lens


@pytest.mark.parametrize('mode', ['max', 'min'])
def test_extremum_edge_cases(mode):
    x, lens = _edge_case()
    want = ref.pool(x, lens, mode)
    g = np.random.RandomState(22).standard_normal((1, lens.shape[1], 4)).astype(np.float32)
    want_grad = ref.pool_grad(g, lens, mode, T, None, want['index'])['grad']
    # what the restatement must itself say about these inputs
    index, value = want['index'][0], want['value'][0]
    assert index[0, 2] == 0 and index[0, 3] == 0 and np.signbit(value[0, 3]) and not np.signbit(value[0, 2])
    assert index[1, 2] == 6 and np.isnan(value[1, 2]) and index[2, 0] == 11 + CHUNK + 2 and np.isnan(value[2, 0])
    if mode == 'max':
        assert index[0, 0] == 1 and index[1, 0] == 6 and value[1, 0] == np.inf and index[1, 1] == 9 and index[2, 1] == 13
        assert value[1, 3] < 0 and np.all(value[3] < 0) and index[2, 3] == 11
    else:
        assert index[0, 1] == 2 and index[1, 0] == 8 and value[1, 0] == -np.inf and index[1, 1] == 7 and index[2, 2] == 12
    off = torch.full((x.size + 1,), float('nan'), device=DEV)
    off[1:].copy_(dev(x).reshape(-1))
    for operand in (dev(x), off[1:].view(x.shape)):                     # the 16-byte path and the 4-byte path
        out, arg = run_forward(operand, lens, None, mode, 4)
        assert ref.same_bits(out, want['value']) and ref.same_bits(arg, want['index'])
    for lead in (4, 1):
        grad = run_backward(g, lens, None, want['index'], mode, T, lead)
        assert ref.same_bits(grad, want_grad)
        assert grad[0, index[1, 2], 2] == g[0, 1, 2]                    # the gradient lands on the first NaN frame


# -------------------------------------------------------------------------------------------------------------------- layouts
def _layouts(x):
    """name -> a device view with the values of ``x`` (B, T, F) under other strides."""
    b, t, f = x.shape
    wide = torch.full((b, t, f + 7), float('nan'), device=DEV)
    wide[:, :, 3:3 + f] = x
    flat = torch.full((x.numel() + 1,), float('nan'), device=DEV)
    flat[1:] = x.reshape(-1)
    swapped = x.transpose(1, 2).contiguous()                            # (B, F, T)
    return {'column slice': wide[:, :, 3:3 + f], 'one float past alignment': flat[1:].view(b, t, f),
            'transposed': swapped.transpose(1, 2)}


@pytest.mark.parametrize('mode', ref.MODES)
def test_strided_views_give_the_bits_of_their_contiguous_copy(mode):
    lens, seq_len = TABLES['main']
    f = 8
    rng = np.random.RandomState(31)
    x_np = rng.standard_normal((3, T, f)).astype(np.float32)
    x_np[~ref.frames_read(lens, seq_len, T)] = np.nan
    x, d_lens, d_seq = dev(x_np), dev(lens), dev(seq_len)
    g = dev(rng.standard_normal((3, lens.shape[1], f)).astype(np.float32))
    views = _layouts(x)
    narrow = dev(x_np[:, :, :1])
    views['stride-0 expand'] = narrow.expand(3, T, f)
    for name, view in views.items():
        copy = view.clone(memory_format=torch.contiguous_format).requires_grad_(True)
        assert copy.data_ptr() % 16 == 0
        view = view.detach().requires_grad_(True)
        assert view.stride() != copy.stride() or view.data_ptr() % 16 != 0, name
        want = utils.pool_segments(copy, d_lens, mode, seq_len=d_seq)
        got = utils.pool_segments(view, d_lens, mode, seq_len=d_seq)
        (want_grad,), (got_grad,) = torch.autograd.grad(want, copy, g), torch.autograd.grad(got, view, g)
        assert ref.same_bits(got.detach().cpu().numpy(), want.detach().cpu().numpy()), name
        assert ref.same_bits(got_grad.cpu().numpy(), want_grad.cpu().numpy()), name
        assert not torch.isnan(got).any() and not torch.isnan(got_grad).any(), name
    restated = ref.pool(x_np, lens, mode, seq_len)
    got = utils.pool_segments(x, d_lens.unsqueeze(-1).int(), mode, seq_len=d_seq).cpu().numpy()        # (B, S, 1) int32 lengths
    _hold('%s value' % mode, got, restated['value'], restated['bound'])


# ---------------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize('f', [3, 64])
@pytest.mark.parametrize('mode', ['sum', 'mean', 'max'])
def test_order_depends_on_the_segment_alone(mode, f):
    lens, seq_len = TABLES['main']
    rng = np.random.RandomState(41)
    utt = rng.standard_normal((T, f)).astype(np.float32)
    row, n = lens[1], seq_len[1]
    g_row = rng.standard_normal((len(row), f)).astype(np.float32)
    # alone: b = 0 of a batch of 1
    out1, arg1 = run_forward(dev(utt[None]), row[None], np.array([n]), mode, 4)
    again, _ = run_forward(dev(utt[None]), row[None], np.array([n]), mode, 4)
    assert ref.same_bits(out1, again)                                   # two calls, equal bits
    grad1 = run_backward(g_row[None], row[None], np.array([n]), arg1, mode, T, 4)
    # b = 2 of a batch of 3, S padded with zero lengths, other utterances and other segment tables in front
    s3 = len(row) + 7
    lens3 = np.zeros((3, s3), dtype=np.int64)
    lens3[0, :4], lens3[1, :], lens3[2, :len(row)] = [T - 30, 3, 3, 3], 1, row
    x3 = rng.standard_normal((3, T, f)).astype(np.float32)
    x3[2] = utt
    g3 = rng.standard_normal((3, s3, f)).astype(np.float32)
    g3[2, :len(row)] = g_row
    seq3 = np.array([T, T, n], dtype=np.int64)
    out3, arg3 = run_forward(dev(x3), lens3, seq3, mode, 3)
    assert ref.same_bits(out3[2, :len(row)], out1[0])
    assert not out3[2, len(row):].any()
    if mode == 'max':
        assert ref.same_bits(arg3[2, :len(row)], arg1[0])
    grad3 = run_backward(g3, lens3, seq3, arg3, mode, T, 3)
    assert ref.same_bits(grad3[2], grad1[0])


# -------------------------------------------------------------------------------------------------------------- graph capture
def assert_same_bits(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert torch.equal(x.reshape(-1).contiguous().view(torch.uint8), y.reshape(-1).contiguous().view(torch.uint8))


@pytest.mark.parametrize('mode', ['mean', 'max'])
def test_forward_and_backward_capture_into_a_graph(mode):
    """SegmentPoolFn forward and backward inside torch.cuda.graph: a replay on new contents of the same buffers - features, segment
    lengths and sequence lengths alike, all of them read on the device - equals the eager call bit for bit."""
    b, s, f = 3, 9, 20

    def contents(seed):
        r = np.random.RandomState(seed)
        lens = r.randint(-1, 14, size=(b, s)).astype(np.int64)
        return (r.standard_normal((b, T, f)).astype(np.float32), lens, r.randint(0, T + 10, size=(b,)).astype(np.int64),
                r.standard_normal((b, s, f)).astype(np.float32))

    x0, lens0, seq0, g0 = contents(52)
    x, lens, seq, g = dev(x0).requires_grad_(True), dev(lens0), dev(seq0), dev(g0)

    def step():
        out = F_hip.SegmentPoolFn.apply(x, lens, seq, mode)
        (dx,) = torch.autograd.grad(out, x, g)
        return out.detach(), dx

    assert_same_bits(step(), step())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                       # a host read inside the node would end the capture
        captured = step()
    for seed in (53, 54):
        x1, lens1, seq1, g1 = contents(seed)
        with torch.no_grad():
            x.copy_(dev(x1)), lens.copy_(dev(lens1)), seq.copy_(dev(seq1)), g.copy_(dev(g1))
        graph.replay()
        torch.cuda.synchronize()
        assert_same_bits(captured, step())
        want = ref.pool(x1, lens1, mode, seq1)
        _hold('%s value' % mode, captured[0].cpu().numpy(), want['value'], want['bound'])


def test_measured_bound_shares_are_reported():
    """The largest share of each derived bound seen by the tests above (printed; DESIGN.md section 4.26 records them)."""
    for kind in sorted(SHARES):
        print('segment pooling, %s: largest share of the derived bound %.4f' % (kind, SHARES[kind]))
    assert all(share <= 1.0 for share in SHARES.values())


# ------------------------------------------------------------------------------------------------------------------ the model
import torch.nn as nn  # noqa: E402

import test_gpu_vae as vae_tests  # noqa: E402  (its batch, its torch GRU / upsample restatements and its tolerances)


def _torch_vae_f0_pooled64(model, feats, eps, pooling):
    """BaseVAE.forward of VAEF0Model(encoder_pooling=pooling) restated in torch float64 on the CPU -> (loss, parameters by name)."""
    sd = {k: v.detach().cpu().double().clone() for k, v in model.state_dict().items()}
    zd, hid = model.z_dim, model.encoder[0].layer.hidden_size
    enc = nn.GRU(3, hid, batch_first=True).double()
    enc.load_state_dict({k[len('encoder.0.layer.'):]: v for k, v in sd.items() if k.startswith('encoder.0.layer.')})
    proj = nn.Linear(hid, 2 * zd).double()
    proj.load_state_dict({'weight': sd['encoder_projection.0.weight'], 'bias': sd['encoder_projection.0.bias']})
    lin = {i: nn.Linear(*sd['layers.%d.weight' % i].shape[::-1]).double() for i in (0, 9, 12)}
    for i, m in lin.items():
        m.load_state_dict({'weight': sd['layers.%d.weight' % i], 'bias': sd['layers.%d.bias' % i]})
    grus = {}
    for i, n_in in ((3, 256), (5, 64), (7, 64)):
        grus[i] = nn.GRU(n_in, 64, batch_first=True).double()
        grus[i].load_state_dict({k[len('layers.%d.layer.' % i):]: v for k, v in sd.items() if k.startswith('layers.%d.layer.' % i)})
    cf = {k: (v.double() if v.is_floating_point() else v) for k, v in vae_tests._cpu(feats).items()}
    t = cf['normalised_counters'].shape[1]
    n_frames = cf['n_frames']
    seq, _ = vae_tests._torch_gru(enc, cf['normalised_lf0_deltas'], n_frames)
    rows = [seq[i, :int(n)] for i, n in enumerate(n_frames)]
    summary = torch.stack([r.mean(0) if pooling == 'mean' else r.max(0).values for r in rows])
    stats = proj(summary)
    mean, logvar = stats[:, :zd], stats[:, zd:]
    z = mean + torch.exp(0.5 * logvar) * eps.double()
    x = torch.cat((vae_tests._torch_upsample(cf['normalised_lab'], cf['dur'], t), cf['normalised_counters'],
                   z[:, None, :].expand(z.shape[0], t, zd)), -1)
    h = torch.sigmoid(lin[0](x))
    for i in (3, 5, 7):
        h, _ = vae_tests._torch_gru(grus[i], h, n_frames)
    pred = lin[12](torch.sigmoid(lin[9](h)))
    mask = (torch.arange(t)[None, :] < n_frames[:, None]).double()[..., None]
    mse = ((pred - cf['normalised_lf0_deltas']) ** 2 * mask).sum(1) / n_frames[:, None].double()
    kld = torch.mean(-0.5 * torch.sum(1 + logvar - mean ** 2 - torch.exp(logvar), dim=-1))
    named = {'encoder.0.layer.' + k: v for k, v in enc.named_parameters()}
    named.update({'encoder_projection.0.' + k: v for k, v in proj.named_parameters()})
    for i, m in lin.items():
        named.update({'layers.%d.%s' % (i, k): v for k, v in m.named_parameters()})
    for i, m in grus.items():
        named.update({'layers.%d.layer.%s' % (i, k): v for k, v in m.named_parameters()})
    return mse.mean() + model.kld_weight * kld, named


def _counter(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize('pooling', ['mean', 'max'])
def test_vae_f0_model_pooled_encoder_vs_torch_float64(pooling, monkeypatch):
    monkeypatch.setattr(ops, 'dropout_draw', lambda device: _counter(77))
    feats = vae_tests._batch(41, b=4, frames=(50, 70))
    torch.manual_seed(4)
    model = models.VAEF0Model(kld_weight=0.3, precision='fp32', encoder_pooling=pooling).to(DEV)
    loss, out = model(data.to_device(feats, DEV))
    loss.backward()
    _, eps = ops.vae_sample(out['mean'].detach(), out['log_variance'].detach(), ops.dropout_seed(), ops.SAMPLE_SITE, _counter(77))
    want_loss, named = _torch_vae_f0_pooled64(model, feats, eps.cpu(), pooling)
    want_loss.backward()
    tol_out, tol_grad = vae_tests.TOLS['fp32']
    assert abs(loss.item() - want_loss.item()) <= tol_out * abs(want_loss.item())
    for name, prm in model.named_parameters():
        err = vae_tests.rel_err(prm.grad.cpu().numpy(), named[name].grad.numpy())
        print('%s pooling, %s: gradient error %.3g' % (pooling, name, err))
        assert err < tol_grad, name


def test_vae_f0_model_last_pooling_is_the_model_of_before(monkeypatch):
    monkeypatch.setattr(ops, 'dropout_draw', lambda device: _counter(77))
    d = data.to_device(vae_tests._batch(41, b=4, frames=(50, 70)), DEV)
    results = []
    for kwargs in ({}, {'encoder_pooling': 'last'}):
        torch.manual_seed(4)
        model = models.VAEF0Model(kld_weight=0.3, precision='fp32', **kwargs).to(DEV)
        loss, _ = model(d)
        loss.backward()
        results.append([loss.detach()] + [p.grad for p in model.parameters()])
    assert_same_bits(results[0], results[1])


def test_experiment_builder_graphed_equals_eager_with_mean_pooling():
    base = vae_tests._batch(51, b=8, frames=(60, 100))
    batches = []
    for i in range(3):
        b = dict(base)
        b['normalised_lf0_deltas'] = (base['normalised_lf0_deltas'] * (1.0 + 0.1 * i)).astype(np.float32)
        batches.append(data.to_device(b, DEV))

    def train(use_graphs):
        torch.manual_seed(3)
        ops.dropout_state(DEV).zero_()
        builder = experiment_builder.ExperimentBuilder(models.VAEF0Model, dict(precision='bf16', dropout_prob=0.1, encoder_pooling='mean'),
                                                       learning_rate=0.01, device=DEV, use_graphs=use_graphs, graph_group=1)
        optimizer = builder.make_optimizer()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            history = [builder.train_epoch(batches, optimizer) for _ in range(2)]      # three steps, then three more on the captured graphs
        assert not [w for w in caught if 'captur' in str(w.message)], [str(w.message) for w in caught]
        params = {k: v.detach().clone() for k, v in builder.model.named_parameters()}
        return history, params, builder

    hist_e, params_e, _ = train(False)
    hist_g, params_g, builder = train(True)
    assert builder.model.encoder_pooling == 'mean'
    assert builder._graph_cache.replayed_steps > 0, builder._graph_cache.stats()
    assert hist_g == hist_e
    for name in params_e:
        assert torch.equal(params_g[name], params_e[name]), name
