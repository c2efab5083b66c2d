"""tests/recurrent_ref64.py checked on the CPU, before any kernel is held to it (no GPU needed):

* the free-running float64 recurrences and every BPTT output against torch.nn.GRU / torch.nn.LSTM in float64 behind
  pack_padded_sequence(enforce_sorted=False) / pad_packed_sequence with autograd (the reference project's call sequence), to 1e-12;
* the step functions chained reproduce the runs (1e-13);
* the bf16 rounding helper equals torch's conversion bit for bit;
* the derived bound HOLDS for an honest float32 evaluation in three summation orders (every element within 1.0 x bound) and BITES for
  a wrong one: each mutation of the float32 evaluation must exceed SAFETY x bound in the same residual drivers the GPU tests use."""
import numpy as np
import pytest
import torch

import recurrent_ref64 as ref

SAFETY = 2.0          # the GPU module's constant (tests/test_gpu_recurrent_ref64.py); a property of fp32, not of a kernel
F32 = np.float32


def _inputs(cell, b, t, h, seed, with_init=True, lengths=True):
    g = 3 if cell == 'gru' else 4
    rng = np.random.RandomState(seed)
    d = {'xproj': rng.randn(b, t, g * h), 'w_hh': rng.uniform(-1, 1, (g * h, h)) / np.sqrt(h), 'b_hh': rng.uniform(-0.5, 0.5, g * h),
         'h0': 0.5 * rng.randn(b, h) if with_init else None, 'c0': 0.5 * rng.randn(b, h) if with_init and cell == 'lstm' else None,
         'grad_out': rng.randn(b, t, h), 'grad_hn': rng.randn(b, h), 'grad_cn': rng.randn(b, h)}
    if lengths:
        sl = rng.randint(1, t + 1, size=b)
        sl[0], sl[-1] = t, 1
        d['seq_len'] = sl.astype(np.int64)
    else:
        d['seq_len'] = None
    return d


# ------------------------------------------------------------------------------------------------- against torch float64
@pytest.mark.parametrize('with_init', [True, False])
@pytest.mark.parametrize('h', [5, 30, 64])
@pytest.mark.parametrize('cell', ['gru', 'lstm'])
def test_runs_and_gradients_equal_torch_float64(cell, h, with_init):
    b, t, i_dim = 6, 9, 7
    g = 3 if cell == 'gru' else 4
    rng = np.random.RandomState(100 + h)
    seq = np.array([t, 4, 7, 2, 9, 1], dtype=np.int64)           # ragged, unsorted, one full item and a 1-step item
    x = rng.randn(b, t, i_dim)
    net = (torch.nn.GRU if cell == 'gru' else torch.nn.LSTM)(i_dim, h, batch_first=True).double()
    w_ih, w_hh, b_ih, b_hh = (p.detach().numpy() for p in (net.weight_ih_l0, net.weight_hh_l0, net.bias_ih_l0, net.bias_hh_l0))
    h0 = 0.5 * rng.randn(b, h) if with_init else None
    c0 = 0.5 * rng.randn(b, h) if with_init and cell == 'lstm' else None
    grad_out = rng.randn(b, t, h)
    grad_hn = rng.randn(b, h) if with_init else None                # "with and without initial states / grad_hn"
    grad_cn = rng.randn(b, h) if with_init and cell == 'lstm' else None

    xt = torch.tensor(x, requires_grad=True)
    h0t = torch.tensor(h0).unsqueeze(0).requires_grad_() if h0 is not None else None
    c0t = torch.tensor(c0).unsqueeze(0).requires_grad_() if c0 is not None else None
    packed = torch.nn.utils.rnn.pack_padded_sequence(xt, torch.tensor(seq), batch_first=True, enforce_sorted=False)
    if cell == 'gru':
        y, hn = net(packed, h0t)
        cn = None
    else:
        hidden = None if h0t is None else (h0t, c0t)
        y, (hn, cn) = net(packed, hidden)
    y, _ = torch.nn.utils.rnn.pad_packed_sequence(y, batch_first=True, total_length=t)
    loss = (y * torch.tensor(grad_out)).sum()
    if grad_hn is not None:
        loss = loss + (hn[0] * torch.tensor(grad_hn)).sum()
    if grad_cn is not None:
        loss = loss + (cn[0] * torch.tensor(grad_cn)).sum()
    loss.backward()

    xproj = x @ w_ih.T + b_ih
    if cell == 'gru':
        out, hstate, saved = ref.gru_run(xproj, w_hh, b_hh, seq, h0)
        dxproj, dhproj, dh0 = ref.gru_run_bwd(grad_out, grad_hn, hstate, saved, w_hh, seq)
        dc0 = None
    else:
        out, hstate, cstate, saved = ref.lstm_run(xproj, w_hh, b_hh, seq, h0, c0)
        dxproj, dh0, dc0 = ref.lstm_run_bwd(grad_out, grad_hn, grad_cn, cstate, saved, w_hh, seq)
        dhproj = dxproj
        assert ref.rel_err(cstate[:, t], cn[0].detach().numpy()) < 1e-12
    checks = {'out': (out, y), 'h_n': (hstate[:, t], hn[0]), 'dx': (dxproj @ w_ih, xt.grad),
              'dw_ih': (np.einsum('btg,bti->gi', dxproj, x), net.weight_ih_l0.grad), 'db_ih': (dxproj.sum((0, 1)), net.bias_ih_l0.grad),
              'dw_hh': (np.einsum('btg,bth->gh', dhproj, hstate[:, :t]), net.weight_hh_l0.grad),
              'db_hh': (dhproj.sum((0, 1)), net.bias_hh_l0.grad)}
    if h0 is not None:
        checks['dh0'] = (dh0, h0t.grad[0])
    if c0 is not None:
        checks['dc0'] = (dc0, c0t.grad[0])
    for name, (got, want) in checks.items():
        assert ref.rel_err(got, want.detach().numpy()) < 1e-12, name
    for item in range(b):                                          # the header's contract past an item's length
        assert np.all(out[item, seq[item]:] == 0) and np.all(hstate[item, seq[item]:] == hstate[item, seq[item]])
        assert np.all(dxproj[item, seq[item]:] == 0)


@pytest.mark.parametrize('cell', ['gru', 'lstm'])
def test_chained_steps_reproduce_the_run(cell):
    d = _inputs(cell, 5, 8, 30, seed=7)
    b, t, h = 5, 8, 30
    if cell == 'gru':
        out, hstate, saved = ref.gru_run(d['xproj'], d['w_hh'], d['b_hh'], d['seq_len'], d['h0'])
        dxproj, dhproj, dh0 = ref.gru_run_bwd(d['grad_out'], d['grad_hn'], hstate, saved, d['w_hh'], d['seq_len'])
        state = d['h0']
        for s in range(t):
            st = ref.gru_step(d['xproj'][:, s], state, state, d['w_hh'], d['b_hh'])
            act = (s < d['seq_len'])[:, None]
            state = np.where(act, st['h_new'].v, state)
            assert np.abs(state - hstate[:, s + 1]).max() < 1e-13
            assert np.abs(np.concatenate([st[k].v for k in ('r', 'z', 'n', 'hn')], 1) - saved[:, s])[act[:, 0]].max() < 1e-13
        carry = ref.Bounded(d['grad_hn'])
        for s in range(t - 1, -1, -1):
            dstate = ref.state_grad(dhproj[:, s + 1] if s + 1 < t else None, d['w_hh'], carry)
            g = ref.gru_step_bwd(dstate, d['grad_out'][:, s], *(saved[:, s, k * h:(k + 1) * h] for k in range(4)), hstate[:, s], s < d['seq_len'])
            assert np.abs(np.concatenate([g[k].v for k in ('dr', 'dz', 'dn')], 1) - dxproj[:, s]).max() < 1e-13
            assert np.abs(g['dnr'].v - dhproj[:, s, 2 * h:]).max() < 1e-13
            carry = g['carry']
        assert np.abs(ref.state_grad(dhproj[:, 0], d['w_hh'], carry).v - dh0).max() < 1e-13
        # and the residual drivers accept the float64 run with a ratio of (next to) zero
        assert ref.gru_forward_residual('f64', d['xproj'], d['w_hh'], d['b_hh'], d['seq_len'], hstate, hstate, out, saved).ratio < 1e-6
        assert ref.gru_backward_residual('f64', d['grad_out'], d['grad_hn'], hstate, saved, d['w_hh'], d['seq_len'], dxproj, dhproj, dhproj,
                                         dh0).ratio < 1e-6
    else:
        out, hstate, cstate, saved = ref.lstm_run(d['xproj'], d['w_hh'], d['b_hh'], d['seq_len'], d['h0'], d['c0'])
        dgates, dh0, dc0 = ref.lstm_run_bwd(d['grad_out'], d['grad_hn'], d['grad_cn'], cstate, saved, d['w_hh'], d['seq_len'])
        hs, cs = d['h0'], d['c0']
        for s in range(t):
            st = ref.lstm_step(d['xproj'][:, s], hs, cs, d['w_hh'], d['b_hh'])
            act = (s < d['seq_len'])[:, None]
            hs, cs = np.where(act, st['h_new'].v, hs), np.where(act, st['c_new'].v, cs)
            assert np.abs(hs - hstate[:, s + 1]).max() < 1e-13 and np.abs(cs - cstate[:, s + 1]).max() < 1e-13
            assert np.abs(np.concatenate([st[k].v for k in ('i', 'f', 'g', 'o')], 1) - saved[:, s])[act[:, 0]].max() < 1e-13
        assert ref.lstm_forward_residual('f64', d['xproj'], d['w_hh'], d['b_hh'], d['seq_len'], hstate, hstate, cstate, out, saved).ratio < 1e-6
        w = ref.lstm_backward_residual('f64', d['grad_out'], d['grad_hn'], d['grad_cn'], cstate, saved, d['w_hh'], d['seq_len'], dgates, dgates,
                                       dh0, dc0)
        assert w.ratio < 1e-6, w.where


def test_stacks_compose_the_single_layer_runs():
    rng = np.random.RandomState(3)
    b, t, h, n_layers = 4, 6, 8, 3
    seq = np.array([t, 3, 5, 1])
    for cell, g in (('gru', 3), ('lstm', 4)):
        w_ih = [rng.uniform(-1, 1, (g * h, h)) / np.sqrt(h) for _ in range(n_layers)]
        w_hh = [rng.uniform(-1, 1, (g * h, h)) / np.sqrt(h) for _ in range(n_layers)]
        b_ih = [rng.uniform(-0.5, 0.5, g * h) for _ in range(n_layers)]
        b_hh = [rng.uniform(-0.5, 0.5, g * h) for _ in range(n_layers)]
        x = rng.randn(b, t, h)
        net = (torch.nn.GRU if cell == 'gru' else torch.nn.LSTM)(h, h, num_layers=n_layers, batch_first=True).double()
        with torch.no_grad():
            for l in range(n_layers):
                for name, val in (('weight_ih', w_ih), ('weight_hh', w_hh), ('bias_ih', b_ih), ('bias_hh', b_hh)):
                    getattr(net, '%s_l%d' % (name, l)).copy_(torch.tensor(val[l]))
        xt = torch.tensor(x, requires_grad=True)
        y, _ = net(torch.nn.utils.rnn.pack_padded_sequence(xt, torch.tensor(seq), batch_first=True, enforce_sorted=False))
        y, _ = torch.nn.utils.rnn.pad_packed_sequence(y, batch_first=True, total_length=t)
        grad_out = rng.randn(b, t, h)
        (y * torch.tensor(grad_out)).sum().backward()
        xproj0 = x @ w_ih[0].T + b_ih[0]
        if cell == 'gru':
            outs, hstates, saveds = ref.gru_stack_run(xproj0, w_ih, w_hh, b_ih, b_hh, seq)
            dxp, dhp, _ = ref.gru_stack_run_bwd(grad_out, None, hstates, saveds, w_ih, w_hh, seq)
        else:
            outs, hstates, cstates, saveds = ref.lstm_stack_run(xproj0, w_ih, w_hh, b_ih, b_hh, seq)
            dxp, _, _ = ref.lstm_stack_run_bwd(grad_out, None, None, cstates, saveds, w_ih, w_hh, seq)
            dhp = dxp
        assert ref.rel_err(outs[-1], y.detach().numpy()) < 1e-12
        assert ref.rel_err(dxp[0] @ w_ih[0], xt.grad.numpy()) < 1e-12
        for l in range(n_layers):
            want = getattr(net, 'weight_hh_l%d' % l).grad.numpy()
            assert ref.rel_err(np.einsum('btg,bth->gh', dhp[l], hstates[l][:, :t]), want) < 1e-12, (cell, l)


# ------------------------------------------------------------------------------------------------- bf16 helper
def test_bf16_round_equals_torch_bit_for_bit():
    rng = np.random.RandomState(11)
    rand = (rng.randn(1000000) * np.exp(rng.uniform(-40, 40, 1000000))).astype(F32)
    hi = np.arange(0x3F80, 0x3F90, dtype=np.uint32) << 16                              # ties: exactly half way between two bf16 values
    ties = np.concatenate([hi | 0x8000, hi | 0x7FFF, hi | 0x8001, (hi | 0x8000) | 0x80000000]).astype(np.uint32).view(F32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-40, 5.8e-39, 1.1754942e-38, 3.4028235e38, -3.4028235e38,
                        3.3895314e38, 3.39e38], dtype=F32)
    x = np.concatenate([rand, ties, special])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = ref.bf16_bits(x)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.all((want[nan] & 0x7FFF) > 0x7F80) and np.all((got[nan] & 0x7FFF) > 0x7F80)       # NaN stays NaN (payloads may differ)
    back = ref.bf16_round(x[~nan])
    assert np.array_equal(back, torch.from_numpy(x[~nan]).to(torch.bfloat16).float().numpy())
    assert ref.bf16_round(x[~nan].astype(np.float64)).dtype == np.float64


# ------------------------------------------------------------------------------------------------- the bound holds, and bites
def _dot32(a, w, order):
    """a [B,K] x w [N,K]^T in float32, one product and one addition at a time, in the given summation order."""
    a, w = a.astype(F32), w.astype(F32)
    k_len = a.shape[1]
    def chain(ks):
        acc = np.zeros((a.shape[0], w.shape[0]), dtype=F32)
        for k in ks:
            acc = acc + a[:, k:k + 1] * w[None, :, k]
        return acc
    if order == 'forward':
        return chain(range(k_len))
    if order == 'reversed':
        return chain(range(k_len - 1, -1, -1))
    q = [chain(range(i * k_len // 4, (i + 1) * k_len // 4)) for i in range(4)]           # the kernels' four waves
    return (q[0] + q[1]) + (q[2] + q[3])


def _sig32(x):
    return (F32(1) / (F32(1) + np.exp(-x.astype(F32)))).astype(F32)


def _gru_f32(d, order, mutate=None):
    """An honest float32 GRU forward + backward (every operation rounded to float32), optionally made wrong in one place."""
    x, w, bias = d['xproj'].astype(F32), d['w_hh'].astype(F32), d['b_hh'].astype(F32)
    b, t, h3 = x.shape
    h = h3 // 3
    seq = d['seq_len']
    w_f = w.copy()
    if mutate == 'drop_k':
        w_f[:, h - 1] = 0
    if mutate == 'swap_zn':
        w_f = np.concatenate([w[:h], w[2 * h:], w[h:2 * h]])
    if mutate == 'drop_bias':
        bias = bias.copy()
        bias[h:2 * h] = 0
    hstate = np.zeros((b, t + 1, h), F32)
    if d['h0'] is not None:
        hstate[:, 0] = d['h0']
    out, saved = np.zeros((b, t, h), F32), np.zeros((b, t, 4 * h), F32)
    for s in range(t):
        hp = hstate[:, s]
        hproj = _dot32(hp, w_f, order) + bias
        r, z = _sig32(x[:, s, :h] + hproj[:, :h]), _sig32(x[:, s, h:2 * h] + hproj[:, h:2 * h])
        hn = hproj[:, 2 * h:]
        n = np.tanh(x[:, s, 2 * h:] + r * hn).astype(F32)
        hnew = (F32(1) - z) * n + z * hp
        act = (np.ones(b, bool) if seq is None else s < seq)[:, None]
        if mutate == 'unfrozen' and s == t - 1:
            act = act | True                                       # the padded items take h_new on this step
        hstate[:, s + 1] = np.where(act, hnew, hp)
        out[:, s] = np.where((np.ones(b, bool) if seq is None else s < seq)[:, None], hnew, 0)
        saved[:, s] = np.concatenate([r, z, n, hn], 1)
    if mutate == 'zero_row':
        hstate[b - 1, 1:], saved[b - 1], out[b - 1] = 0, 0, 0
    dxproj, dhproj = np.zeros((b, t, h3), F32), np.zeros((b, t, h3), F32)
    carry = np.zeros((b, h), F32) if mutate == 'no_grad_hn' else d['grad_hn'].astype(F32)
    go = d['grad_out'].astype(F32)
    wt = np.ascontiguousarray(w.T)
    for s in range(t - 1, -1, -1):
        dstate = carry + _dot32(dhproj[:, s + 1], wt, order) if s + 1 < t else carry
        r, z, n, hn = (saved[:, s, k * h:(k + 1) * h] for k in range(4))
        dh = dstate + go[:, s]
        dn = dh * (F32(1) - z) * (F32(1) - n * n)
        dz = dh * (hstate[:, s] - n) * z * (F32(1) - z)
        dr = dn * hn * r * (F32(1) - r)
        act = (np.ones(b, bool) if seq is None else s < seq)[:, None]
        dxproj[:, s] = np.where(act, np.concatenate([dr, dz, dn], 1), 0)
        dhproj[:, s] = np.where(act, np.concatenate([dr, dz, dn * r], 1), 0)
        carry = np.where(act, dh * z, dstate)
    dh0 = carry + _dot32(dhproj[:, 0], wt, order)
    return out, hstate, saved, dxproj, dhproj, dh0


def _lstm_f32(d, order, mutate=None):
    x, w, bias = d['xproj'].astype(F32), d['w_hh'].astype(F32), d['b_hh'].astype(F32)
    b, t, h4 = x.shape
    h = h4 // 4
    seq = d['seq_len']
    w_f = w.copy()
    if mutate == 'drop_k':
        w_f[:, h - 1] = 0
    if mutate == 'swap_zn':                                        # the LSTM's twin: f and g slices
        w_f = np.concatenate([w[:h], w[2 * h:3 * h], w[h:2 * h], w[3 * h:]])
    if mutate == 'drop_bias':
        bias = bias.copy()
        bias[h:2 * h] = 0
    hstate, cstate = np.zeros((b, t + 1, h), F32), np.zeros((b, t + 1, h), F32)
    if d['h0'] is not None:
        hstate[:, 0], cstate[:, 0] = d['h0'], d['c0']
    out, saved = np.zeros((b, t, h), F32), np.zeros((b, t, 4 * h), F32)
    for s in range(t):
        hp, cp = hstate[:, s], cstate[:, s]
        pre = x[:, s] + (_dot32(hp, w_f, order) + bias)
        i, f, o = _sig32(pre[:, :h]), _sig32(pre[:, h:2 * h]), _sig32(pre[:, 3 * h:])
        g = np.tanh(pre[:, 2 * h:3 * h]).astype(F32)
        cnew = f * cp + i * g
        hnew = o * np.tanh(cnew).astype(F32)
        live = (np.ones(b, bool) if seq is None else s < seq)[:, None]
        act = live | True if (mutate == 'unfrozen' and s == t - 1) else live
        hstate[:, s + 1], cstate[:, s + 1] = np.where(act, hnew, hp), np.where(act, cnew, cp)
        out[:, s] = np.where(live, hnew, 0)
        saved[:, s] = np.concatenate([i, f, g, o], 1)
    if mutate == 'zero_row':
        hstate[b - 1, 1:], cstate[b - 1, 1:], saved[b - 1], out[b - 1] = 0, 0, 0, 0
    dgates = np.zeros((b, t, h4), F32)
    carry_h = np.zeros((b, h), F32) if mutate == 'no_grad_hn' else d['grad_hn'].astype(F32)
    carry_c = d['grad_cn'].astype(F32)
    go = d['grad_out'].astype(F32)
    wt = np.ascontiguousarray(w.T)
    one = F32(1)
    for s in range(t - 1, -1, -1):
        dh_state = carry_h + _dot32(dgates[:, s + 1], wt, order) if s + 1 < t else carry_h
        i, f, g, o = (saved[:, s, k * h:(k + 1) * h] for k in range(4))
        dh = dh_state + go[:, s]
        tc = np.tanh(cstate[:, s + 1]).astype(F32)
        dc = carry_c + dh * o * (one - tc * tc)
        act = (np.ones(b, bool) if seq is None else s < seq)[:, None]
        dg = np.concatenate([dc * g * i * (one - i), dc * cstate[:, s] * f * (one - f), dc * i * (one - g * g), dh * tc * o * (one - o)], 1)
        dgates[:, s] = np.where(act, dg, 0)
        carry_h = np.where(act, 0, dh_state).astype(F32)
        carry_c = np.where(act, dc * f, carry_c).astype(F32)
    dh0 = carry_h + _dot32(dgates[:, 0], wt, order)
    return out, hstate, cstate, saved, dgates, dh0, carry_c


def _residuals(cell, d, res):
    if cell == 'gru':
        out, hstate, saved, dxproj, dhproj, dh0 = res
        fwd = ref.gru_forward_residual('f32 numpy', d['xproj'].astype(F32), d['w_hh'].astype(F32), d['b_hh'].astype(F32), d['seq_len'], hstate,
                                       hstate, out, saved)
        bwd = ref.gru_backward_residual('f32 numpy', d['grad_out'].astype(F32), d['grad_hn'].astype(F32), hstate, saved, d['w_hh'].astype(F32),
                                        d['seq_len'], dxproj, dhproj, dhproj, dh0)
    else:
        out, hstate, cstate, saved, dgates, dh0, dc0 = res
        fwd = ref.lstm_forward_residual('f32 numpy', d['xproj'].astype(F32), d['w_hh'].astype(F32), d['b_hh'].astype(F32), d['seq_len'], hstate,
                                        hstate, cstate, out, saved)
        bwd = ref.lstm_backward_residual('f32 numpy', d['grad_out'].astype(F32), d['grad_hn'].astype(F32), d['grad_cn'].astype(F32), cstate, saved,
                                         d['w_hh'].astype(F32), d['seq_len'], dgates, dgates, dh0, dc0)
    return fwd, bwd


_HONEST = {}


def _honest(cell, h, order):
    key = (cell, h, order)
    if key not in _HONEST:
        d = _inputs(cell, 33, 4, h, seed=h)
        _HONEST[key] = (d, (_gru_f32 if cell == 'gru' else _lstm_f32)(d, order))
    return _HONEST[key]


@pytest.mark.parametrize('order', ['forward', 'reversed', 'split4'])
@pytest.mark.parametrize('h', [100, 256, 512])
@pytest.mark.parametrize('cell', ['gru', 'lstm'])
def test_bound_holds_for_an_honest_float32_evaluation(cell, h, order):
    d, res = _honest(cell, h, order)
    fwd, bwd = _residuals(cell, d, res)
    print('%s H=%d %s: forward %.4f x bound, backward %.4f x bound' % (cell, h, order, fwd.ratio, bwd.ratio))
    assert fwd.checks > 0 and bwd.checks > 0
    assert fwd.ratio <= 1.0, fwd.where
    assert bwd.ratio <= 1.0, bwd.where


MUTATIONS = {'drop_k': 'fwd', 'drop_bias': 'fwd', 'swap_zn': 'fwd', 'unfrozen': 'fwd', 'no_grad_hn': 'bwd', 'zero_row': 'fwd'}


@pytest.mark.parametrize('mutation', sorted(MUTATIONS))
@pytest.mark.parametrize('h', [100, 256, 512])
@pytest.mark.parametrize('cell', ['gru', 'lstm'])
def test_bound_bites_for_a_wrong_evaluation(cell, h, mutation):
    """drop contraction element H - 1; drop b_hh of one gate; swap two gate slices of w_hh (GRU z / n, LSTM f / g); take h_new instead of
    the frozen state on one padded step; forget grad_hn; zero the last row of the batch tile - each must FAIL the residual check."""
    d = _inputs(cell, 33, 4, h, seed=h)
    res = (_gru_f32 if cell == 'gru' else _lstm_f32)(d, 'split4', mutate=mutation)
    fwd, bwd = _residuals(cell, d, res)
    hit = fwd if MUTATIONS[mutation] == 'fwd' else bwd
    print('%s H=%d %s: %.3g x bound (%s)' % (cell, h, mutation, hit.ratio, hit.where))
    assert hit.ratio > SAFETY, 'the bound does not catch %s: %.3g x bound' % (mutation, hit.ratio)
