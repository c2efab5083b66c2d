"""Every GRU / LSTM recurrence kernel against the float64 STEP reference of tests/recurrent_ref64.py.

The forward kernels return every state and every gate, so each step is checked on its own, in float64, from the kernel's own stored
inputs of that step and with the exact operands the kernel had (for the bf16 forms: ``hstate_bf[:, t]`` and ``bf16(W_hh)``, both exact
in float64).  Errors do not compound over T and a bf16 rounding flip of a state cannot happen; what remains is the rounding of one K-deep
fp32 dot product plus one cell, for which the reference returns a DERIVED bound per element.  A test asserts
``|got - want| <= SAFETY * bound`` elementwise, with the one module-level SAFETY for every kernel, plus the structural contract of the
header exactly (``out == 0`` and the state frozen past ``seq_len[b]``, shadows bit-equal to the rounded fp32 arrays; ``saved`` past an
item's length is not compared).  The backward kernels do not store their elementwise carry; the reference re-forms it in float64 from
the kernel's own per-step outputs (carry_t = dh_t z_t is a function of quantities the step check has just verified), which makes the
backward residual one product deep as well (recurrent_ref64.gru_backward_residual).  The worst observed / bound ratio of every test goes
to the suite's parity report (tests/parity_report.py) through parity_report.note.

The 26 recurrent entry points of include/morgana_hip.h (K3) and the case that reaches each:
  mg_gru_fwd_f32, mg_gru_bwd_f32                     test_gru_f32_step (general kernels <0>, <8> / <24> at H = 512; H % 4 != 0, H % 16 != 0),
                                                     test_gru_f32_misaligned_views (C ABI, vec == 0 by alignment; H = 128 routes forward to
                                                     the general and backward to the workgroup-local kernel)
  mg_gru_fwd_small_f32, mg_gru_bwd_small_f32         test_gru_small (reached through mg_gru_fwd_f32 / mg_gru_bwd_f32 at H = 64 / 128)
  mg_gru_fwd_persist_f32, mg_gru_bwd_persist_f32     test_gru_f32_persistent
  mg_gru_fwd_bf16, mg_gru_bwd_bf16                   test_gru_bf16[step-*], test_fast_cell_accuracy
  mg_gru_fwd_persist_bf16, _rows_bf16, _out_bf16     test_gru_bf16[persist-*] (ops routes all three through mg_gru_fwd_persist_out_bf16 with
                                                     xrows / out_bf NULL or set; the two narrower entry points are called in
                                                     test_gru_bf16_persistent_narrow_entry_points)
  mg_gru_bwd_persist_bf16                            test_gru_bf16[persist-*] (full and shadows_only)
  mg_lstm_fwd_f32, mg_lstm_bwd_f32                   test_lstm_f32_step, test_lstm_f32_misaligned_views
  mg_lstm_fwd_persist_f32, mg_lstm_bwd_persist_f32   test_lstm_f32_persistent
  mg_lstm_fwd_persist_bf16, mg_lstm_bwd_persist_bf16 test_lstm_bf16_persistent
  mg_lstm_pstack_fwd_bf16, mg_lstm_pstack_bwd_bf16   test_lstm_pstack
  mg_gru_stack_fwd_small_f32, _fast_f32, mg_gru_stack_bwd_small_f32, _fast_f32   test_gru_small_stack[exact / fast]
  mg_lstm_stack_fwd_f32, mg_lstm_stack_bwd_f32       test_lstm_skewed_stack

Free-running check (looser, second): the whole trajectory and all BPTT outputs against gru_run / lstm_run in float64.  Its bound is
measured against the reference ALONE, on the CPU: e_ref = rel_err(numpy float32 run, float64 run) per output (for bf16: float32 with
bf16 operand rounding against float64 with bf16 operand rounding); the kernel must stay within FREE_FACTOR x e_ref.  e_ref as
`python tests/test_gpu_recurrent_ref64.py` prints it (computed again at test time):

    case                      out      h_n      dgate    dh0
    gru  fp32 (16,50,512)   1.8e-07  2.1e-07  1.6e-07  1.3e-07
    gru  fp32 (33,300,256)  3.2e-07  1.9e-07  2.0e-07  2.0e-07
    gru  bf16 (16,50,512)   1.7e-04  1.3e-04  1.2e-04  1.5e-04
    gru  bf16 (33,300,256)  2.7e-04  1.5e-04  2.1e-04  2.1e-04
    lstm fp32 (16,50,512)   2.1e-07  1.7e-07  1.6e-07  4.4e-07
    lstm fp32 (33,300,256)  3.0e-07  1.9e-07  1.7e-07  4.6e-07
    lstm bf16 (16,50,512)   2.0e-04  9.5e-05  1.4e-04  1.9e-04
    lstm bf16 (33,300,256)  2.1e-04  3.4e-05  1.1e-04  3.1e-04

(dgate = dxproj / dgates [B,T,G]; the float32 run's matrix products are numpy's, so the last digit depends on the BLAS underneath.)
"""
import numpy as np
import pytest

import parity_report
import recurrent_ref64 as ref

pytestmark = pytest.mark.gpu

SAFETY = 2.0          # one constant for every kernel: a property of fp32 (the MFMA may round its 4-term partial unlike a scalar chain)
FREE_FACTOR = 8.0     # free-running: a different summation order and, for bf16, state-rounding flips of one bf16 ulp each
DEV = 'cuda:0'


def _torch():
    import torch
    return torch


def _ops():
    from morgana_amd import ops
    return ops


def _dev(a, dtype=None):
    torch = _torch()
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=dtype or torch.float32)


def _host(x):
    """A device tensor as a float64-exact numpy array (bf16 -> float32 is exact)."""
    torch = _torch()
    if x is None:
        return None
    return (x.float() if x.dtype == torch.bfloat16 else x).cpu().numpy()


def _bits(x):
    torch = _torch()
    return x.view(torch.int16).cpu().numpy().view(np.uint16)


def _make(cell, b, t, h, seed, ragged=True, init=True, scale=1.0, on_device=True):
    """Operand distributions of the issue, fixed seeds; everything float32-exact."""
    g = 3 if cell == 'gru' else 4
    rng = np.random.RandomState(seed)
    d = {'xproj': (scale * rng.randn(b, t, g * h)).astype(np.float32), 'w_hh': (rng.uniform(-1, 1, (g * h, h)) / np.sqrt(h)).astype(np.float32),
         'b_hh': rng.uniform(-0.5, 0.5, g * h).astype(np.float32), 'grad_out': rng.randn(b, t, h).astype(np.float32)}
    d['h0'] = (0.5 * rng.randn(b, h)).astype(np.float32) if init else None
    d['c0'] = (0.5 * rng.randn(b, h)).astype(np.float32) if init and cell == 'lstm' else None
    d['grad_hn'] = rng.randn(b, h).astype(np.float32) if init else None
    d['grad_cn'] = rng.randn(b, h).astype(np.float32) if init and cell == 'lstm' else None
    if ragged:
        sl = rng.randint(1, t + 1, size=b).astype(np.int64)
        sl[0], sl[-1] = t, 1
        d['seq_len'] = sl
    else:
        d['seq_len'] = None
    if on_device:
        d['dev'] = {k: (_dev(v, _torch().int64) if k == 'seq_len' else _dev(v)) for k, v in d.items()}
    return d


def _settle(worst_list, finite=()):
    """Record and assert a list of Worst results; ``finite``: arrays that must hold no NaN / inf."""
    worst = max(worst_list, key=lambda w: w.ratio)
    assert all(w.checks > 0 for w in worst_list)
    parity_report.note(worst.ratio, worst.where, bound=SAFETY)
    print('%-60s %.4f x bound' % (worst.form, worst.ratio))
    for a in finite:
        assert np.isfinite(np.asarray(a, dtype=np.float64)).all()
    assert worst.ratio <= SAFETY, worst.where


VARIANTS = [('ragged', True, True), ('full-noinit', False, False)]       # (name, seq_len given, h0 / c0 / grad_hn / grad_cn given)


# ------------------------------------------------------------------------------------------------------------------ GRU drivers
def _gru_case(form, b, t, h, seed, ragged, init, scale=1.0, xrows=False, out_bf=False):
    """Run one forward + backward form through morgana_amd.ops and check every step.  form: step / persist / bf16_step / bf16_persist."""
    torch, ops = _torch(), _ops()
    d = _make('gru', b, t, h, seed, ragged, init, scale)
    v = d['dev']
    bf = form.startswith('bf16')
    persistent = form.endswith('persist')
    label = 'gru %s (%d,%d,%d)%s%s' % (form, b, t, h, '' if ragged else ' seq_len=None', '' if init else ' no h0/grad_hn')
    hstate_bf = None
    if bf:
        kw = {}
        xp = v['xproj']
        if xrows:                                                 # the projections as a shuffled table read through a row map
            perm = np.random.RandomState(seed + 1).permutation(b * t)
            table = torch.empty((b * t, 3 * h), dtype=torch.float32, device=DEV)
            table[_dev(perm, torch.int64)] = v['xproj'].reshape(b * t, 3 * h)
            xp, kw['xrows'] = table, _dev(perm.astype(np.int32), torch.int32).reshape(b, t)
        if out_bf:
            kw['out_bf'] = torch.empty((b, t, h), dtype=torch.bfloat16, device=DEV)
        out, hstate, saved, hstate_bf = ops.gru_fwd_bf16(xp, v['w_hh'], v['b_hh'], v['seq_len'], v['h0'], b, t, h, persistent=persistent, **kw)
        if out_bf:
            assert np.array_equal(_bits(kw['out_bf']), ref.bf16_bits(_host(out))), label + ': out_bf != bf16(out)'
        assert np.array_equal(_bits(hstate_bf), ref.bf16_bits(_host(hstate))), label + ': hstate_bf != bf16(hstate)'
        w_op = ref.bf16_round(d['w_hh'])
    else:
        out, hstate, saved = ops.gru_fwd(v['xproj'], v['w_hh'], v['b_hh'], v['seq_len'], v['h0'], b, t, h, persistent=persistent)
        w_op = d['w_hh']
    out_h, hs_h, sv_h = _host(out), _host(hstate), _host(saved)
    if d['h0'] is not None:
        assert np.array_equal(hs_h[:, 0], d['h0'])
    else:
        assert not hs_h[:, 0].any()
    fwd = ref.gru_forward_residual(label + ' forward', d['xproj'], w_op, d['b_hh'], d['seq_len'], hs_h, _host(hstate_bf) if bf else hs_h, out_h, sv_h,
                                   fast=bf)
    if bf:
        dxp, dhp, dh0, dhp_bf = ops.gru_bwd_bf16(v['grad_out'], v['grad_hn'], hstate, saved, v['w_hh'], v['seq_len'], b, t, h, persistent=persistent)
        assert np.array_equal(_bits(dhp_bf), ref.bf16_bits(_host(dhp))), label + ': dhproj_bf != bf16(dhproj)'
        operand = _host(dhp_bf)
        if persistent:
            dxp_bf2, dhp_bf2, dh02 = ops.gru_bwd_bf16(v['grad_out'], v['grad_hn'], hstate, saved, v['w_hh'], v['seq_len'], b, t, h, persistent=True,
                                                      shadows_only=True)
            assert np.array_equal(_bits(dhp_bf2), _bits(dhp_bf)) and np.array_equal(_bits(dxp_bf2), ref.bf16_bits(_host(dxp)))
            assert np.array_equal(_host(dh02), _host(dh0)), label + ': shadows_only dh0'
    else:
        dxp, dhp, dh0 = ops.gru_bwd(v['grad_out'], v['grad_hn'], hstate, saved, v['w_hh'], v['seq_len'], b, t, h, persistent=persistent)
        operand = _host(dhp)
    bwd = ref.gru_backward_residual(label + ' backward', d['grad_out'], d['grad_hn'], hs_h, sv_h, w_op, d['seq_len'], _host(dxp), _host(dhp), operand,
                                    _host(dh0))
    _settle([fwd, bwd], finite=(out_h, hs_h, _host(dxp), _host(dhp), _host(dh0)))


GRU_STEP_SHAPES = [(33, 12, 256), (130, 9, 384), (5, 20, 320), (16, 10, 512), (7, 11, 30), (19, 6, 100), (3, 5, 187), (1, 1, 17)]


@pytest.mark.parametrize('variant', VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize('shape', GRU_STEP_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_gru_f32_step(shape, variant):
    _gru_case('step', *shape, seed=sum(shape), ragged=variant[1], init=variant[2])


def test_gru_f32_step_saturated():
    _gru_case('step', 33, 12, 256, seed=5, ragged=True, init=True, scale=40.0)


@pytest.mark.parametrize('variant', VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize('shape', [(5, 37, 64), (37, 21, 128)], ids=lambda s: '%dx%dx%d' % s)
def test_gru_small(shape, variant):
    assert _ops()._lib.load().mg_gru_small_supported(shape[2])
    _gru_case('step', *shape, seed=sum(shape), ragged=variant[1], init=variant[2])


@pytest.mark.parametrize('variant', VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize('shape', [(64, 30, 512), (100, 7, 320)], ids=lambda s: '%dx%dx%d' % s)
def test_gru_f32_persistent(shape, variant):
    if not _ops().gru_persist_f32_ok(*shape):
        pytest.skip('mg_gru_persist_f32_supported(%d, %d, %d) == 0' % shape)
    _gru_case('persist', *shape, seed=sum(shape), ragged=variant[1], init=variant[2])


GRU_BF16_SHAPES = [(5, 37, 128), (33, 20, 256), (200, 9, 128), (17, 30, 384), (64, 40, 512)]


@pytest.mark.parametrize('variant', VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize('shape', GRU_BF16_SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('form', ['step', 'persist'])
def test_gru_bf16(form, shape, variant):
    if form == 'persist' and not _ops().gru_persist_ok(*shape):
        pytest.skip('mg_gru_persist_supported(%d, %d, %d) == 0' % shape)
    _gru_case('bf16_' + form, *shape, seed=sum(shape), ragged=variant[1], init=variant[2], xrows=form == 'persist' and variant[1],
              out_bf=form == 'persist')


def test_gru_bf16_saturated():
    _gru_case('bf16_step', 33, 20, 256, seed=6, ragged=True, init=True, scale=40.0)


def test_gru_bf16_persistent_narrow_entry_points():
    """mg_gru_fwd_persist_bf16 and mg_gru_fwd_persist_rows_bf16 (ops calls the widest of the three): the same bits as the _out_ entry."""
    torch, ops = _torch(), _ops()
    b, t, h = 33, 20, 256
    if not ops.gru_persist_ok(b, t, h):
        pytest.skip('mg_gru_persist_supported(%d, %d, %d) == 0' % (b, t, h))
    d = _make('gru', b, t, h, 77)
    v = d['dev']
    want = ops.gru_fwd_bf16(v['xproj'], v['w_hh'], v['b_hh'], v['seq_len'], v['h0'], b, t, h, persistent=True)
    lib = ops._lib.load()
    w_bf = ops.cast_pad_bf16(v['w_hh'])
    ws = ops._persist_workspace(v['xproj'].device, b, h)
    rows = torch.arange(b * t, dtype=torch.int32, device=DEV)
    for entry in ('plain', 'rows'):
        hstate = torch.zeros((b, t + 1, h), dtype=torch.float32, device=DEV)
        hstate[:, 0] = v['h0']
        hstate_bf = hstate.to(torch.bfloat16)
        out = torch.empty((b, t, h), dtype=torch.float32, device=DEV)
        saved = torch.zeros((b, t, 4 * h), dtype=torch.float32, device=DEV)
        p = ops._p
        if entry == 'plain':
            rc = lib.mg_gru_fwd_persist_bf16(p(v['xproj']), p(w_bf), w_bf.shape[1], p(v['b_hh']), p(v['seq_len']), b, t, h, p(hstate), p(hstate_bf),
                                             p(out), p(saved), p(ws), ws.numel(), ops._stream())
        else:
            rc = lib.mg_gru_fwd_persist_rows_bf16(p(v['xproj'].reshape(b * t, 3 * h)), p(rows), b * t, p(w_bf), w_bf.shape[1], p(v['b_hh']),
                                                  p(v['seq_len']), b, t, h, p(hstate), p(hstate_bf), p(out), p(saved), p(ws), ws.numel(), ops._stream())
        ops._lib.check(rc, 'mg_gru_fwd_persist_%s' % entry)
        assert np.array_equal(_host(out), _host(want[0])) and np.array_equal(_host(hstate), _host(want[1]))
        assert np.array_equal(_bits(hstate_bf), _bits(want[3]))
        live = (np.arange(t)[None, :] < d['seq_len'][:, None])
        assert np.array_equal(_host(saved)[live], _host(want[2])[live])


def _offset_view(a, torch):
    """A copy of ``a`` that starts 4 bytes into a 256-byte aligned buffer: never 16-byte aligned."""
    buf = torch.zeros(a.numel() + 8, dtype=a.dtype, device=DEV)
    view = buf[1:1 + a.numel()].view(a.shape)
    view.copy_(a)
    assert view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize('shape', [(9, 7, 256), (9, 7, 128)], ids=lambda s: '%dx%dx%d' % s)
def test_gru_f32_misaligned_views(shape):
    """w_hh, hstate and dhproj as 4-byte-offset views (C ABI): ld4_guard's scalar path by alignment.  At H = 128 the forward leaves the
    workgroup-local kernel for the general one (gru.hip: w_hh alignment) while the backward routes on H alone: the pair must agree."""
    torch, ops = _torch(), _ops()
    b, t, h = shape
    d = _make('gru', b, t, h, 31 + h)
    v = d['dev']
    lib, p = ops._lib.load(), ops._p
    w = _offset_view(v['w_hh'], torch)
    hs0 = torch.zeros((b, t + 1, h), dtype=torch.float32, device=DEV)
    hs0[:, 0] = v['h0']
    hstate = _offset_view(hs0, torch)
    out = torch.empty((b, t, h), dtype=torch.float32, device=DEV)
    saved = torch.empty((b, t, 4 * h), dtype=torch.float32, device=DEV)
    ops._lib.check(lib.mg_gru_fwd_f32(p(v['xproj']), p(w), p(v['b_hh']), p(v['seq_len']), b, t, h, p(hstate), p(out), p(saved), ops._stream()),
                   'mg_gru_fwd_f32')
    dxp = torch.empty((b, t, 3 * h), dtype=torch.float32, device=DEV)
    dhp = _offset_view(torch.zeros((b, t, 3 * h), dtype=torch.float32, device=DEV), torch)
    dh0 = torch.empty((b, h), dtype=torch.float32, device=DEV)
    ws = torch.empty(lib.mg_gru_bwd_workspace_bytes(b, h), dtype=torch.uint8, device=DEV)
    ops._lib.check(lib.mg_gru_bwd_f32(p(v['grad_out']), p(v['grad_hn']), p(hstate), p(saved), p(w), p(v['seq_len']), b, t, h, p(dxp), p(dhp), p(dh0),
                                      p(ws), ws.numel(), ops._stream()), 'mg_gru_bwd_f32')
    label = 'gru step misaligned (%d,%d,%d)' % shape
    hs_h, sv_h = _host(hstate), _host(saved)
    fwd = ref.gru_forward_residual(label + ' forward', d['xproj'], d['w_hh'], d['b_hh'], d['seq_len'], hs_h, hs_h, _host(out), sv_h)
    bwd = ref.gru_backward_residual(label + ' backward', d['grad_out'], d['grad_hn'], hs_h, sv_h, d['w_hh'], d['seq_len'], _host(dxp), _host(dhp),
                                    _host(dhp), _host(dh0))
    _settle([fwd, bwd], finite=(_host(dxp), _host(dh0)))


# ------------------------------------------------------------------------------------------------------------------ LSTM drivers
def _lstm_case(form, b, t, h, seed, ragged, init, scale=1.0):
    """form: step / persist (fp32) / bf16 (the persistent bf16-operand launch)."""
    ops = _ops()
    d = _make('lstm', b, t, h, seed, ragged, init, scale)
    v = d['dev']
    bf = form == 'bf16'
    label = 'lstm %s (%d,%d,%d)%s%s' % (form, b, t, h, '' if ragged else ' seq_len=None', '' if init else ' no h0/c0/grad_hn/grad_cn')
    if bf:
        out, hstate, cstate, saved, hstate_bf = ops.lstm_fwd_bf16(v['xproj'], v['w_hh'], v['b_hh'], v['seq_len'], v['h0'], v['c0'], b, t, h)
        assert np.array_equal(_bits(hstate_bf), ref.bf16_bits(_host(hstate))), label + ': hstate_bf != bf16(hstate)'
        w_op, h_op = ref.bf16_round(d['w_hh']), _host(hstate_bf)
    else:
        out, hstate, cstate, saved = ops.lstm_fwd(v['xproj'], v['w_hh'], v['b_hh'], v['seq_len'], v['h0'], v['c0'], b, t, h, persistent=form == 'persist')
        w_op, h_op = d['w_hh'], _host(hstate)
    hs_h, cs_h, sv_h, out_h = _host(hstate), _host(cstate), _host(saved), _host(out)
    for got, init_v in ((hs_h, d['h0']), (cs_h, d['c0'])):
        assert np.array_equal(got[:, 0], init_v if init_v is not None else np.zeros_like(got[:, 0]))
    fwd = ref.lstm_forward_residual(label + ' forward', d['xproj'], w_op, d['b_hh'], d['seq_len'], hs_h, h_op, cs_h, out_h, sv_h, fast=bf)
    if bf:
        dg, dh0, dc0, dg_bf = ops.lstm_bwd_bf16(v['grad_out'], v['grad_hn'], v['grad_cn'], cstate, saved, v['w_hh'], v['seq_len'], b, t, h)
        assert np.array_equal(_bits(dg_bf), ref.bf16_bits(_host(dg))), label + ': dgates_bf != bf16(dgates)'
        none, dh02, dc02, dg_bf2 = ops.lstm_bwd_bf16(v['grad_out'], v['grad_hn'], v['grad_cn'], cstate, saved, v['w_hh'], v['seq_len'], b, t, h,
                                                     want_f32=False)
        assert none is None and np.array_equal(_bits(dg_bf2), _bits(dg_bf))
        assert np.array_equal(_host(dh02), _host(dh0)) and np.array_equal(_host(dc02), _host(dc0)), label + ': want_f32=False'
        operand = _host(dg_bf)
    else:
        dg, dh0, dc0 = ops.lstm_bwd(v['grad_out'], v['grad_hn'], v['grad_cn'], cstate, saved, v['w_hh'], v['seq_len'], b, t, h, persistent=form == 'persist')
        operand = _host(dg)
    bwd = ref.lstm_backward_residual(label + ' backward', d['grad_out'], d['grad_hn'], d['grad_cn'], cs_h, sv_h, w_op, d['seq_len'], _host(dg), operand,
                                     _host(dh0), _host(dc0), fast=bf)
    _settle([fwd, bwd], finite=(out_h, hs_h, cs_h, _host(dg), _host(dh0), _host(dc0)))


@pytest.mark.parametrize('variant', VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize('shape', GRU_STEP_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_lstm_f32_step(shape, variant):
    _lstm_case('step', *shape, seed=1 + sum(shape), ragged=variant[1], init=variant[2])


def test_lstm_f32_step_saturated():
    _lstm_case('step', 33, 12, 256, seed=8, ragged=True, init=True, scale=40.0)


@pytest.mark.parametrize('variant', VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize('shape', [(64, 30, 512), (100, 7, 320)], ids=lambda s: '%dx%dx%d' % s)
def test_lstm_f32_persistent(shape, variant):
    if not _ops().lstm_persist_f32_ok(*shape):
        pytest.skip('mg_lstm_persist_f32_supported(%d, %d, %d) == 0' % shape)
    _lstm_case('persist', *shape, seed=1 + sum(shape), ragged=variant[1], init=variant[2])


@pytest.mark.parametrize('variant', VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize('shape', [(33, 20, 256), (12, 15, 384), (64, 40, 512)], ids=lambda s: '%dx%dx%d' % s)
def test_lstm_bf16_persistent(shape, variant):
    if not _ops().lstm_persist_ok(*shape):
        pytest.skip('mg_lstm_persist_supported(%d, %d, %d) == 0' % shape)
    _lstm_case('bf16', *shape, seed=1 + sum(shape), ragged=variant[1], init=variant[2])


def test_lstm_bf16_saturated():
    if not _ops().lstm_persist_ok(33, 20, 256):
        pytest.skip('mg_lstm_persist_supported(33, 20, 256) == 0')
    _lstm_case('bf16', 33, 20, 256, seed=9, ragged=True, init=True, scale=40.0)


def test_lstm_f32_misaligned_views():
    """w_hh, hstate and dgates as 4-byte-offset views (C ABI): lstm_ld4's scalar path by alignment."""
    torch, ops = _torch(), _ops()
    b, t, h = 9, 7, 256
    d = _make('lstm', b, t, h, 41)
    v = d['dev']
    lib, p = ops._lib.load(), ops._p
    w = _offset_view(v['w_hh'], torch)
    hs0 = torch.zeros((b, t + 1, h), dtype=torch.float32, device=DEV)
    hs0[:, 0] = v['h0']
    hstate = _offset_view(hs0, torch)
    cstate = torch.zeros((b, t + 1, h), dtype=torch.float32, device=DEV)
    cstate[:, 0] = v['c0']
    out = torch.empty((b, t, h), dtype=torch.float32, device=DEV)
    saved = torch.empty((b, t, 4 * h), dtype=torch.float32, device=DEV)
    ops._lib.check(lib.mg_lstm_fwd_f32(p(v['xproj']), p(w), p(v['b_hh']), p(v['seq_len']), b, t, h, p(hstate), p(cstate), p(out), p(saved),
                                       ops._stream()), 'mg_lstm_fwd_f32')
    dg = _offset_view(torch.zeros((b, t, 4 * h), dtype=torch.float32, device=DEV), torch)
    dh0 = torch.empty((b, h), dtype=torch.float32, device=DEV)
    dc0 = torch.empty((b, h), dtype=torch.float32, device=DEV)
    ws = torch.empty(lib.mg_lstm_bwd_workspace_bytes(b, h), dtype=torch.uint8, device=DEV)
    ops._lib.check(lib.mg_lstm_bwd_f32(p(v['grad_out']), p(v['grad_hn']), p(v['grad_cn']), p(cstate), p(saved), p(w), p(v['seq_len']), b, t, h, p(dg),
                                       p(dh0), p(dc0), p(ws), ws.numel(), ops._stream()), 'mg_lstm_bwd_f32')
    hs_h, cs_h, sv_h = _host(hstate), _host(cstate), _host(saved)
    fwd = ref.lstm_forward_residual('lstm step misaligned forward', d['xproj'], d['w_hh'], d['b_hh'], d['seq_len'], hs_h, hs_h, cs_h, _host(out), sv_h)
    bwd = ref.lstm_backward_residual('lstm step misaligned backward', d['grad_out'], d['grad_hn'], d['grad_cn'], cs_h, sv_h, d['w_hh'], d['seq_len'],
                                     _host(dg), _host(dg), _host(dh0), _host(dc0))
    _settle([fwd, bwd], finite=(_host(dg), _host(dh0), _host(dc0)))


# ------------------------------------------------------------------------------------------------------------------ stacks
def _stack_weights(g, h, n_layers, seed):
    rng = np.random.RandomState(seed)
    mk = lambda: (rng.uniform(-1, 1, (g * h, h)) / np.sqrt(h)).astype(np.float32)
    bias = lambda: rng.uniform(-0.5, 0.5, g * h).astype(np.float32)
    return [mk() for _ in range(n_layers)], [mk() for _ in range(n_layers)], [bias() for _ in range(n_layers)], [bias() for _ in range(n_layers)]


def _projection_all(below, w_ih, b_ih, b, t):
    """The in-step input projections of a stacked layer for all steps: (value, magnitude sum), each [B,T,G]."""
    val, mag = ref.in_step_projection(below.reshape(b * t, -1), w_ih, b_ih)
    return val.reshape(b, t, -1), mag.reshape(b, t, -1)


def _handed_down_all(gates_operand, w_ih_above, b, t):
    g = ref.handed_down_gradient(gates_operand.reshape(b * t, -1), w_ih_above)
    return g.v.reshape(b, t, -1), g.e.reshape(b, t, -1)


@pytest.mark.parametrize('fast', [False, True], ids=['exact', 'fast'])
def test_gru_small_stack(fast):
    """(13, 57, 64) x 3 layers: layer l >= 1 forms its input projection inside the step from the stored ``out`` of the layer below (K = 2H in
    the bound) and hands dxproj W_ih down.  fast: the operands (state, lower layer's output, gate gradients, W) rounded to bf16."""
    ops = _ops()
    b, t, h, n_layers = 13, 57, 64, 3
    if not ops.gru_stack_small_ok(b, t, h, n_layers):
        pytest.skip('mg_gru_stack_small_supported(%d, %d, %d, %d) == 0' % (b, t, h, n_layers))
    rnd = ref.bf16_round if fast else (lambda a: a)
    d = _make('gru', b, t, h, 91)
    v = d['dev']
    w_ih, w_hh, b_ih, b_hh = _stack_weights(3, h, n_layers, 92)
    rng = np.random.RandomState(93)
    h0s = (0.5 * rng.randn(n_layers, b, h)).astype(np.float32)
    ghn = rng.randn(n_layers, b, h).astype(np.float32)
    dv = lambda xs: [_dev(x) for x in xs]
    w_ih_d, w_hh_d, b_ih_d, b_hh_d = dv(w_ih), dv(w_hh), dv(b_ih), dv(b_hh)
    outs, hstates, saveds = ops.gru_stack_small_fwd(v['xproj'], w_ih_d, w_hh_d, b_ih_d, b_hh_d, v['seq_len'], _dev(h0s), b, t, h, fast=fast)
    dxps, dhps, dh0 = ops.gru_stack_small_bwd(v['grad_out'], [_dev(g) for g in ghn], hstates, saveds, w_ih_d, w_hh_d, v['seq_len'], b, t, h, fast=fast)
    results = []
    name = 'gru small stack %s (%d,%d,%d) x %d' % ('fast' if fast else 'exact', b, t, h, n_layers)
    go, go_err = d['grad_out'], None
    for l in range(n_layers):
        hs_h = _host(hstates[l])
        if l == 0:
            xp, mag = d['xproj'], None
        else:
            xp, mag = _projection_all(rnd(_host(outs[l - 1])), rnd(w_ih[l]), b_ih[l], b, t)
        results.append(ref.gru_forward_residual('%s layer %d forward' % (name, l), xp, rnd(w_hh[l]), b_hh[l], d['seq_len'], hs_h, rnd(hs_h),
                                                _host(outs[l]), _host(saveds[l]), fast=fast, xproj_mag=mag))
    for l in range(n_layers - 1, -1, -1):
        dxp_h, dhp_h = _host(dxps[l]), _host(dhps[l])
        results.append(ref.gru_backward_residual('%s layer %d backward' % (name, l), go, ghn[l], _host(hstates[l]), _host(saveds[l]), rnd(w_hh[l]),
                                                 d['seq_len'], dxp_h, dhp_h, rnd(dhp_h), _host(dh0[l]), grad_out_err=go_err))
        if l > 0:
            go, go_err = _handed_down_all(rnd(dxp_h), rnd(w_ih[l]), b, t)
    _settle(results, finite=[_host(x) for x in dxps + dhps] + [_host(dh0)])


@pytest.mark.parametrize('shape', [(20, 30, 128, 3), (64, 24, 512, 8)], ids=lambda s: '%dx%dx%dx%d' % s)
def test_lstm_pstack(shape):
    """The whole-stack bf16 wavefronts: layer l >= 1's input projection from the stored hstate_bf of the layer below (K = 2H), the gate
    gradients handed down through bf16(W_ih) of the layer above."""
    ops = _ops()
    b, t, h, n_layers = shape
    if not ops.lstm_pstack_ok(b, t, h, n_layers):
        pytest.skip('mg_lstm_pstack_supported(%d, %d, %d, %d) == 0' % shape)
    if not ops.lstm_pstack_bwd_ok(b, t, h, n_layers):
        pytest.skip('mg_lstm_pstack_bwd_supported(%d, %d, %d, %d) == 0' % shape)
    rnd = ref.bf16_round
    d = _make('lstm', b, t, h, 101 + h)
    v = d['dev']
    w_ih, w_hh, b_ih, b_hh = _stack_weights(4, h, n_layers, 102)
    rng = np.random.RandomState(103)
    h0s, c0s = ((0.5 * rng.randn(n_layers, b, h)).astype(np.float32) for _ in range(2))
    ghn, gcn = (rng.randn(n_layers, b, h).astype(np.float32) for _ in range(2))
    dv = lambda xs: [_dev(x) for x in xs]
    w_ih_d, w_hh_d, b_ih_d, b_hh_d = dv(w_ih), dv(w_hh), dv(b_ih), dv(b_hh)
    out, hstate, cstate, saved, hstate_bf = ops.lstm_pstack_fwd(v['xproj'], w_ih_d, w_hh_d, b_ih_d, b_hh_d, v['seq_len'], _dev(h0s), _dev(c0s), b, t, h)
    dgs, dg_bfs, dh0, dc0 = ops.lstm_pstack_bwd(v['grad_out'], dv(ghn), dv(gcn), cstate, saved, w_ih_d, w_hh_d, v['seq_len'], b, t, h, want_f32=True)
    name = 'lstm pstack (%d,%d,%d) x %d' % shape
    results = []
    for l in range(n_layers):
        hb = _host(hstate_bf[l])
        if l == 0:
            xp, mag = d['xproj'], None
        else:
            xp, mag = _projection_all(_host(hstate_bf[l - 1])[:, 1:], rnd(w_ih[l]), b_ih[l], b, t)
        results.append(ref.lstm_forward_residual('%s layer %d forward' % (name, l), xp, rnd(w_hh[l]), b_hh[l], d['seq_len'], None, hb, _host(cstate[l]),
                                                 _host(out) if l == n_layers - 1 else None, _host(saved[l]), fast=True, xproj_mag=mag,
                                                 hstate_rows_valid=False))
        assert np.array_equal(ref.bf16_bits(_host(hstate[l])[:, t]), _bits(hstate_bf[l])[:, t]), '%s layer %d: h_n' % (name, l)
    go, go_err = d['grad_out'], None
    for l in range(n_layers - 1, -1, -1):
        assert np.array_equal(_bits(dg_bfs[l]), ref.bf16_bits(_host(dgs[l]))), '%s layer %d: dgates_bf != bf16(dgates)' % (name, l)
        operand = _host(dg_bfs[l])
        results.append(ref.lstm_backward_residual('%s layer %d backward' % (name, l), go, ghn[l], gcn[l], _host(cstate[l]), _host(saved[l]),
                                                  rnd(w_hh[l]), d['seq_len'], _host(dgs[l]), operand, _host(dh0[l]), _host(dc0[l]),
                                                  grad_out_err=go_err, fast=True))
        if l > 0:
            go, go_err = _handed_down_all(operand, rnd(w_ih[l]), b, t)
    _settle(results, finite=[_host(x) for x in dgs] + [_host(dh0), _host(dc0)])


@pytest.mark.parametrize('lag', [1, 4])
def test_lstm_skewed_stack(lag):
    """mg_lstm_stack_fwd_f32 / _bwd_f32 at (9, 33, 128) x 2: one launch per step serves both layers, layer 1 ``lag`` steps behind.  The entry
    points take every layer's input projections and output gradients from the caller, so each layer is given its own."""
    torch, ops = _torch(), _ops()
    from morgana_amd import _lib
    b, t, h, n_layers = 9, 33, 128, 2
    ds = [_make('lstm', b, t, h, 111 + l) for l in range(n_layers)]
    seq, seq_d = ds[0]['seq_len'], ds[0]['dev']['seq_len']
    keep = []
    fd = (_lib.mg_lstm_fwd_layer * n_layers)()
    bufs = []
    for l, d in enumerate(ds):
        v = d['dev']
        hs = torch.zeros((b, t + 1, h), dtype=torch.float32, device=DEV)
        cs = torch.zeros((b, t + 1, h), dtype=torch.float32, device=DEV)
        hs[:, 0], cs[:, 0] = v['h0'], v['c0']
        out = torch.empty((b, t, h), dtype=torch.float32, device=DEV)
        sv = torch.empty((b, t, 4 * h), dtype=torch.float32, device=DEV)
        fd[l].xproj, fd[l].x_T, fd[l].x_t0 = v['xproj'].data_ptr(), t, 0
        fd[l].w_hh, fd[l].b_hh = v['w_hh'].data_ptr(), v['b_hh'].data_ptr()
        fd[l].hstate, fd[l].cstate, fd[l].out, fd[l].saved = hs.data_ptr(), cs.data_ptr(), out.data_ptr(), sv.data_ptr()
        bufs.append((hs, cs, out, sv))
    ops.lstm_stack_fwd(fd, n_layers, seq_d, b, t, h, lag, 0, t + (n_layers - 1) * lag)
    bd = (_lib.mg_lstm_bwd_layer * n_layers)()
    grads = []
    for l, d in enumerate(ds):
        v = d['dev']
        hs, cs, out, sv = bufs[l]
        dg = torch.empty((b, t, 4 * h), dtype=torch.float32, device=DEV)
        carry_h, carry_c = v['grad_hn'].clone(), v['grad_cn'].clone()
        dh0 = torch.empty((b, h), dtype=torch.float32, device=DEV)
        dc0 = torch.empty((b, h), dtype=torch.float32, device=DEV)
        bd[l].grad_out, bd[l].g_T, bd[l].g_t0 = v['grad_out'].data_ptr(), t, 0
        bd[l].cstate, bd[l].saved, bd[l].w_hh, bd[l].dgates = cs.data_ptr(), sv.data_ptr(), v['w_hh'].data_ptr(), dg.data_ptr()
        bd[l].carry_h, bd[l].carry_c, bd[l].dh0, bd[l].dc0 = carry_h.data_ptr(), carry_c.data_ptr(), dh0.data_ptr(), dc0.data_ptr()
        keep += [carry_h, carry_c]
        grads.append((dg, dh0, dc0))
    t_pad = -(-t // lag) * lag
    ops.lstm_stack_bwd(bd, n_layers, seq_d, b, t, h, lag, 0, t_pad + (n_layers - 1) * lag + 1)
    results = []
    for l, d in enumerate(ds):
        hs, cs, out, sv = (_host(x) for x in bufs[l])
        dg, dh0, dc0 = (_host(x) for x in grads[l])
        name = 'lstm skewed stack lag %d (%d,%d,%d) layer %d' % (lag, b, t, h, l)
        results.append(ref.lstm_forward_residual(name + ' forward', d['xproj'], d['w_hh'], d['b_hh'], seq, hs, hs, cs, out, sv))
        results.append(ref.lstm_backward_residual(name + ' backward', d['grad_out'], d['grad_hn'], d['grad_cn'], cs, sv, d['w_hh'], seq, dg, dg, dh0, dc0))
    _settle(results, finite=[_host(g[0]) for g in grads])


# ------------------------------------------------------------------------------------------------------------------ fast cell
def test_fast_cell_accuracy():
    """mg_sigmoid_fast and the tanh form 2 s(2x) - 1 (gru_cell.h) measured through the bf16 per-step GRU at T = 1 with W_hh = 0, b_hh = 0,
    h0 = 0: ``saved`` is then s(x_r), s(x_z), tanh(x_n) of the inputs.  The header's claim: <= 2e-7 absolute for the sigmoid, hence <= 4e-7
    for the tanh form; all finite; exactly 0 / 1 / +-1 where the float32 result saturates (s: x >= 20 -> 1, x <= -104 -> 0, below the
    smallest subnormal; tanh: |x| >= 10)."""
    torch, ops = _torch(), _ops()
    b, h = 1024, 128
    n = b * h
    sweep = np.linspace(-100.0, 100.0, n - 16).astype(np.float32)
    edge = np.array([88.7, -88.7, 89.0, -89.0, 1e4, -1e4, np.inf, -np.inf, 0.0, -0.0, 20.0, -104.0, 10.0, -10.0, 87.3, -87.3], dtype=np.float32)
    x = np.concatenate([sweep, edge])
    xproj = np.stack([np.random.RandomState(s).permutation(x).reshape(b, h) for s in range(3)], axis=1).reshape(b, 1, 3 * h)
    w = torch.zeros((3 * h, h), dtype=torch.float32, device=DEV)
    bias = torch.zeros(3 * h, dtype=torch.float32, device=DEV)
    _, hstate, saved, _ = ops.gru_fwd_bf16(_dev(xproj), w, bias, None, None, b, 1, h, persistent=False)
    sv = _host(saved)[:, 0].astype(np.float64)
    xs = xproj[:, 0].astype(np.float64)
    assert np.isfinite(sv).all() and np.isfinite(_host(hstate)).all()
    with np.errstate(over='ignore'):
        want_s = 1.0 / (1.0 + np.exp(-xs[:, :2 * h]))
    want_n = np.tanh(xs[:, 2 * h:])
    err_s = np.abs(sv[:, :2 * h] - want_s)
    err_n = np.abs(sv[:, 2 * h:3 * h] - want_n)
    parity_report.note(err_s.max(), 'mg_sigmoid_fast: max absolute error over [-100, 100] and the edges', bound=ref.FAST_SIGMOID_ABS)
    print('mg_sigmoid_fast: max abs error %.3g at x = %r; tanh form: %.3g at x = %r' % (
        err_s.max(), xs[:, :2 * h].flat[int(err_s.argmax())], err_n.max(), xs[:, 2 * h:].flat[int(err_n.argmax())]))
    assert err_s.max() <= ref.FAST_SIGMOID_ABS
    assert err_n.max() <= 2 * ref.FAST_SIGMOID_ABS
    s_got, s_x = sv[:, :2 * h], xs[:, :2 * h]
    assert np.all(s_got[s_x >= 20.0] == 1.0) and np.all(s_got[s_x <= -104.0] == 0.0)
    n_got, n_x = sv[:, 2 * h:3 * h], xs[:, 2 * h:]
    assert np.all(n_got[n_x >= 10.0] == 1.0) and np.all(n_got[n_x <= -10.0] == -1.0)
    assert not sv[:, 3 * h:].any()                                 # hn = W_hn h + b_hn = 0


# ------------------------------------------------------------------------------------------------------------------ free running
FREE_SHAPES = [(16, 50, 512), (33, 300, 256)]


def _free_reference(cell, bf, shape, on_device=True):
    """(inputs, float64 results, e_ref per output): e_ref = rel_err(float32 numpy run, float64 run), both with the same operand rounding."""
    b, t, h = shape
    d = _make(cell, b, t, h, 200 + h, on_device=on_device)
    rnd = ref.bf16_round if bf else None
    res = {}
    for dtype in (np.float64, np.float32):
        if cell == 'gru':
            out, hs, sv = ref.gru_run(d['xproj'], d['w_hh'], d['b_hh'], d['seq_len'], d['h0'], rnd, dtype)
            dxp, dhp, dh0 = ref.gru_run_bwd(d['grad_out'], d['grad_hn'], hs, sv, d['w_hh'], d['seq_len'], rnd, dtype)
            res[dtype] = {'out': out, 'h_n': hs[:, t], 'dgate': dxp, 'dh0': dh0}
        else:
            out, hs, cs, sv = ref.lstm_run(d['xproj'], d['w_hh'], d['b_hh'], d['seq_len'], d['h0'], d['c0'], rnd, dtype)
            dg, dh0, dc0 = ref.lstm_run_bwd(d['grad_out'], d['grad_hn'], d['grad_cn'], cs, sv, d['w_hh'], d['seq_len'], rnd, dtype)
            res[dtype] = {'out': out, 'h_n': hs[:, t], 'dgate': dg, 'dh0': dh0}
    e_ref = {k: ref.rel_err(res[np.float32][k], res[np.float64][k]) for k in res[np.float64]}
    return d, res[np.float64], e_ref


@pytest.mark.parametrize('shape', FREE_SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('cell', ['gru', 'lstm'])
def test_free_running_trajectory(cell, precision, shape):
    ops = _ops()
    b, t, h = shape
    bf = precision == 'bf16'
    d, want, e_ref = _free_reference(cell, bf, shape)
    v = d['dev']
    if cell == 'gru':
        if bf:
            out, hs, sv, _ = ops.gru_fwd_bf16(v['xproj'], v['w_hh'], v['b_hh'], v['seq_len'], v['h0'], b, t, h)
            dxp, _, dh0, _ = ops.gru_bwd_bf16(v['grad_out'], v['grad_hn'], hs, sv, v['w_hh'], v['seq_len'], b, t, h)
        else:
            out, hs, sv = ops.gru_fwd(v['xproj'], v['w_hh'], v['b_hh'], v['seq_len'], v['h0'], b, t, h)
            dxp, _, dh0 = ops.gru_bwd(v['grad_out'], v['grad_hn'], hs, sv, v['w_hh'], v['seq_len'], b, t, h)
    else:
        if bf:
            if not ops.lstm_persist_ok(b, t, h):
                pytest.skip('mg_lstm_persist_supported(%d, %d, %d) == 0' % shape)
            out, hs, cs, sv, _ = ops.lstm_fwd_bf16(v['xproj'], v['w_hh'], v['b_hh'], v['seq_len'], v['h0'], v['c0'], b, t, h)
            dxp, dh0, _, _ = ops.lstm_bwd_bf16(v['grad_out'], v['grad_hn'], v['grad_cn'], cs, sv, v['w_hh'], v['seq_len'], b, t, h)
        else:
            out, hs, cs, sv = ops.lstm_fwd(v['xproj'], v['w_hh'], v['b_hh'], v['seq_len'], v['h0'], v['c0'], b, t, h)
            dxp, dh0, _ = ops.lstm_bwd(v['grad_out'], v['grad_hn'], v['grad_cn'], cs, sv, v['w_hh'], v['seq_len'], b, t, h)
    got = {'out': _host(out), 'h_n': _host(hs)[:, t], 'dgate': _host(dxp), 'dh0': _host(dh0)}
    worst = 0.0
    for key in sorted(got):
        err = ref.rel_err(got[key], want[key])
        print('%s %s %s %s: kernel %.3g, e_ref %.3g (%.2f x)' % (cell, precision, shape, key, err, e_ref[key], err / e_ref[key]))
        parity_report.note(err / e_ref[key], '%s: kernel rel err / e_ref' % key, bound=FREE_FACTOR)
        worst = max(worst, err / e_ref[key])
    assert worst <= FREE_FACTOR


if __name__ == '__main__':      # the e_ref table of the module docstring (CPU only)
    print('    case                      out      h_n      dgate    dh0')
    for cell_ in ('gru', 'lstm'):
        for bf_ in (False, True):
            for shape_ in FREE_SHAPES:
                e = _free_reference(cell_, bf_, shape_, on_device=False)[2]
                print('    %-4s %s %-13s %s' % (cell_, 'bf16' if bf_ else 'fp32', '(%d,%d,%d)' % shape_, '  '.join('%.1e' % e[k] for k in ('out', 'h_n', 'dgate', 'dh0'))))
