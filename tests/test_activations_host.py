"""CPU-only checks of nn.Tanh / nn.ReLU as activations of a fused Linear run (reference: the modules SequentialWithRecurrent.forward
runs one by one, morgana/utils.py:401-418): the container collects them into the run as it collects nn.Sigmoid, the new C-ABI entry
points exist and validate their arguments on the host, the forward entry points accept the new ``act`` values, and every
shape-specialised Sigmoid fusion declines them (such stacks take the generic kernels)."""
import torch
import torch.nn as nn

from morgana_amd import _lib, ops, utils

NEW_SYMBOLS = ('mg_linear_dgrad_act_f32', 'mg_linear_dgrad_act_bf16', 'mg_act_f32', 'mg_act_grad_f32')


def test_linear_run_collects_tanh_and_relu_like_sigmoid():
    mods = [nn.Linear(6, 5), nn.Tanh(), nn.Dropout(0.), nn.Linear(5, 4), nn.ReLU(inplace=True), nn.Linear(4, 3)]
    net = utils.SequentialWithRecurrent(*mods)
    end, run = net._linear_run(list(net._modules.values()), 0)
    assert end == len(mods) and len(run) == 3
    assert tuple(act for _, act in run) == (ops.ACT_TANH, ops.ACT_RELU, ops.ACT_NONE)
    assert [lin for lin, _ in run] == [mods[0], mods[3], mods[5]]
    assert run.drops == (0., 0., 0.)
    # an active dropout behind the activation stays inside the run, as behind a Sigmoid
    net = utils.SequentialWithRecurrent(nn.Linear(6, 5), nn.ReLU(), nn.Dropout(0.2), nn.Linear(5, 4), nn.Tanh(), nn.Linear(4, 1))
    net.train()
    end, run = net._linear_run(list(net._modules.values()), 0)
    assert end == 6 and tuple(act for _, act in run) == (ops.ACT_RELU, ops.ACT_TANH, ops.ACT_NONE)
    assert abs(run.drops[0] - 0.2) < 1e-12 and run.drops[1:] == (0., 0.)
    # subclasses and other activations are not taken for one of the three
    net = utils.SequentialWithRecurrent(nn.Linear(6, 5), nn.LeakyReLU(), nn.Linear(5, 4))
    end, run = net._linear_run(list(net._modules.values()), 0)
    assert end == 1 and tuple(act for _, act in run) == (ops.ACT_NONE,)


def test_node_specs_and_run_accessors():
    """The records the Linear-run nodes take as their first argument, and what a run hands them: defaults, keywords, and a
    two-activation ``acts`` that stays ``acts`` (a bare tuple of two could once be read as (acts, maps))."""
    from morgana_amd import functional as F_hip
    spec = F_hip.LinearStackSpec((ops.ACT_SIGMOID, ops.ACT_NONE), 'fp32')
    assert (spec.acts, spec.precision, spec.extra, spec.rows_runs) == ((ops.ACT_SIGMOID, ops.ACT_NONE), 'fp32', 0, False)
    assert spec.drop is None and spec.shadow is None and spec.front is None and spec.latent is None
    shadow = torch.zeros(2, 8, dtype=torch.bfloat16)
    spec = F_hip.LinearStackSpec(acts=(ops.ACT_TANH,), precision='bf16', latent=(6, 3), shadow=shadow, rows_runs=True)
    assert spec.latent == (6, 3) and spec.shadow is shadow and spec.rows_runs is True and spec.extra == 0 and spec.front is None
    assert spec._fields == ('acts', 'precision', 'extra', 'rows_runs', 'drop', 'shadow', 'front', 'latent')
    try:
        spec.extra = 1
        raise AssertionError('LinearStackSpec must be immutable')
    except AttributeError:
        pass

    mods = [nn.Linear(6, 5), nn.Tanh(), nn.Dropout(0.25), nn.Linear(5, 4, bias=False), nn.ReLU(), nn.Linear(4, 3)]
    net = utils.SequentialWithRecurrent(*mods)
    net.train()
    end, run = net._linear_run(list(net._modules.values()), 0)
    assert end == len(mods) and run.acts == (ops.ACT_TANH, ops.ACT_RELU, ops.ACT_NONE)
    want = [mods[0].weight, mods[0].bias, mods[3].weight, None, mods[5].weight, mods[5].bias]
    got = run.params()
    assert len(got) == len(want) and all(g is w for g, w in zip(got, want))
    got = run.params(-2)
    assert len(got) == 2 and got[0] is mods[0].weight and got[1] is mods[0].bias
    assert len(run.params(2)) == 4 and run.params(2)[3] is None
    assert run.drop_spec() == ((0.25, 0., 0.), 0)

    two = (ops.ACT_SIGMOID, ops.ACT_NONE)
    mse = F_hip.LinearStackMSESpec(two)
    assert mse.acts == two and mse.maps is None and mse.table_bf16 is None and mse.phone_rate is None and mse.pending is None
    assert mse._fields == ('acts', 'maps', 'table_bf16', 'phone_rate', 'pending')
    maps, holder = (torch.zeros(2, 3), torch.zeros(4)), object()
    mse = F_hip.LinearStackMSESpec(acts=two, maps=maps, phone_rate=True)
    assert mse.acts == two and mse.maps is maps and mse.phone_rate is True and mse.pending is None
    mse = F_hip.LinearStackMSESpec(two, pending=holder, table_bf16=shadow)
    assert mse.acts == two and mse.maps is None and mse.pending is holder and mse.table_bf16 is shadow
    # what forward unpacks: five fields in this order, whatever the length of acts
    acts, maps_, table, order, pending = mse
    assert (acts, maps_, order) == (two, None, None) and table is shadow and pending is holder


def test_activation_constants_follow_the_header():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'morgana_hip.h')).read()
    values = {name: int(v, 0) for name, v in re.findall(r'#define (MG_ACT_[A-Z_]+) (\w+)', header)}
    assert (values['MG_ACT_NONE'], values['MG_ACT_SIGMOID'], values['MG_ACT_TANH'], values['MG_ACT_RELU']) == (0, 1, 2, 3)
    assert (ops.ACT_NONE, ops.ACT_SIGMOID, ops.ACT_TANH, ops.ACT_RELU) == (0, 1, 2, 3)
    assert values['MG_ACT_RELU'] < values['MG_ACT_ROWS_RUNS']          # the hint is OR-ed into act


def test_new_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), 'libmorgana_hip.so does not export %s' % name
    for name in ('act', 'act_grad', 'linear_dgrad_f32', 'linear_dgrad_bf16'):
        assert callable(getattr(ops, name))


def test_forward_entry_points_accept_tanh_and_relu_and_refuse_others():
    """Fake (never dereferenced) addresses: the host validation runs before any launch.  With act = 2 / 3 and another bad argument
    the message names the other argument; act = 4 is refused by name."""
    lib = _lib.load()
    for act in (ops.ACT_TANH, ops.ACT_RELU):
        # lda = 8 < K = 16
        assert lib.mg_linear_fwd_f32(16, 8, None, 4, 16, 16, None, 8, 16, 8, act, None) == -1
        assert 'unknown activation' not in _lib.last_error() and 'lda=8' in _lib.last_error()
        # ldy = 12 is no multiple of 8
        assert lib.mg_linear_fwd_bf16(16, 16, None, 4, 16, 16, 16, None, 8, 16, 12, 0, act, None) == -1
        assert 'unknown activation' not in _lib.last_error() and 'ldy=12' in _lib.last_error()
        assert lib.mg_linear_fwd_bf16(16, 16, None, 4, 16, 16, 16, None, 8, 16, 12, 0, act | 0x100, None) == -1
        assert 'unknown activation' not in _lib.last_error()
        # nothing to do: no launch, and the activation passed the check
        assert lib.mg_linear_fwd_f32(16, 16, None, 0, 16, 16, None, 8, 16, 8, act, None) == 0
        assert lib.mg_linear_fwd_bf16(16, 16, None, 0, 16, 16, 16, None, 8, 16, 8, 0, act, None) == 0
        # mg_phone_concat_layer_bf16: C = 17 frame features are refused, the activation is not
        assert lib.mg_phone_concat_layer_bf16(16, 512, 16, 8, 16, 17, 16, 640, 600, None, 512, act, 32, 512, 0, None) == -1
        assert 'C=17' in _lib.last_error()
    assert lib.mg_linear_fwd_f32(16, 16, None, 4, 16, 16, None, 8, 16, 8, 4, None) == -1
    assert 'unknown activation 4' in _lib.last_error()
    assert lib.mg_linear_fwd_bf16(16, 16, None, 4, 16, 16, 16, None, 8, 16, 8, 0, 4, None) == -1
    assert 'unknown activation 4' in _lib.last_error()
    assert lib.mg_phone_concat_layer_bf16(16, 512, 16, 8, 16, 9, 16, 640, 600, None, 512, 4, 32, 512, 0, None) == -1
    assert 'act=4' in _lib.last_error()


def test_new_entry_points_validate_their_arguments():
    lib = _lib.load()
    # mg_linear_dgrad_act_f32(dY, M, N, W, K, H, act, dX, stream)
    assert lib.mg_linear_dgrad_act_f32(16, 4, 8, 16, 8, 16, 4, 16, None) == -1 and 'unknown activation 4' in _lib.last_error()
    assert lib.mg_linear_dgrad_act_f32(None, 4, 8, 16, 8, 16, ops.ACT_TANH, 16, None) == -1 and 'mg_linear_dgrad_act_f32' in _lib.last_error()
    assert lib.mg_linear_dgrad_act_f32(16, 4, 8, 16, 8, 16, ops.ACT_RELU, None, None) == -1
    assert lib.mg_linear_dgrad_act_f32(16, 4, 8, 16, 8, None, ops.ACT_TANH, 16, None) == -1 and 'needs its output H' in _lib.last_error()
    assert lib.mg_linear_dgrad_act_f32(16, 0, 8, 16, 8, 16, ops.ACT_TANH, 16, None) == 0            # no rows: no launch
    # mg_linear_dgrad_act_bf16(dY, lddy, M, N, WT, ldwt, K, H, ldh, act, dX, lddx, dx_f32, stream)
    assert lib.mg_linear_dgrad_act_bf16(16, 8, 4, 8, 16, 8, 8, 16, 8, 4, 16, 8, 0, None) == -1 and 'unknown activation 4' in _lib.last_error()
    assert lib.mg_linear_dgrad_act_bf16(None, 8, 4, 8, 16, 8, 8, 16, 8, ops.ACT_RELU, 16, 8, 0, None) == -1
    assert 'mg_linear_dgrad_act_bf16' in _lib.last_error()
    assert lib.mg_linear_dgrad_act_bf16(16, 8, 4, 8, 16, 8, 8, None, 0, ops.ACT_RELU, 16, 8, 0, None) == -1
    assert 'needs its output H' in _lib.last_error()
    assert lib.mg_linear_dgrad_act_bf16(16, 8, 4, 8, 16, 8, 8, 16, 12, ops.ACT_TANH, 16, 8, 0, None) == -1 and 'ldh=12' in _lib.last_error()
    assert lib.mg_linear_dgrad_act_bf16(16, 8, 4, 8, 16, 8, 8, 24, 8, ops.ACT_TANH, 16, 8, 0, None) == -1 and '16-byte' in _lib.last_error()
    assert lib.mg_linear_dgrad_act_bf16(16, 8, 0, 8, 16, 8, 8, 16, 8, ops.ACT_TANH, 16, 8, 0, None) == 0
    # mg_act_f32(x, y, n, act, stream) / mg_act_grad_f32(dy, y, dx, n, act, stream)
    assert lib.mg_act_f32(16, 16, 8, 4, None) == -1 and 'unknown activation 4' in _lib.last_error()
    assert lib.mg_act_f32(16, 16, 8, ops.ACT_NONE, None) == -1 and 'unknown activation 0' in _lib.last_error()
    assert lib.mg_act_f32(None, 16, 8, ops.ACT_TANH, None) == -1 and 'mg_act_f32' in _lib.last_error()
    assert lib.mg_act_f32(16, None, 8, ops.ACT_RELU, None) == -1
    assert lib.mg_act_f32(16, 16, 0, ops.ACT_RELU, None) == 0
    assert lib.mg_act_grad_f32(16, 16, 16, 8, 4, None) == -1 and 'unknown activation 4' in _lib.last_error()
    assert lib.mg_act_grad_f32(16, None, 16, 8, ops.ACT_TANH, None) == -1 and 'mg_act_grad_f32' in _lib.last_error()
    assert lib.mg_act_grad_f32(None, 16, 16, 8, ops.ACT_TANH, None) == -1
    assert lib.mg_act_grad_f32(16, 16, None, 8, ops.ACT_SIGMOID, None) == -1
    assert lib.mg_act_grad_f32(16, 16, 16, 0, ops.ACT_SIGMOID, None) == 0
    # the Sigmoid forms keep their own names in their messages
    assert lib.mg_linear_dgrad_f32(None, 4, 8, 16, 8, None, 16, None) == -1 and 'mg_linear_dgrad_f32:' in _lib.last_error()
    assert lib.mg_linear_dgrad_bf16(16, 8, 4, 8, 16, 8, 8, 16, 12, 16, 8, 0, None) == -1 and 'mg_linear_dgrad_bf16:' in _lib.last_error()


def _readme_stack(act_module, precision):
    dims = (600, 512, 128, 32, 1)
    mods = []
    for i in range(4):
        mods.append(nn.Linear(dims[i], dims[i + 1]))
        if i < 3:
            mods.append(act_module())
    return utils.SequentialWithRecurrent(*mods, precision=precision)


def test_sigmoid_only_fusions_decline_tanh_and_relu():
    """At the C2 shapes (20,480 phone rows, 256,000 frames, 600 -> 512 -> 128 -> 32 -> 1) every F0Model-shaped fusion takes the
    Sigmoid stack and declines the same stack with Tanh or ReLU."""
    assert ops.phone_rate_table_ok(20480, 256000, 512, 128, ops.ACT_SIGMOID, enabled=True)
    for act in (ops.ACT_TANH, ops.ACT_RELU, ops.ACT_NONE):
        assert not ops.phone_rate_table_ok(20480, 256000, 512, 128, act, enabled=True)
    targets = torch.zeros(2, 10, 1)
    sig = _readme_stack(nn.Sigmoid, 'bf16')
    assert sig._fused_mse_spec(targets, 'bf16') is not None
    lins = [m for m in sig if isinstance(m, nn.Linear)]
    assert ops.l2tail_ok(lins[1].weight, lins[2].weight, lins[3].weight, ops.ACT_SIGMOID)
    for module, act in ((nn.Tanh, ops.ACT_TANH), (nn.ReLU, ops.ACT_RELU)):
        net = _readme_stack(module, 'bf16')
        assert net._fused_mse_spec(targets, 'bf16') is None
        assert not ops.l2tail_ok(lins[1].weight, lins[2].weight, lins[3].weight, act)
        for precision in ('fp32', 'bf16x3'):
            assert _readme_stack(module, precision)._readme_tail(targets, precision) is None
        assert _readme_stack(nn.Sigmoid, 'fp32')._readme_tail(targets, 'fp32') is not None
    # one swapped activation anywhere in the stack is enough
    mixed = utils.SequentialWithRecurrent(nn.Linear(600, 512), nn.Tanh(), nn.Linear(512, 128), nn.Sigmoid(), nn.Linear(128, 32), nn.Sigmoid(),
                                          nn.Linear(32, 1), precision='bf16')
    assert mixed._fused_mse_spec(targets, 'bf16') is None
    # ... except in FRONT of the exact-fp32 tail, whose leading layers run through the generic node with any activation
    found = utils.SequentialWithRecurrent(nn.Linear(600, 512), nn.Tanh(), nn.Linear(512, 128), nn.Sigmoid(), nn.Linear(128, 32), nn.Sigmoid(),
                                          nn.Linear(32, 1), precision='fp32')._readme_tail(targets, 'fp32')
    assert found is not None and found[0][0][1] == ops.ACT_TANH
