"""The three ways a backward pass of the fused stack nodes hands its parameter gradients over (functional._grad_sink,
'defer' / 'direct' / 'temp') on models.F0Model, precisions 'bf16' (functional.LinearStackMSEFn, both orders of operations) and 'bf16x3'
(functional.F0StackX3Fn), eager and captured (``-m gpu``, MI355X): the entry points of a step under _lib.CALL_LOG, written out per
configuration, and bit equality of losses, prediction, parameters and both Adam moments between hand-overs.

Batches: synthetic.make_batch(32, 480, seed=6, frames_per_phone=5.0) with the loader's tables - 3072 table rows + 1024 extra = 4096
rows, 15 360 frames: the smallest batch that takes the fused phone-rate step (tests/test_gpu_phone_step_ref64.py), ops.x3_step_ok and,
at frame rate, ops.can_fuse_bwd - and synthetic.make_batch(16, 400, seed=21) under the 600-512-512-512-128-32-1 stack that registers
more slab sources than the update kernel's plan holds.

Hand-overs: ``defer`` = optim.Adam(fused_loop=True) + functional.backward; ``direct`` = optim.Adam(fused_loop=False) +
functional.backward; ``flat`` = optim.Adam + plain loss.backward() ('temp' that ends in one fused add into the optimiser's buffer);
``torch`` = torch.optim.Adam + loss.backward() ('temp' as tensors).  An eager case is the third step of three; a ``graph`` case is
graphs.GraphedTrainStep(warmup=2) - which switches the optimiser's fused loop ON, so its ``direct`` row captures the same step as
its ``defer`` row - followed by three replays.  ``hook``: a recording callable installed with functional.set_early_grads_hook; the entry
'EARLY' marks where it fired.  ``riders``: MORGANA_TAIL_RIDERS; ``fuse2``: MORGANA_FUSE_WGRAD2.

What is equal, as measured on the commit before the hand-over was given one interface and asserted here:
* ``defer``, ``direct`` and ``flat`` of one precision, order and launch set are EQUAL bit for bit - with and without the hook at
  phone rate; at frame rate the hook (like MORGANA_FUSE_WGRAD2=0) takes the one-launch backward of both layers away, and those
  five cases are equal among themselves.  Captured: ``defer``, ``direct`` and the rider form are equal.
* ``torch`` is merely close (the third loss differs in the last place: torch.optim.Adam's update is other arithmetic) and is left out
  of the equality assertion; its entry points are pinned.
* 'bf16x3' fires the hook in ``direct`` only: in ``flat`` its slab sums run when the node is done, so nothing is final early and
  the callable is never called - the list below has no 'EARLY', as found."""
import functools
import os

import pytest
import torch

from morgana_amd import _lib, data, graphs, models, ops, optim, synthetic
from morgana_amd import functional as F_hip

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
UPDATE = ['mg_store_pair_f32', 'mg_adam_step_plan_f32']

# name -> (precision, phone rate, hand-over, options, the step's entry points)
CASES = {
    # ------------------------------------------------------------------------------------------------ bf16, phone rate
    'bf16-phone-defer': ('bf16', True, 'defer', {}, [
        'mg_phone_front_linear_fwd_bf16', 'mg_f0_l2tail_rows_slabs_bf16', 'mg_expand_column_reduce_f32', 'mg_linear_wgrad_dgrad_bf16',
        'mg_linear_wgrad_slabs_bf16', 'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'bf16-phone-direct': ('bf16', True, 'direct', {}, [
        'mg_phone_front_linear_fwd_bf16', 'mg_f0_l2tail_rows_slabs_bf16', 'mg_expand_column_reduce_f32', 'mg_linear_wgrad_dgrad_bf16',
        'mg_slab_reduce_f32', 'mg_linear_wgrad_slabs_bf16', 'mg_slab_reduce_f32', 'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'bf16-phone-flat': ('bf16', True, 'flat', {}, [
        'mg_phone_front_linear_fwd_bf16', 'mg_f0_l2tail_rows_slabs_bf16', 'mg_expand_column_reduce_f32', 'mg_linear_wgrad_bf16',
        'mg_linear_dgrad_act_bf16', 'mg_linear_wgrad_bf16', 'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'bf16-phone-torch': ('bf16', True, 'torch', {}, [
        'mg_cast_params_bf16', 'mg_phone_front_linear_fwd_bf16', 'mg_f0_l2tail_rows_slabs_bf16', 'mg_expand_column_reduce_f32',
        'mg_linear_wgrad_bf16', 'mg_linear_dgrad_act_bf16', 'mg_linear_wgrad_bf16']),
    'bf16-phone-direct-hook': ('bf16', True, 'direct', {'hook': True}, [
        'mg_phone_front_linear_fwd_bf16', 'mg_f0_l2tail_rows_slabs_bf16', 'mg_expand_column_reduce_f32', 'mg_linear_wgrad_dgrad_bf16',
        'mg_slab_reduce_f32', 'EARLY', 'mg_linear_wgrad_slabs_bf16', 'mg_slab_reduce_f32', 'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'bf16-phone-flat-hook': ('bf16', True, 'flat', {'hook': True}, [
        'mg_phone_front_linear_fwd_bf16', 'mg_f0_l2tail_rows_slabs_bf16', 'mg_expand_column_reduce_f32', 'mg_linear_wgrad_bf16', 'EARLY',
        'mg_linear_dgrad_act_bf16', 'mg_linear_wgrad_bf16', 'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'bf16-phone-defer-graph': ('bf16', True, 'defer', {'graph': True}, [
        'mg_phone_front_linear_fwd_bf16', 'mg_f0_l2tail_rows_slabs_bf16', 'mg_linear_wgrad_dgrad_bf16', 'mg_linear_wgrad_slabs_bf16',
        'mg_adam_step_plan_f32']),
    'bf16-phone-direct-graph': ('bf16', True, 'direct', {'graph': True}, [
        'mg_phone_front_linear_fwd_bf16', 'mg_f0_l2tail_rows_slabs_bf16', 'mg_linear_wgrad_dgrad_bf16', 'mg_linear_wgrad_slabs_bf16',
        'mg_adam_step_plan_f32']),
    'bf16-phone-defer-graph-riders': ('bf16', True, 'defer', {'graph': True, 'riders': 'grid'}, [
        'mg_phone_front_linear_fwd_bf16', 'mg_f0_l2tail_rows_slabs_bf16', 'mg_linear_wgrad_dgrad_expand_bf16', 'mg_linear_wgrad_slabs_bf16',
        'mg_adam_step_plan_f32']),
    # ------------------------------------------------------------------------------------------------ bf16, frame rate
    'bf16-frame-defer': ('bf16', False, 'defer', {}, [
        'mg_upsample_index', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_bf16', 'mg_linear_bwd_fused2_slabs_bf16', 'mg_store_pair_f32',
        'mg_adam_step_plan_f32']),
    'bf16-frame-direct': ('bf16', False, 'direct', {}, [
        'mg_upsample_index', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_bf16', 'mg_linear_bwd_fused2_slabs_bf16', 'mg_slab_reduce_f32',
        'mg_slab_reduce_f32', 'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'bf16-frame-flat': ('bf16', False, 'flat', {}, [
        'mg_upsample_index', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_bf16', 'mg_linear_bwd_fused2_slabs_bf16', 'mg_slab_reduce_f32',
        'mg_slab_reduce_f32', 'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'bf16-frame-torch': ('bf16', False, 'torch', {}, [
        'mg_upsample_index', 'mg_cast_params_bf16', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_bf16', 'mg_linear_bwd_fused2_slabs_bf16',
        'mg_slab_reduce_f32', 'mg_slab_reduce_f32']),
    'bf16-frame-direct-hook': ('bf16', False, 'direct', {'hook': True}, [
        'mg_upsample_index', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_bf16', 'mg_linear_wgrad_slabs_bf16', 'mg_slab_reduce_f32', 'EARLY',
        'mg_linear_bwd_fused_bf16', 'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'bf16-frame-flat-hook': ('bf16', False, 'flat', {'hook': True}, [
        'mg_upsample_index', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_bf16', 'mg_linear_wgrad_bf16', 'EARLY', 'mg_linear_bwd_fused_bf16',
        'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'bf16-frame-defer-graph': ('bf16', False, 'defer', {'graph': True}, [
        'mg_upsample_index', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_slabs_bf16', 'mg_linear_bwd_fused2_slabs_bf16', 'mg_adam_step_plan_f32']),
    'bf16-frame-direct-graph': ('bf16', False, 'direct', {'graph': True}, [
        'mg_upsample_index', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_slabs_bf16', 'mg_linear_bwd_fused2_slabs_bf16', 'mg_adam_step_plan_f32']),
    'bf16-frame-defer-nofuse2': ('bf16', False, 'defer', {'fuse2': '0'}, [
        'mg_upsample_index', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_bf16', 'mg_linear_wgrad_slabs_bf16', 'mg_linear_bwd_fused_slabs_bf16',
        'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'bf16-frame-direct-nofuse2': ('bf16', False, 'direct', {'fuse2': '0'}, [
        'mg_upsample_index', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_bf16', 'mg_linear_wgrad_slabs_bf16', 'mg_slab_reduce_f32',
        'mg_linear_bwd_fused_bf16', 'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'bf16-frame-flat-nofuse2': ('bf16', False, 'flat', {'fuse2': '0'}, [
        'mg_upsample_index', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_bf16', 'mg_linear_wgrad_bf16', 'mg_linear_bwd_fused_bf16', 'mg_store_pair_f32',
        'mg_adam_step_plan_f32']),
    'bf16-frame-torch-nofuse2': ('bf16', False, 'torch', {'fuse2': '0'}, [
        'mg_upsample_index', 'mg_cast_params_bf16', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_bf16', 'mg_linear_wgrad_bf16',
        'mg_linear_bwd_fused_bf16']),
    'bf16-frame-defer-graph-nofuse2': ('bf16', False, 'defer', {'graph': True, 'fuse2': '0'}, [
        'mg_upsample_index', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_slabs_bf16', 'mg_linear_wgrad_slabs_bf16', 'mg_linear_bwd_fused_slabs_bf16',
        'mg_adam_step_plan_f32']),
    'bf16-frame-direct-graph-nofuse2': ('bf16', False, 'direct', {'graph': True, 'fuse2': '0'}, [
        'mg_upsample_index', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_slabs_bf16', 'mg_linear_wgrad_slabs_bf16', 'mg_linear_bwd_fused_slabs_bf16',
        'mg_adam_step_plan_f32']),
    # ------------------------------------------------------------------------------------------------ bf16x3 (phone rate)
    'x3-defer': ('bf16x3', True, 'defer', {}, [
        'mg_phone_front_linear_fwd_x3', 'mg_f0_l2tail_x3', 'mg_expand_column_reduce_f32', 'mg_linear_wgrad_dgrad_x3', 'mg_linear_wgrad_slabs_x3',
        'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'x3-direct': ('bf16x3', True, 'direct', {}, [
        'mg_phone_front_linear_fwd_x3', 'mg_f0_l2tail_x3', 'mg_expand_column_reduce_f32', 'mg_linear_wgrad_dgrad_x3', 'mg_slab_reduce_f32',
        'mg_slab_reduce_f32', 'mg_linear_wgrad_slabs_x3', 'mg_slab_reduce_f32', 'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'x3-flat': ('bf16x3', True, 'flat', {}, [
        'mg_phone_front_linear_fwd_x3', 'mg_f0_l2tail_x3', 'mg_expand_column_reduce_f32', 'mg_linear_wgrad_dgrad_x3', 'mg_linear_wgrad_slabs_x3',
        'mg_slab_reduce_f32', 'mg_slab_reduce_f32', 'mg_slab_reduce_f32', 'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'x3-torch': ('bf16x3', True, 'torch', {}, [
        'mg_split3_bf16', 'mg_split3_bf16', 'mg_split3_bf16', 'mg_phone_front_linear_fwd_x3', 'mg_f0_l2tail_x3', 'mg_expand_column_reduce_f32',
        'mg_linear_wgrad_dgrad_x3', 'mg_linear_wgrad_slabs_x3', 'mg_slab_reduce_f32', 'mg_slab_reduce_f32', 'mg_slab_reduce_f32']),
    'x3-direct-hook': ('bf16x3', True, 'direct', {'hook': True}, [
        'mg_phone_front_linear_fwd_x3', 'mg_f0_l2tail_x3', 'mg_expand_column_reduce_f32', 'mg_linear_wgrad_dgrad_x3', 'mg_slab_reduce_f32',
        'mg_slab_reduce_f32', 'EARLY', 'mg_linear_wgrad_slabs_x3', 'mg_slab_reduce_f32', 'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'x3-flat-hook': ('bf16x3', True, 'flat', {'hook': True}, [
        'mg_phone_front_linear_fwd_x3', 'mg_f0_l2tail_x3', 'mg_expand_column_reduce_f32', 'mg_linear_wgrad_dgrad_x3', 'mg_linear_wgrad_slabs_x3',
        'mg_slab_reduce_f32', 'mg_slab_reduce_f32', 'mg_slab_reduce_f32', 'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
    'x3-defer-graph': ('bf16x3', True, 'defer', {'graph': True}, [
        'mg_phone_front_linear_fwd_x3', 'mg_f0_l2tail_x3', 'mg_linear_wgrad_dgrad_x3', 'mg_linear_wgrad_slabs_x3', 'mg_adam_step_plan_f32']),
    'x3-direct-graph': ('bf16x3', True, 'direct', {'graph': True}, [
        'mg_phone_front_linear_fwd_x3', 'mg_f0_l2tail_x3', 'mg_linear_wgrad_dgrad_x3', 'mg_linear_wgrad_slabs_x3', 'mg_adam_step_plan_f32']),
    'x3-defer-graph-riders': ('bf16x3', True, 'defer', {'graph': True, 'riders': 'grid'}, [
        'mg_phone_front_linear_fwd_x3', 'mg_f0_l2tail_x3', 'mg_expand_column_reduce_f32', 'mg_linear_wgrad_dgrad_x3', 'mg_linear_wgrad_slabs_x3',
        'mg_adam_step_plan_f32']),
    # ------------------------------------------------------------------------------------------------ the deep stack
    'deep-defer': ('bf16', True, 'defer', {'deep': True}, [
        'mg_upsample_index_maps', 'mg_cast_pad_bf16', 'mg_linear_fwd_bf16', 'mg_linear_fwd_bf16', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_bf16',
        'mg_linear_wgrad_slabs_bf16', 'mg_linear_dgrad_act_bf16', 'mg_linear_wgrad_slabs_bf16', 'mg_linear_dgrad_act_bf16',
        'mg_linear_wgrad_slabs_bf16', 'mg_linear_dgrad_act_bf16', 'mg_linear_wgrad_slabs_bf16', 'mg_slab_reduce_f32', 'mg_store_pair_f32',
        'mg_adam_step_plan_f32']),
    'deep-direct': ('bf16', True, 'direct', {'deep': True}, [
        'mg_upsample_index_maps', 'mg_cast_pad_bf16', 'mg_linear_fwd_bf16', 'mg_linear_fwd_bf16', 'mg_linear_fwd_bf16', 'mg_f0_l2tail_bf16',
        'mg_linear_wgrad_slabs_bf16', 'mg_slab_reduce_f32', 'mg_linear_dgrad_act_bf16', 'mg_linear_wgrad_slabs_bf16', 'mg_slab_reduce_f32',
        'mg_linear_dgrad_act_bf16', 'mg_linear_wgrad_slabs_bf16', 'mg_slab_reduce_f32', 'mg_linear_dgrad_act_bf16',
        'mg_linear_wgrad_slabs_bf16', 'mg_slab_reduce_f32', 'mg_store_pair_f32', 'mg_adam_step_plan_f32']),
}

# hand-overs whose losses, prediction, parameters and Adam moments are equal bit for bit (see the module's docstring)
EQUAL = [
    ['bf16-phone-defer', 'bf16-phone-direct', 'bf16-phone-flat', 'bf16-phone-direct-hook', 'bf16-phone-flat-hook'],
    ['bf16-phone-defer-graph', 'bf16-phone-direct-graph', 'bf16-phone-defer-graph-riders'],
    ['bf16-frame-defer', 'bf16-frame-direct', 'bf16-frame-flat'],
    ['bf16-frame-defer-nofuse2', 'bf16-frame-direct-nofuse2', 'bf16-frame-flat-nofuse2', 'bf16-frame-direct-hook', 'bf16-frame-flat-hook'],
    ['bf16-frame-defer-graph', 'bf16-frame-direct-graph'],
    ['bf16-frame-defer-graph-nofuse2', 'bf16-frame-direct-graph-nofuse2'],
    ['x3-defer', 'x3-direct', 'x3-flat', 'x3-direct-hook', 'x3-flat-hook'],
    ['x3-defer-graph', 'x3-direct-graph', 'x3-defer-graph-riders'],
    ['deep-defer', 'deep-direct'],
]


@functools.lru_cache(maxsize=None)
def _batch(deep):
    if deep:
        return data.to_device(synthetic.make_batch(16, 400, seed=21), DEV)
    feats = data.to_device(synthetic.make_batch(32, 480, seed=6, frames_per_phone=5.0), DEV)
    assert feats['normalised_lab'].shape[:2] == (32, 96)
    data.add_bf16_table(feats)
    return data.add_bf16_table(feats, 'normalised_lab:x3')


def _model(precision, deep):
    if deep:
        torch.manual_seed(0)
        return models.F0Model(hidden_dims=(512, 512, 512, 128, 32), precision=precision).to(DEV)
    model = models.F0Model(precision=precision).to(DEV)
    own = model.state_dict()
    for key, value in synthetic.f0_model_state().items():
        own[key].copy_(torch.from_numpy(value))
    return model


@functools.lru_cache(maxsize=None)
def _run(name):
    """(entry points of the step, losses, [prediction, parameters..., moments...] on the host) of one case; run once, shared."""
    precision, phone_rate, hand, options, _ = CASES[name]
    feats, model = _batch(options.get('deep', False)), _model(precision, options.get('deep', False))
    if hand == 'torch':
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
    else:
        opt = optim.Adam(model.parameters(), lr=0.01, fused_loop=(hand == 'defer'))
    backward = F_hip.backward if hand in ('defer', 'direct') else (lambda loss: loss.backward())

    def fired(params):
        assert _lib.CALL_LOG is None or 'EARLY' not in _lib.CALL_LOG, 'the early hook fired twice in one step'
        if _lib.CALL_LOG is not None:
            _lib.CALL_LOG.append('EARLY')

    env = {'MORGANA_TAIL_RIDERS': options.get('riders', 'adam'), 'MORGANA_FUSE_WGRAD2': options.get('fuse2', '1')}
    old_env = {key: os.environ.get(key) for key in env}
    os.environ.update(env)
    old_rate, ops.PHONE_RATE = ops.PHONE_RATE, phone_rate
    old_hook = F_hip.set_early_grads_hook(fired if options.get('hook') else None)
    losses = []
    try:
        if options.get('graph'):
            _lib.CALL_LOG = []
            step = graphs.GraphedTrainStep(model, opt, feats, warmup=2)
            log = [c for c in _lib.CALL_LOG if not c.endswith('_status')]
            _lib.CALL_LOG = None
            first = CASES[name][4][0]                        # the capture: what follows the last start of a step
            calls = log[len(log) - 1 - log[::-1].index(first):]
            for _ in range(3):
                losses.append(step().item())
            out = step.output
        else:
            for i in range(3):                               # the first step builds the operand shadows
                _lib.CALL_LOG = [] if i == 2 else None
                opt.zero_grad()
                loss, out = model(feats)
                backward(loss)
                opt.step()
                calls = [c for c in _lib.CALL_LOG or [] if not c.endswith('_status')]
                _lib.CALL_LOG = None
                losses.append(loss.item())
    finally:
        _lib.CALL_LOG = None
        F_hip.set_early_grads_hook(old_hook)
        ops.PHONE_RATE = old_rate
        for key, value in old_env.items():
            if value is None:
                del os.environ[key]
            else:
                os.environ[key] = value
    state = [out[key] for key in sorted(out)] + list(model.parameters())
    if hand == 'torch':
        state += [opt.state[p][key] for p in model.parameters() for key in ('exp_avg', 'exp_avg_sq')]
    else:
        state += [opt.flat_buffers()['exp_avg'], opt.flat_buffers()['exp_avg_sq']]
    return calls, losses, [t.detach().cpu().clone() for t in state]


@pytest.mark.parametrize('name', sorted(CASES))
def test_a_step_runs_exactly_these_entry_points(name):
    """The third eager step (zero_grad to update) or the captured step of the case calls exactly the listed entry points, in order; a
    hooked case holds 'EARLY' once, where the callable fired.  If a hand-over changes its launches, this fails."""
    calls, losses, _ = _run(name)
    assert calls == CASES[name][4], calls
    assert all(loss == loss and abs(loss) < 1e3 for loss in losses), losses


@pytest.mark.parametrize('names', EQUAL, ids=lambda names: names[0])
def test_hand_overs_train_bit_for_bit_alike(names):
    """Three steps through each hand-over of the group: the losses, the last prediction, every parameter and both Adam moments are EQUAL."""
    want_losses, want_state = _run(names[0])[1:]
    for name in names[1:]:
        losses, state = _run(name)[1:]
        assert losses == want_losses, (name, losses, want_losses)
        assert len(state) == len(want_state)
        for i, (a, b) in enumerate(zip(state, want_state)):
            assert torch.equal(a, b), (name, i)
