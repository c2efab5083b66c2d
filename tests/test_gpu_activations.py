"""nn.Tanh / nn.ReLU inside fused Linear runs on the HIP path (``-m gpu``, MI355X), in the three precision modes.

Reference for every number: torch's own nn.Linear / nn.Tanh / nn.ReLU / nn.GRU and autograd ON THE CPU IN FLOAT64 with the same weights
and inputs - what the reference project executes for these modules (morgana/utils.py:401-418).  Tolerances are the project's own
(tests/test_gpu_configs.py): 1e-4 max-relative in 'fp32' and 'bf16x3' on outputs, loss and gradients; 2e-2 on outputs and 5e-2
relative L2 on gradients in 'bf16'.

The ReLU mask at rounding distance from zero.  Where the float64 pre-activation z of a ReLU layer lies within the kernel's rounding
error of 0, device and reference may take different branches of y > 0 - both correct roundings, but the gradients then differ by a
whole term, which no tolerance describes.  ``_Ref64`` therefore computes per element delta = eps * (sum_k |a_k| |w_k| + |b|) with
eps = 1.01 * 2^-8 ('bf16': two operands rounded to 8 mantissa bits), (K + 2) * 2^-24 ('fp32'), (K + 2) * 2^-24 + 2^-16 ('bf16x3': the
dropped lo * lo term); asserts that the device's mask equals the reference's wherever |z| >= delta, without exception; builds the
reference gradient with the reference's mask, adopting the device's decision on the elements with |z| < delta only; and asserts that
those are at most 10 % ('bf16') / 0.5 % (exact modes) of the valid elements - a condition on the test's inputs, not a measurement of
the kernels.  Shares of the float64 reference alone, measured on the CPU for the inputs below (fixed seeds), 'bf16' / 'fp32' /
'bf16x3' bound: the 512 -> 128 ReLU layer of the item-1 stack 5.0 % / 0.04 % / 0.06-0.07 % (4096 uniform rows, and 512 phone rows
repeated to 4096 frames); the ReLU layers of the recurrent stacks at most 5.8 % / 0.06 % / 0.08 %; the dropout stack about 3 % /
0.01 % / 0.02 % (it depends on the masks drawn).  Every run prints its shares.  Tanh is smooth and needs none of this.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from morgana_amd import _lib, graphs, losses, ops, optim, utils
from morgana_amd import functional as F_hip

from parity_report import note, rel_err

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
RTOL = 1e-4           # fp32 parity bar, tests/test_gpu_configs.py
RTOL_BF16 = 2e-2      # bf16 throughput mode, outputs and loss
GTOL_BF16 = 5e-2      # bf16 mode, relative L2 of a gradient
ORDER_TOL_BF16 = 3e-2  # phone rate against frame rate in bf16 mode (test_first_layer_of_the_609_input_models_at_phone_rate)
PRECISIONS = ('fp32', 'bf16', 'bf16x3')


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)


def _eps(precision, k):
    if precision == 'bf16':
        return 1.01 * 2.0 ** -8
    return (k + 2) * 2.0 ** -24 + (2.0 ** -16 if precision == 'bf16x3' else 0.0)


class _Ref64(object):
    """The container's modules on the CPU in float64: forward with autograd, the masked MSE, gradients per device parameter.

    ``relu_masks``: {module index: bool (B, T, N) device decisions y > 0 of that ReLU}; ``drop_masks``: {module index: float (B, T, N)
    scaled keep masks read back from the device}.  ``valid``: bool (B, T) - rows outside take no part in the mask comparison (their
    gradient is zero under the masked loss)."""

    def __init__(self, modules, precision):
        self.modules, self.precision = list(modules), precision
        self.params = {}           # device Parameter -> float64 leaf
        self.shares = []

    def leaf(self, prm):
        if prm not in self.params:
            self.params[prm] = prm.detach().double().cpu().requires_grad_(True)
        return self.params[prm]

    def forward(self, x, seq_len=None, relu_masks=None, drop_masks=None, valid=None):
        relu_masks, drop_masks = relu_masks or {}, drop_masks or {}
        last = None
        for idx, mod in enumerate(self.modules):
            if type(mod) is nn.Linear:
                w, b = self.leaf(mod.weight), self.leaf(mod.bias)
                last = (x, w, b)
                x = torch.nn.functional.linear(x, w, b)
            elif type(mod) is nn.Tanh:
                x = torch.tanh(x)
            elif type(mod) is nn.Sigmoid:
                x = torch.sigmoid(x)
            elif type(mod) is nn.ReLU:
                x = self.relu(idx, x, last, relu_masks.get(idx), valid)
            elif type(mod) is nn.Dropout:
                if mod.training and mod.p > 0:
                    x = x * drop_masks[idx].double()
            elif isinstance(mod, utils.RecurrentCuDNNWrapper):
                x = self.gru(mod.layer, x, seq_len)
            else:
                raise AssertionError('no float64 reference for %r' % (mod,))
        return x

    def relu(self, idx, z, last, dev_mask, valid):
        a, w, b = last
        with torch.no_grad():
            delta = _eps(self.precision, w.shape[1]) * (a.abs() @ w.abs().t() + b.abs())
            inside = z.abs() < delta
            ref_mask = z > 0
            rows = torch.ones(z.shape[:-1], dtype=torch.bool) if valid is None else valid
            share = float(inside[rows].double().mean())
            self.shares.append(share)
            print('ReLU at module %d (%s): %.4f %% of the valid elements within delta of 0' % (idx, self.precision, 100 * share))
            if dev_mask is None:
                mask = ref_mask
            else:
                differ = (dev_mask != ref_mask) & ~inside & rows.unsqueeze(-1)
                assert not bool(differ.any()), ('device and float64 ReLU masks differ on %d elements with |z| >= delta (module %d)'
                                                % (int(differ.sum()), idx))
                mask = torch.where(inside & rows.unsqueeze(-1), dev_mask, ref_mask)
            assert share <= (0.10 if self.precision == 'bf16' else 0.005), share
        return z * mask.double()

    def gru(self, layer, x, seq_len):
        ref = nn.GRU(layer.input_size, layer.hidden_size, batch_first=True).double()
        for name, prm in ref.named_parameters():
            prm.data.copy_(getattr(layer, name).detach().double().cpu())
            self.params[getattr(layer, name)] = prm
        packed = nn.utils.rnn.pack_padded_sequence(x, seq_len.cpu(), batch_first=True, enforce_sorted=False)
        out, _ = ref(packed)
        return nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=x.shape[1])[0]


def _mse64(pred, target, seq_len):
    """losses.mse (morgana/losses.py:29-51): per-utterance mean over the valid frames, then the mean over (batch, feature)."""
    t = pred.shape[1]
    mask = (torch.arange(t)[None, :] < seq_len.cpu()[:, None]).double().unsqueeze(-1)
    per_item = ((pred - target) ** 2 * mask).sum(1) / seq_len.cpu().double()[:, None]
    return per_item.mean()


def _valid(seq_len, t):
    return torch.arange(t)[None, :] < seq_len.cpu()[:, None]


def _device_relu_masks(modules, precision, make_input, call_kwargs, counter=None):
    """The device's decisions y > 0 of every ReLU behind a Linear: the container's prefix up to that ReLU, run as its own container on
    the same input (the same kernels on the same operands)."""
    masks = {}
    for idx, mod in enumerate(modules):
        if type(mod) is nn.ReLU:
            prefix = utils.SequentialWithRecurrent(*modules[:idx + 1], precision=precision)
            prefix.train(modules[0].training)
            if counter is not None:
                _set_counter(counter)
            with torch.no_grad():
                out, _ = prefix(make_input(), **call_kwargs)
            masks[idx] = (out > 0).cpu()
    return masks


def _set_counter(value):
    ops.dropout_draw(torch.device(DEV))
    ops._dropout_state[torch.device(DEV).index or 0].fill_(int(value))


def _compare(precision, got_out, got_loss, got_grads, ref, want_out, want_loss, valid=None, tag=''):
    """Output (valid frames), loss and every parameter gradient against the float64 run at the mode's tolerance."""
    exact = precision != 'bf16'
    go, wo = got_out.detach().double().cpu(), want_out.detach()
    if valid is not None:
        go, wo = go[valid], wo[valid]
    assert rel_err(go.numpy(), wo.numpy(), tag + 'output') < (RTOL if exact else RTOL_BF16)
    want_loss = float(want_loss.detach()) if torch.is_tensor(want_loss) else float(want_loss)
    err = abs(float(got_loss) - want_loss) / abs(want_loss)
    note(err, tag + 'loss')
    assert err < (RTOL if exact else RTOL_BF16), (tag, float(got_loss), want_loss)
    for prm, leaf in ref.params.items():
        got, want = got_grads[prm].double().cpu().numpy(), leaf.grad.numpy()
        err = rel_err(got, want, tag + 'grad') if exact else note(rel_l2(got, want), tag + 'grad (relative L2)')
        assert err < (RTOL if exact else GTOL_BF16), (tag, tuple(prm.shape), err)


# ------------------------------------------------------------------------------------------------------------ 1  stack parity
def _item1_modules():
    torch.manual_seed(1234)
    return [nn.Linear(600, 512), nn.Tanh(), nn.Linear(512, 128), nn.ReLU(), nn.Linear(128, 32), nn.Tanh(), nn.Linear(32, 3)]


def _item1_inputs(form):
    """4096 rows uniform in [0, 1) (min-max normalised labels): 'rows' = a (8, 512, 600) tensor; 'phone' / 'frame' = 8 x 64 phone rows
    repeated 8 times each by upsample_to_repetitions(fused=True), at the two orders of operations."""
    rng = np.random.RandomState(77)
    seq_len = torch.tensor([512, 480, 400, 512, 333, 512, 256, 500], dtype=torch.int64)
    target = torch.from_numpy(rng.standard_normal((8, 512, 3)).astype(np.float32))
    if form == 'rows':
        x = torch.from_numpy(rng.random_sample((8, 512, 600)).astype(np.float32))
        return x, None, target, seq_len
    lab = torch.from_numpy(rng.random_sample((8, 64, 600)).astype(np.float32))
    dur = torch.full((8, 64, 1), 8, dtype=torch.int64)
    return lab, dur, target, seq_len


def _run_item1(precision, form):
    modules = [m.to(DEV) for m in _item1_modules()]
    net = utils.SequentialWithRecurrent(*modules, precision=precision)
    x, dur, target, seq_len = _item1_inputs(form)
    x_dev = x.to(DEV)
    if form == 'rows':
        x_dev.requires_grad_(True)
        make_input = lambda: x_dev.detach()
        x64 = x.double().requires_grad_(True)
        ref_in = x64
    else:
        dur_dev = dur.to(DEV)
        make_input = lambda: utils.upsample_to_repetitions(x_dev, dur_dev, max_len=512, fused=True, phone_rate=(form == 'phone'))
        ref_in = torch.repeat_interleave(x.double(), 8, dim=1)
    sl_dev = seq_len.to(DEV)
    out, _ = net(x_dev if form == 'rows' else make_input(), seq_len=sl_dev)
    loss = losses.mse(out, target.to(DEV), sl_dev)
    loss.backward()
    grads = {p: p.grad.detach().clone() for p in net.parameters()}
    masks = _device_relu_masks(modules, precision, make_input, dict(seq_len=sl_dev))
    ref = _Ref64(modules, precision)
    want_out = ref.forward(ref_in, relu_masks=masks, valid=_valid(seq_len, 512))
    want_loss = _mse64(want_out, target.double(), seq_len)
    want_loss.backward()
    _compare(precision, out, loss.item(), grads, ref, want_out, want_loss, tag=form + ' ')
    if form == 'rows':
        got, want = x_dev.grad.double().cpu().numpy(), x64.grad.numpy()
        err = rel_err(got, want, 'input grad') if precision != 'bf16' else note(rel_l2(got, want), 'input grad (relative L2)')
        assert err < (RTOL if precision != 'bf16' else GTOL_BF16), err
    return out.detach(), loss.item(), grads, list(net.parameters())


@pytest.mark.parametrize('precision', PRECISIONS)
def test_stack_parity_on_frame_rows(precision):
    """Linear(600, 512) Tanh Linear(512, 128) ReLU Linear(128, 32) Tanh Linear(32, 3) on 4096 rows uniform in [0, 1), torch's default
    init under a fixed seed, losses.mse with a seq_len: output, loss, every parameter gradient and the input gradient against the
    float64 CPU run.  ReLU elements within delta of 0 (module docstring): 5.0 % in 'bf16', 0.04-0.07 % in the exact modes."""
    _run_item1(precision, 'rows')


@pytest.mark.parametrize('precision', PRECISIONS)
def test_stack_parity_on_an_upsampled_input_in_both_orders(precision):
    """The same stack on ``upsample_to_repetitions(lab, dur, fused=True)`` with ``phone_rate=True`` (the run works on the phone rows and
    its output is repeated) and ``phone_rate=False`` (every product on the frame rows): each against the float64 CPU run, and the two
    against each other at the tolerance the existing phone-rate tests use for that comparison (1e-4 exact modes, 3e-2 bf16)."""
    got = {form: _run_item1(precision, form) for form in ('phone', 'frame')}
    tol = RTOL if precision != 'bf16' else ORDER_TOL_BF16
    (out_p, loss_p, grads_p, prms_p), (out_f, loss_f, grads_f, prms_f) = got['phone'], got['frame']
    assert rel_err(out_p.cpu().numpy(), out_f.cpu().numpy(), 'orders: output') < tol
    assert abs(loss_p - loss_f) / abs(loss_f) < tol
    for pp, pf in zip(prms_p, prms_f):
        assert rel_err(grads_p[pp].cpu().numpy(), grads_f[pf].cpu().numpy(), 'orders: grad') < tol, tuple(pp.shape)


# ------------------------------------------------------------------------------------------------------------ 2  shipped shapes
def _gru(n_in, n_hid, precision):
    return utils.RecurrentCuDNNWrapper(nn.GRU(n_in, n_hid, batch_first=True), precision=precision)


def _shipped_modules(which, act, precision):
    """models/f0_test_model.py:28-45 and the RNN_SPSS layer layout (Linear / act / GRU / Linear / act / Linear) with the activation swapped."""
    torch.manual_seed(99)
    if which == 'gru_f0':
        return [nn.Linear(609, 256), act(), nn.Dropout(0.), _gru(256, 64, precision), nn.Dropout(0.), _gru(64, 64, precision), nn.Dropout(0.),
                _gru(64, 64, precision), nn.Dropout(0.), nn.Linear(64, 64), act(), nn.Dropout(0.), nn.Linear(64, 3)]
    return [nn.Linear(600, 512), act(), _gru(512, 512, precision), nn.Linear(512, 256), act(), nn.Linear(256, 80)]


@pytest.mark.parametrize('packed', [True, False])
@pytest.mark.parametrize('act', [nn.Tanh, nn.ReLU])
@pytest.mark.parametrize('which', ['gru_f0', 'rnn_spss'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_shipped_shape_stacks_with_the_activation_swapped(precision, which, act, packed):
    """The GRUF0Model and RNNSPSS containers with Tanh, then ReLU, in place of Sigmoid around the recurrent wrappers, on a ragged batch
    (12 utterances of 60-200 frames) with the packed-frame layout on and off: output on the valid frames, loss and every gradient
    against the float64 CPU run (nn.GRU on packed sequences, as the reference's wrapper runs it).  ReLU elements within delta of 0:
    at most 5.8 % ('bf16') / 0.08 % (exact modes)."""
    modules = [m.to(DEV) for m in _shipped_modules(which, act, precision)]
    net = utils.SequentialWithRecurrent(*modules, precision=precision)
    rng = np.random.RandomState(5)
    b, t = 12, 200
    seq_len = torch.from_numpy(np.concatenate(([t], rng.randint(60, t + 1, size=b - 1))).astype(np.int64))
    k_in, n_out = modules[0].in_features, modules[-1].out_features
    x = torch.from_numpy(rng.random_sample((b, t, k_in)).astype(np.float32))
    x = x * _valid(seq_len, t).unsqueeze(-1)                            # zero padded, as collate_fn pads
    target = torch.from_numpy(rng.standard_normal((b, t, n_out)).astype(np.float32))
    x_dev, sl_dev = x.to(DEV), seq_len.to(DEV)
    utils.set_packed_frames(packed, rows_min_padding=0.1)
    try:
        layout = utils.FrameLayout.for_batch({'n_frames': sl_dev, 'n_frames_total': int(seq_len.sum())}, t)
        assert (layout is not None) == packed
        kwargs = dict(seq_len=sl_dev, max_len=t, layout=layout)
        out, _ = net(x_dev, **kwargs)
        loss = losses.mse(out, target.to(DEV), sl_dev)
        loss.backward()
        ops.check_persistent_status()
        grads = {p: p.grad.detach().clone() for p in net.parameters()}
        masks = _device_relu_masks(modules, precision, lambda: x_dev, kwargs)
    finally:
        utils.set_packed_frames(True, rows_min_padding=0.75)
    valid = _valid(seq_len, t)
    ref = _Ref64(modules, precision)
    want_out = ref.forward(x.double(), seq_len=seq_len, relu_masks=masks, valid=valid)
    want_loss = _mse64(want_out, target.double(), seq_len)
    want_loss.backward()
    _compare(precision, out, loss.item(), grads, ref, want_out, want_loss, valid=valid)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_run_with_active_dropout_against_the_masks_read_back(precision):
    """Linear Tanh Dropout(0.2) Linear ReLU Dropout(0.2) Linear as ONE autograd node with HIP masks, against the float64 CPU run with
    the very same masks (read back through ops.dropout with the node's seed / sites / counter value, as tests/test_gpu_dropout.py
    does).  ReLU elements within delta of 0: about 3 % ('bf16') / 0.02 % (exact modes)."""
    torch.manual_seed(3)
    p = 0.2
    modules = [m.to(DEV) for m in (nn.Linear(48, 160), nn.Tanh(), nn.Dropout(p), nn.Linear(160, 96), nn.ReLU(), nn.Dropout(p), nn.Linear(96, 24))]
    net = utils.SequentialWithRecurrent(*modules, precision=precision)
    net.train()
    rng = np.random.RandomState(8)
    x = torch.from_numpy(rng.random_sample((6, 50, 48)).astype(np.float32))
    target = torch.from_numpy(rng.standard_normal((6, 50, 24)).astype(np.float32))
    seq_len = torch.tensor([50, 41, 50, 17, 33, 50], dtype=torch.int64)
    x_dev, sl_dev = x.to(DEV), seq_len.to(DEV)
    _set_counter(1000)
    calls = []
    _lib.CALL_LOG = calls
    try:
        out, _ = net(x_dev)
    finally:
        _lib.CALL_LOG = None
    assert calls.count('mg_dropout') == 2 and calls.count('mg_dropout_advance') == 1          # one node, one draw, two masks
    loss = losses.mse(out, target.to(DEV), sl_dev)
    loss.backward()
    grads = {prm: prm.grad.detach().clone() for prm in net.parameters()}
    used = torch.tensor([1000], dtype=torch.int64, device=DEV)
    seed = ops.dropout_seed()
    drop_masks = {}
    for site, (idx, width) in enumerate(((2, 160), (5, 96))):          # site0 = index of the run's first module, one site per layer
        shape = (300, ops.pad_ld(width)) if precision == 'bf16' else (300, width)
        ones = torch.ones(shape, dtype=torch.bfloat16 if precision == 'bf16' else torch.float32, device=DEV)
        drop_masks[idx] = ops.dropout(ones, p, seed, site, used).float()[:, :width].reshape(6, 50, width).cpu()
    masks = _device_relu_masks(modules, precision, lambda: x_dev, {}, counter=1000)
    ref = _Ref64(modules, precision)
    want_out = ref.forward(x.double(), relu_masks=masks, drop_masks=drop_masks)
    want_loss = _mse64(want_out, target.double(), seq_len)
    want_loss.backward()
    _compare(precision, out, loss.item(), grads, ref, want_out, want_loss)


# ------------------------------------------------------------------------------------------------------------ 3  no torch kernel
@pytest.mark.parametrize('precision', PRECISIONS)
def test_no_torch_kernel_runs_for_the_activations(precision, monkeypatch):
    """nn.Tanh.forward and nn.ReLU.forward replaced by functions that raise: the stacks of the tests above and a stand-alone nn.Tanh
    behind a recurrent wrapper run forward and backward without touching them."""
    def refuse(self, input):
        raise AssertionError('torch ran %s.forward' % type(self).__name__)
    monkeypatch.setattr(nn.Tanh, 'forward', refuse)
    monkeypatch.setattr(nn.ReLU, 'forward', refuse)
    rng = np.random.RandomState(2)
    x, dur, target, seq_len = _item1_inputs('phone')
    stacks = [(_item1_modules(), torch.from_numpy(rng.random_sample((8, 512, 600)).astype(np.float32)), seq_len, None)]
    for order in (True, False):
        stacks.append((_item1_modules(), (x, dur, order), seq_len, None))
    sl = torch.tensor([200] + [150] * 11, dtype=torch.int64)
    for which in ('gru_f0', 'rnn_spss'):
        for act in (nn.Tanh, nn.ReLU):
            mods = _shipped_modules(which, act, precision)
            stacks.append((mods, torch.from_numpy(rng.random_sample((12, 200, mods[0].in_features)).astype(np.float32)), sl, 200))
    torch.manual_seed(4)
    stacks.append(([nn.Linear(40, 64), nn.ReLU(inplace=True), _gru(64, 64, precision), nn.Tanh(), nn.Linear(64, 8)],
                   torch.from_numpy(rng.random_sample((12, 200, 40)).astype(np.float32)), sl, 200))
    for mods, inp, lens, max_len in stacks:
        net = utils.SequentialWithRecurrent(*mods, precision=precision).to(DEV)
        if isinstance(inp, tuple):
            inp = utils.upsample_to_repetitions(inp[0].to(DEV), inp[1].to(DEV), max_len=512, fused=True, phone_rate=inp[2])
        else:
            inp = inp.to(DEV)
        out, _ = net(inp, seq_len=lens.to(DEV), max_len=max_len)
        loss = losses.mse(out, torch.zeros_like(out), lens.to(DEV))
        loss.backward()
        ops.check_persistent_status()
        assert bool(torch.isfinite(loss)) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    with pytest.raises(AssertionError):
        nn.Tanh()(torch.zeros(1))                                       # the patch is live


def test_stand_alone_activations_match_float64():
    """[Linear, ReLU, GRU, Tanh, Linear]: the stand-alone nn.Tanh behind the recurrent wrapper runs mg_act_f32 / mg_act_grad_f32; output,
    loss and gradients against the float64 CPU run in fp32 mode."""
    torch.manual_seed(4)
    modules = [m.to(DEV) for m in (nn.Linear(40, 64), nn.ReLU(), _gru(64, 64, 'fp32'), nn.Tanh(), nn.Linear(64, 8))]
    net = utils.SequentialWithRecurrent(*modules, precision='fp32')
    rng = np.random.RandomState(6)
    seq_len = torch.tensor([90, 70, 90, 31], dtype=torch.int64)
    x = torch.from_numpy(rng.random_sample((4, 90, 40)).astype(np.float32)) * _valid(seq_len, 90).unsqueeze(-1)
    target = torch.from_numpy(rng.standard_normal((4, 90, 8)).astype(np.float32))
    x_dev, sl_dev = x.to(DEV), seq_len.to(DEV)
    calls = []
    _lib.CALL_LOG = calls
    try:
        out, _ = net(x_dev, seq_len=sl_dev, max_len=90)
        loss = losses.mse(out, target.to(DEV), sl_dev)
        loss.backward()
    finally:
        _lib.CALL_LOG = None
    # forward: the Tanh; backward: the Tanh, and the ReLU as the trailing activation of the one-layer run [Linear, ReLU]
    assert calls.count('mg_act_f32') == 1 and calls.count('mg_act_grad_f32') == 2
    grads = {p: p.grad.detach().clone() for p in net.parameters()}
    masks = _device_relu_masks(modules, 'fp32', lambda: x_dev, dict(seq_len=sl_dev, max_len=90))
    valid = _valid(seq_len, 90)
    ref = _Ref64(modules, 'fp32')
    want_out = ref.forward(x.double(), seq_len=seq_len, relu_masks=masks, valid=valid)
    want_loss = _mse64(want_out, target.double(), seq_len)
    want_loss.backward()
    _compare('fp32', out, loss.item(), grads, ref, want_out, want_loss, valid=valid)


# ------------------------------------------------------------------------------------------------------------ 4  Sigmoid unchanged
def _p(t):
    return ops._p(t)


@pytest.mark.parametrize('m,n,k', [(300, 96, 24), (4096, 128, 512), (1000, 32, 160)])
def test_sigmoid_dgrad_entry_points_are_the_act_forms(m, n, k):
    """mg_linear_dgrad_f32 / _bf16 give results torch.equal to mg_linear_dgrad_act_* with MG_ACT_SIGMOID on the same operands (narrow,
    128 x 128 and wide-tile shapes), and MG_ACT_NONE through the new entry points equals H = NULL through the old ones."""
    lib = _lib.load()
    torch.manual_seed(m + n)
    dy, w = torch.randn(m, n, device=DEV), torch.randn(n, k, device=DEV) * 0.1
    h = torch.sigmoid(torch.randn(m, k, device=DEV))
    st = ops._stream()

    def f32(old, h_, act):
        dx = torch.full((m, k), float('nan'), device=DEV)
        if old:
            _lib.check(lib.mg_linear_dgrad_f32(_p(dy), m, n, _p(w), k, _p(h_), _p(dx), st), 'mg_linear_dgrad_f32')
        else:
            _lib.check(lib.mg_linear_dgrad_act_f32(_p(dy), m, n, _p(w), k, _p(h_), act, _p(dx), st), 'mg_linear_dgrad_act_f32')
        return dx
    assert torch.equal(f32(True, h, None), f32(False, h, ops.ACT_SIGMOID))
    assert torch.equal(f32(True, None, None), f32(False, None, ops.ACT_NONE))
    assert torch.equal(f32(True, None, None), f32(False, h, ops.ACT_NONE))
    want = (dy.double() @ w.double()) * h.double() * (1 - h.double())
    assert rel_err(f32(False, h, ops.ACT_SIGMOID).double().cpu().numpy(), want.cpu().numpy()) < RTOL

    dy_b, wt_b, h_b = ops.cast_pad_bf16(dy), ops.cast_pad_bf16(w.t().contiguous()), ops.cast_pad_bf16(h)
    lddx = ops.pad8(k)

    def bf16(old, h_, act, out_f32):
        dx = torch.zeros((m, lddx), dtype=torch.float32 if out_f32 else torch.bfloat16, device=DEV)
        ldh = h_.shape[1] if h_ is not None else 0
        if old:
            _lib.check(lib.mg_linear_dgrad_bf16(_p(dy_b), dy_b.shape[1], m, n, _p(wt_b), wt_b.shape[1], k, _p(h_), ldh, _p(dx), lddx,
                                                1 if out_f32 else 0, st), 'mg_linear_dgrad_bf16')
        else:
            _lib.check(lib.mg_linear_dgrad_act_bf16(_p(dy_b), dy_b.shape[1], m, n, _p(wt_b), wt_b.shape[1], k, _p(h_), ldh, act, _p(dx),
                                                    lddx, 1 if out_f32 else 0, st), 'mg_linear_dgrad_act_bf16')
        return dx
    for out_f32 in (False, True):
        assert torch.equal(bf16(True, h_b, None, out_f32), bf16(False, h_b, ops.ACT_SIGMOID, out_f32))
        assert torch.equal(bf16(True, None, None, out_f32), bf16(False, None, ops.ACT_NONE, out_f32))
        assert torch.equal(bf16(True, None, None, out_f32), bf16(False, h_b, ops.ACT_NONE, out_f32))
    assert rel_err(bf16(False, h_b, ops.ACT_SIGMOID, True)[:, :k].double().cpu().numpy(), want.cpu().numpy()) < RTOL_BF16
    # the two new derivatives through the same kernels
    for act, fn in ((ops.ACT_TANH, lambda y: 1 - y * y), (ops.ACT_RELU, lambda y: (y > 0).double())):
        y = (torch.tanh(torch.randn(m, k, device=DEV)) if act == ops.ACT_TANH else torch.relu(torch.randn(m, k, device=DEV)))
        want = (dy.double() @ w.double()) * fn(y.double())
        assert rel_err(f32(False, y, act).double().cpu().numpy(), want.cpu().numpy()) < RTOL
        y_b = ops.cast_pad_bf16(y)
        want_b = (dy.double() @ w.double()) * fn(y_b[:, :k].double())
        assert rel_err(bf16(False, y_b, act, True)[:, :k].double().cpu().numpy(), want_b.cpu().numpy()) < RTOL_BF16


# ------------------------------------------------------------------------------------------------------------ 5  elementwise kernels
@pytest.mark.parametrize('n', [1, 255, 1025, 4099, 1 << 20 | 3])
def test_elementwise_kernels_against_float64(n):
    """mg_act_f32 / mg_act_grad_f32 for sizes that are no multiples of the block size.  Tanh over [-20, 20] with 0, +-tiny and +-large
    (saturation, no NaN): 1e-6 relative (tanhf: a few ulp).  ReLU bit for bit as torch.relu on the CPU has it: relu(-0.0) = -0.0, NaN
    stays NaN; its gradient as torch's threshold_backward: 0 where y <= 0, the incoming gradient where y is NaN."""
    rng = np.random.RandomState(n % 1000)
    special = np.array([0.0, -0.0, 1e-30, -1e-30, 1e-38, -1e-38, 20.0, -20.0, 88.8, -88.8, 1e4, -1e4, 3e38, -3e38, np.inf, -np.inf], dtype=np.float32)
    x = np.linspace(-20, 20, n).astype(np.float32)
    x[:min(n, special.size)] = special[:min(n, special.size)]
    if n > special.size + 8:
        x[special.size:special.size + 8] = rng.standard_normal(8).astype(np.float32) * 1e-4
    dy = rng.standard_normal(n).astype(np.float32)
    x_dev, dy_dev = torch.from_numpy(x).to(DEV), torch.from_numpy(dy).to(DEV)
    # tanh
    y = ops.act(x_dev, ops.ACT_TANH)
    want = torch.tanh(torch.from_numpy(x).double())
    assert not bool(torch.isnan(y).any())
    np.testing.assert_allclose(y.double().cpu().numpy(), want.numpy(), rtol=1e-6, atol=0)
    g = ops.act_grad(dy_dev, y, ops.ACT_TANH)
    want_g = torch.from_numpy(dy).double() * (1 - y.double().cpu() ** 2)
    np.testing.assert_allclose(g.double().cpu().numpy(), want_g.numpy(), rtol=1e-6, atol=2e-7 * float(np.abs(dy).max()))
    # sigmoid through the same entry points equals the dedicated ones bit for bit
    assert torch.equal(ops.act(x_dev, ops.ACT_SIGMOID), ops.sigmoid(x_dev))
    s = ops.sigmoid(x_dev)
    assert torch.equal(ops.act_grad(dy_dev, s, ops.ACT_SIGMOID), ops.sigmoid_grad(dy_dev, s))
    # relu, with NaNs among the inputs
    xr = x.copy()
    xr[::7] = np.nan if n > 1 else xr[::7]
    xr_t = torch.from_numpy(xr).requires_grad_(True)
    want_r = torch.relu(xr_t)
    want_r.backward(torch.from_numpy(dy))
    y = ops.act(torch.from_numpy(xr).to(DEV), ops.ACT_RELU).cpu()
    assert torch.equal(torch.isnan(y), torch.isnan(want_r.detach()))
    ok = ~torch.isnan(y)
    assert torch.equal(y[ok], want_r.detach()[ok]) and torch.equal(torch.signbit(y[ok]), torch.signbit(want_r.detach()[ok]))
    g = ops.act_grad(dy_dev, y.to(DEV), ops.ACT_RELU).cpu()
    assert torch.equal(g, xr_t.grad)


# ------------------------------------------------------------------------------------------------------------ 6  graph capture
class _StackModel(nn.Module):
    def __init__(self, precision):
        super(_StackModel, self).__init__()
        self.layers = utils.SequentialWithRecurrent(*_item1_modules(), precision=precision)

    def forward(self, features):
        out, _ = self.layers(features['x'], seq_len=features['n_frames'])
        return losses.mse(out, features['y'], features['n_frames']), out


@pytest.mark.parametrize('precision', PRECISIONS)
def test_graph_replay_equals_eager(precision):
    """graphs.GraphedTrainStep on the item-1 model: replays against eager steps on the same batch - losses, parameters and both Adam
    moments EQUAL bit for bit, as the existing graph tests assert for the Sigmoid models."""
    x, _, target, seq_len = _item1_inputs('rows')
    feats = {'x': x.to(DEV), 'y': target.to(DEV), 'n_frames': seq_len.to(DEV)}

    def fresh():
        model = _StackModel(precision).to(DEV)
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
