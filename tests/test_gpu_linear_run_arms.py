"""Which path ``SequentialWithRecurrent`` takes for a Linear run, pinned by the entry points it calls (``-m gpu``, MI355X).

``SequentialWithRecurrent._forward_linear_run`` chooses among eight arms by the type of its input.  Two are pinned where they are
measured (tests/test_gpu_configs.py::test_first_layer_of_the_609_input_models_at_phone_rate: the concat at phone rate by
``mg_phone_concat_layer_bf16``, the plain concat by ``mg_gather_concat_bf16``).  This module pins the other six, in the idiom of that
test - the case must take the path it names: each arm's distinguishing entry points are counted under ``_lib.CALL_LOG`` over one
forward and one ``functional.backward``, next to the neighbouring arm that must not call them.  The numbers these paths compute are
held elsewhere (tests/test_gpu_activations.py, tests/test_gpu_vae.py, tests/test_gpu_parity.py); the shapes are theirs.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from morgana_amd import _lib, data, losses, ops, synthetic, utils
from morgana_amd import functional as F_hip

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PRECISIONS = ('fp32', 'bf16', 'bf16x3')


def _gru(n_in, n_hid, precision):
    return utils.RecurrentCuDNNWrapper(nn.GRU(n_in, n_hid, batch_first=True), precision=precision)


def _calls(net, make_input, target, seq_len, **kwargs):
    """Entry points of one forward + backward of ``losses.mse(net(input), target, seq_len)``; the loss and gradients must be finite."""
    log = []
    _lib.CALL_LOG = log
    try:
        out, _ = net(make_input(), seq_len=seq_len, **kwargs)
        loss = losses.mse(out, target, seq_len)
        F_hip.backward(loss)
    finally:
        _lib.CALL_LOG = None
    ops.check_persistent_status()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in net.parameters())
    return log


def _phone_rows():
    """8 x 64 phone rows of 600 labels, each repeated 8 times: 512 + 1024 extra table rows against 4096 frames."""
    rng = np.random.RandomState(77)
    lab = torch.from_numpy(rng.random_sample((8, 64, 600)).astype(np.float32)).to(DEV)
    dur = torch.full((8, 64, 1), 8, dtype=torch.int64, device=DEV)
    seq_len = torch.tensor([512, 480, 400, 512, 333, 512, 256, 500], dtype=torch.int64, device=DEV)
    target = torch.from_numpy(rng.standard_normal((8, 512, 3)).astype(np.float32)).to(DEV)
    return lab, dur, target, seq_len


@pytest.mark.parametrize('precision', PRECISIONS)
def test_upsampled_input_runs_on_phone_rows_or_frame_rows_as_asked(precision):
    """An ``UpsampledSequence`` into a run that ends the stack: at phone rate the run works on the table and its OUTPUT is repeated
    (one ``mg_gather_rows_f32``, its backward one ``mg_segment_sum``); at frame rate the first layer's loader applies the frame map
    (neither call, and no materialised input).  In front of a GRU wrapper the table goes to the wrapper, which repeats the rows of its
    own input projection and sums the gate gradients per phone."""
    lab, dur, target, seq_len = _phone_rows()
    torch.manual_seed(1234)
    net = utils.SequentialWithRecurrent(nn.Linear(600, 512), nn.Tanh(), nn.Linear(512, 128), nn.ReLU(), nn.Linear(128, 3), precision=precision).to(DEV)
    for phone_rate in (True, False):
        calls = _calls(net, lambda: utils.upsample_to_repetitions(lab, dur, max_len=512, fused=True, phone_rate=phone_rate), target, seq_len)
        assert calls.count('mg_gather_rows_f32') == (1 if phone_rate else 0), (phone_rate, calls)
        assert calls.count('mg_segment_sum') == (1 if phone_rate else 0), (phone_rate, calls)
        assert calls.count('mg_upsample_index_maps') == (1 if phone_rate else 0) and calls.count('mg_upsample_index') == (0 if phone_rate else 1)
        assert 'mg_gather_rows_bf16' not in calls and 'mg_scatter_rows_f32' not in calls
    torch.manual_seed(7)
    net = utils.SequentialWithRecurrent(nn.Linear(600, 256), nn.Tanh(), _gru(256, 64, precision), nn.Linear(64, 3), precision=precision).to(DEV)
    calls = _calls(net, lambda: utils.upsample_to_repetitions(lab, dur, max_len=512, fused=True, phone_rate=True), target, seq_len, max_len=512)
    first_gru = min(i for i, c in enumerate(calls) if c.startswith('mg_gru_fwd'))
    assert calls.count('mg_gather_rows_f32') == 1 and calls.index('mg_gather_rows_f32') == first_gru - 1, calls      # the projected rows
    assert calls.count('mg_segment_sum') == 1 and calls.index('mg_segment_sum') > calls.index('mg_masked_mse_f32'), calls
    calls = _calls(net, lambda: utils.upsample_to_repetitions(lab, dur, max_len=512, fused=True, phone_rate=False), target, seq_len, max_len=512)
    assert 'mg_gather_rows_f32' not in calls and 'mg_segment_sum' not in calls, calls


@pytest.mark.parametrize('precision', PRECISIONS)
def test_run_behind_a_recurrence_packs_the_frames_when_the_layout_says_so(precision):
    """12 utterances of 60-200 frames behind a GRU wrapper: with a worthwhile ``FrameLayout`` the run gathers the valid rows, its
    result is unpacked (backward: the padding rows' column sums, ``mg_pad_rows_colsum_f32``) and its input gradient is scattered back
    (``mg_scatter_rows_f32``); without one it runs on the padded rows and calls neither.  In 'bf16' mode the padded rows' first layer
    reads the bf16 copy the recurrence wrote (no cast between the recurrence and the run) - and casts when that copy is switched off."""
    torch.manual_seed(99)
    net = utils.SequentialWithRecurrent(nn.Linear(600, 512), nn.Tanh(), _gru(512, 512, precision), nn.Linear(512, 256), nn.Tanh(), nn.Linear(256, 80),
                                        precision=precision).to(DEV)
    rng = np.random.RandomState(5)
    b, t = 12, 200
    seq_len = torch.from_numpy(np.concatenate(([t], rng.randint(60, t + 1, size=b - 1))).astype(np.int64))
    valid = (torch.arange(t)[None, :] < seq_len[:, None]).float()
    x = (torch.from_numpy(rng.random_sample((b, t, 600)).astype(np.float32)) * valid.unsqueeze(-1)).to(DEV)
    target = torch.from_numpy(rng.standard_normal((b, t, 80)).astype(np.float32)).to(DEV)
    sl = seq_len.to(DEV)

    def casts_behind_the_recurrence(calls):
        first = min(i for i, c in enumerate(calls) if c.startswith('mg_gru_fwd'))
        return calls[first:calls.index('mg_masked_mse_f32')].count('mg_cast_pad_bf16')

    for packed in (True, False):
        utils.set_packed_frames(packed, rows_min_padding=0.1)
        try:
            layout = utils.FrameLayout.for_batch({'n_frames': sl, 'n_frames_total': int(seq_len.sum())}, t)
            assert (layout is not None) == packed
            calls = _calls(net, lambda: x, target, sl, max_len=t, layout=layout)
        finally:
            utils.set_packed_frames(True, rows_min_padding=0.75)
        assert calls.count('mg_pad_rows_colsum_f32') == (1 if packed else 0), (packed, calls)
        assert calls.count('mg_scatter_rows_f32') == (1 if packed else 0), (packed, calls)
        assert calls.count('mg_gather_rows_bf16') == (1 if packed and precision == 'bf16' else 0), (packed, calls)
        if precision == 'bf16' and not packed:
            assert utils.OUT_SHADOW and 'mg_gru_fwd_persist_out_bf16' in calls and casts_behind_the_recurrence(calls) == 0, calls
    if precision == 'bf16':
        old, utils.OUT_SHADOW = utils.OUT_SHADOW, False
        try:
            calls = _calls(net, lambda: x, target, sl, max_len=t, layout=None)
        finally:
            utils.OUT_SHADOW = old
        assert casts_behind_the_recurrence(calls) == 1, calls


@pytest.mark.parametrize('precision', PRECISIONS)
def test_concat_with_a_latent_takes_the_latent_entry(precision):
    """cat(upsampled labels, counters, z of the item) -> Linear: one gather pass writes the operand with z in it
    (``mg_gather_concat_latent_*``) and z's gradient is the per-item row sums of the first layer's gradient (``mg_rows_sum_per_item``);
    the same input without z takes the plain concat."""
    feats = synthetic.make_acoustic_batch(4, (40, 90), streams=(('lf0', 3, 'mse'),), seed=31)
    t = feats['normalised_counters'].shape[1]
    d = data.to_device(feats, DEV)
    rng = np.random.RandomState(3)
    z = torch.from_numpy(rng.randn(4, 16).astype(np.float32)).to(DEV).requires_grad_(True)
    target = torch.from_numpy(rng.randn(4, t, 3).astype(np.float32)).to(DEV)
    gather = 'mg_gather_concat_latent_bf16' if precision == 'bf16' else 'mg_gather_concat_latent_f32'
    plain = 'mg_gather_concat_bf16' if precision == 'bf16' else 'mg_gather_concat_f32'
    for latent in (z, None):
        torch.manual_seed(2)
        net = utils.SequentialWithRecurrent(nn.Linear(609 + (16 if latent is not None else 0), 256), nn.Sigmoid(), _gru(256, 64, precision), nn.Linear(64, 3),
                                            precision=precision).to(DEV)

        def make():
            up = utils.upsample_to_repetitions(d['normalised_lab'], d['dur'], max_len=t, fused=True)
            return utils.concat_frame_features(up, d['normalised_counters'], latent)
        calls = _calls(net, make, target, d['n_frames'], max_len=t)
        assert calls.count(gather) == (1 if latent is not None else 0), calls
        assert calls.count('mg_rows_sum_per_item') == (1 if latent is not None else 0), calls
        assert calls.count(plain) == (0 if latent is not None else 1), calls
    assert z.grad is not None and torch.isfinite(z.grad).all() and float(z.grad.abs().max()) > 0
