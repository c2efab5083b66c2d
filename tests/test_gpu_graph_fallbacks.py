"""The fallback paths of graphs.GraphedStepCache (run with ``-m gpu`` on an MI355X): a training step that is not replayed from a graph -
a capture the step refuses, a graph budget used up, a resident group that falls back to single steps, a capture that fails half way
through - must train, and report its losses, exactly as the eager loop does.  Every case trains the same model twice from the same
state, once with ``use_graphs=False`` (the reference) and once through the path under test: epoch losses, the 'loss' metric and every
parameter EQUAL (the eager steps of a fallback run the same kernels; replays are held bit-equal to eager in test_gpu_parity.py), and
the cache's counters show that the path under test was the one taken."""
import warnings

import pytest
import torch

from morgana_amd import _lib, data, experiment_builder, graphs, models, ops, optim, synthetic
from morgana_amd import functional as F_hip

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _load_state(model, state):
    own = model.state_dict()
    for key, value in state.items():
        own[key].copy_(torch.from_numpy(value))
    return model


class ReadsBack(models.F0Model):
    """An F0Model whose step reads a device value back to the host (HIP refuses that inside a stream capture).  ``read_first``: the
    read comes before anything else of the forward pass; else it comes after the whole stack and its loss - by then a capture has
    recorded (not run) the re-cast of every stale bf16 operand copy.  ``read_batch``: only batches of this many utterances read (None:
    every batch).  ``fail_with``: an exception type raised instead, and only while the stream is capturing."""
    read_first = False
    read_batch = None
    fail_with = None

    def _read(self, features):
        if self.fail_with is not None:
            if torch.cuda.is_current_stream_capturing():
                raise self.fail_with('refused by the step (test)')
            return
        if self.read_batch is None or features['n_frames'].shape[0] == self.read_batch:
            self.frames_seen = getattr(self, 'frames_seen', 0) + int(features['n_frames'].sum().item())

    def forward(self, features):
        if self.read_first:
            self._read(features)
        loss, outputs = super().forward(features)
        if not self.read_first:
            self._read(features)
        return loss, outputs


def _model_class(**attrs):
    return type('ReadsBackVariant', (ReadsBack,), attrs)


def _perturb_in_place(model, seed):
    """Every parameter changed in place (``load_state_dict`` of a perturbed copy: torch's version counters move, no optimiser step)."""
    gen = torch.Generator().manual_seed(seed)
    state = model.state_dict()
    for name, p in model.named_parameters():
        state[name] = p.detach() + 0.01 * torch.randn(p.shape, generator=gen).to(p.device)
    model.load_state_dict(state)


def _train(model_class, batches, use_graphs, group=1, epochs=3, precision='bf16', setup=None, before_epoch=None):
    torch.manual_seed(3)
    builder = experiment_builder.ExperimentBuilder(model_class, dict(precision=precision), learning_rate=0.01, device=DEV,
                                                   use_graphs=use_graphs, graph_group=group)
    _load_state(builder.model, synthetic.f0_model_state())
    dev_batches = [data.to_device(b, DEV, bf16_tables=builder.model.bf16_table_features()) for b in batches]
    optimizer = builder.make_optimizer()
    if use_graphs and setup is not None:
        setup(builder._cache_for(optimizer))
    history, metric = [], []
    for epoch in range(epochs):
        if before_epoch is not None:
            before_epoch(epoch, builder.model)
        history.append(builder.train_epoch(dev_batches, optimizer))
        metric.append(float(builder.model.metrics['train']['loss'].result()))
    params = {k: v.detach().clone() for k, v in builder.model.named_parameters()}
    return history, metric, params, builder


def _assert_same_training(ref, got):
    hist_e, metric_e, params_e, _ = ref
    hist_g, metric_g, params_g, _ = got
    assert hist_g == hist_e
    assert metric_g == metric_e
    for name in params_e:
        assert torch.equal(params_g[name], params_e[name]), name


def _check_current_copies(model):
    """Every bf16 operand copy (ops.param_shadows) and pair-plane copy (ops.pair_shadows) whose stamp says current equals a fresh
    cast / split of its weight.  Returns how many were checked."""
    checked = 0
    for p in model.parameters():
        stamp = (p._version, getattr(p, '_mg_updates', 0))
        w = p.detach()
        sh = getattr(p, '_mg_shadow', None)
        if sh is not None and sh['version'] == stamp:
            assert torch.equal(sh['plain'][:, :p.shape[1]], w.to(torch.bfloat16))
            if sh['t'] is not None:
                assert torch.equal(sh['t'][:, :p.shape[0]], w.t().to(torch.bfloat16))
            checked += 1
        pr = getattr(p, '_mg_pair', None)
        if pr is not None and pr['version'] == stamp:
            for got, transpose in ((pr['plain'], False), (pr['t'], True)):
                if got is None:
                    continue
                want = ops.split_pair(w, transpose=transpose)
                cols = p.shape[0] if transpose else p.shape[1]
                ldp = ops.pad_ld(cols)
                assert torch.equal(got[:, :cols], want[:, :cols])                       # hi plane
                assert torch.equal(got[:, ldp:ldp + cols], want[:, ldp:ldp + cols])     # lo plane
            checked += 1
    return checked


def test_group_fallback_with_a_refused_capture_files_every_loss():
    """Resident groups of three over seven batches (the last group short) and a model that reads the device on every forward, with
    ``max_group_graphs = 0``: every group of a warmed-up epoch takes the single-step fallback, whose first step's capture is refused
    (``step``'s failed-capture exit) and whose later steps stay on ordinary launches.  Each of those steps must file its loss into the
    epoch's loss log; before, their entries stayed 0 and the epoch mean came out low."""
    batches = [synthetic.make_batch(16, 120, seed=900 + i) for i in range(7)]
    cls = _model_class(read_first=True)

    def setup(cache):
        cache.max_group_graphs = 0

    ref = _train(cls, batches, False, group=3)
    with pytest.warns(UserWarning, match='cannot be captured'):
        got = _train(cls, batches, True, group=3, setup=setup)
    _assert_same_training(ref, got)
    stats = got[3]._graph_cache.stats()
    assert stats['eager'] == 21 and stats['replayed'] == 0 and stats['graphs'] == 0 and stats['group_graphs'] == 0, stats


def test_group_fallback_with_the_graph_budget_used_files_every_loss():
    """Resident groups of three over 21 batches of distinct frame counts (21 signatures), one group graph and a single-step budget of
    four graphs (``max_graphs = 2``): the first group is captured and replayed, the next four batches capture single-step graphs
    in the second epoch and replay them (their losses ride in the next load), the other fourteen find the budget used and run as
    ordinary launches (``step``'s last exit) - both ways of filing a loss meet in one epoch's loss log."""
    batches = [synthetic.make_batch(8, 60 + 3 * i, seed=950 + i) for i in range(21)]

    def setup(cache):
        cache.max_group_graphs, cache.max_graphs = 1, 2

    ref = _train(models.F0Model, batches, False, group=3)
    got = _train(models.F0Model, batches, True, group=3, setup=setup)
    _assert_same_training(ref, got)
    stats = got[3]._graph_cache.stats()
    assert stats['group_graphs'] == 1 and stats['group_replays'] == 2 and stats['graphs'] == 4, stats
    assert stats['eager'] == 21 + 14 + 14 and stats['replayed'] == 2 * 3 + 4 + 4, stats


@pytest.mark.parametrize('group', [1, 3])
@pytest.mark.parametrize('precision,b,t', [('bf16', 16, 120), ('bf16x3', 96, 500)])
def test_a_capture_that_fails_after_recording_casts_leaves_no_stale_copy(group, precision, b, t):
    """Every weight is changed in place right before the epoch whose steps are first captured, and the capture fails only AFTER the
    forward pass has recorded the re-cast of each bf16 operand copy (the device read sits behind the loss).  Recording a cast runs
    nothing: a copy stamped current by it still holds the old weight.  ``group`` 1: the single-step capture fails; 3: a resident
    group whose middle batch reads the device, so the capture has recorded the first batch's whole step (forward, backward, the
    update with its re-casts) before it fails.  The eager steps behind the failure must see the changed weights: losses and
    parameters EQUAL to the eager loop, and every copy that claims to be current equals a fresh cast of its weight."""
    batches = [synthetic.make_batch(b - 4 * (i == 1), t - 20 * (i == 2), seed=1000 + i) for i in range(3)]      # three signatures
    cls = _model_class(read_batch=(b - 4) if group > 1 else None)

    def before_epoch(epoch, model):
        if epoch == 1:                                  # the epoch whose steps are captured (the first one sees every signature once)
            _perturb_in_place(model, seed=11)

    ref = _train(cls, batches, False, group=group, precision=precision, before_epoch=before_epoch)
    with pytest.warns(UserWarning, match='cannot be captured'):
        got = _train(cls, batches, True, group=group, precision=precision, before_epoch=before_epoch)
    _assert_same_training(ref, got)
    assert got[3].model.frames_seen == ref[3].model.frames_seen
    stats = got[3]._graph_cache.stats()
    assert stats['eager'] == 9 and stats['replayed'] == 0 and stats['graphs'] == 0 and stats['group_graphs'] == 0, stats
    assert _check_current_copies(got[3].model) > 0


@pytest.mark.parametrize('group', [1, 3])
@pytest.mark.parametrize('error', [ValueError, _lib.MorganaHipError, torch.cuda.OutOfMemoryError])
def test_errors_inside_a_capture_are_raised_not_swallowed(group, error):
    """A kernel argument the library refuses (ValueError: MG_EINVAL), a launch error that is no stream-capture status
    (``_lib.MorganaHipError``) or an allocation that fails while the step is being captured is a fault of the step, not a step that
    cannot be captured: ``train_epoch`` raises it instead of warning and falling back to ordinary launches.  The thread stays usable:
    an ordinary model captures and replays afterwards."""
    batches = [synthetic.make_batch(16, 120, seed=1100 + i) for i in range(4)]
    builder = experiment_builder.ExperimentBuilder(_model_class(fail_with=error), dict(precision='bf16'), learning_rate=0.01, device=DEV,
                                                   use_graphs=True, graph_group=group)
    dev_batches = [data.to_device(x, DEV, bf16_tables=builder.model.bf16_table_features()) for x in batches]
    optimizer = builder.make_optimizer()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        with pytest.raises(error, match='refused by the step'):
            for _ in range(2):                          # the first capture comes in the first epoch (group 1) or the second
                builder.train_epoch(dev_batches, optimizer)
    assert not [w for w in caught if 'cannot be captured' in str(w.message)]
    assert builder._graph_cache.stats()['replayed'] == 0
    plain = experiment_builder.ExperimentBuilder(models.F0Model, dict(precision='bf16'), learning_rate=0.01, device=DEV, use_graphs=True,
                                                 graph_group=1)
    dev_batches = [data.to_device(x, DEV, bf16_tables=plain.model.bf16_table_features()) for x in batches]
    plain.train_epoch(dev_batches, plain.make_optimizer())
    assert plain._graph_cache.stats()['replayed'] == 3


def test_step_files_the_loss_on_every_exit():
    """``GraphedStepCache.step(features, loss_slot=)`` driven through each of its exits - first sight (eager), capture and replay,
    second capture of the pair, replay of a loaded batch, a refused capture, a signature left on ordinary launches, the graph budget
    used - with the loss slots of ten consecutive steps: after ``flush`` every slot holds its step's loss, EQUAL to the eager loop's,
    and so are the parameters."""
    a = [data.to_device(synthetic.make_batch(16, 120, seed=1200 + i), DEV) for i in range(5)]
    bb = [data.to_device(synthetic.make_batch(12, 120, seed=1210 + i), DEV) for i in range(3)]      # reads the device back
    c = [data.to_device(synthetic.make_batch(16, 150, seed=1220 + i), DEV) for i in range(2)]
    seq = [a[0], bb[0], bb[1], a[1], a[2], c[0], c[1], a[3], bb[2], a[4]]
    # first sight, first sight, refused capture, capture, capture (pair), first sight, budget used, replay, no-capture signature, replay
    cls = _model_class(read_batch=12)

    def fresh():
        torch.manual_seed(3)
        model = _load_state(cls(precision='bf16').to(DEV), synthetic.f0_model_state())
        return model, optim.Adam(model.parameters(), lr=0.01, fused_loop=True)

    model_e, opt_e = fresh()
    want = []
    for f in seq:
        opt_e.zero_grad()
        loss, _ = model_e(f)
        F_hip.backward(loss)
        opt_e.step()
        want.append(loss.detach().clone())
    model_g, opt_g = fresh()
    cache = graphs.GraphedStepCache(model_g, opt_g, max_graphs=1)
    slots = torch.zeros(len(seq), dtype=torch.float32, device=DEV)
    with pytest.warns(UserWarning, match='cannot be captured'):
        for i, f in enumerate(seq):
            cache.step(f, clone_loss=False, loss_slot=slots[i])
    cache.flush()
    assert slots.tolist() == torch.stack(want).tolist()
    for (name, p_e), p_g in zip(model_e.named_parameters(), model_g.parameters()):
        assert torch.equal(p_g, p_e), name
    stats = cache.stats()
    assert stats['eager'] == 6 and stats['replayed'] == 4 and stats['graphs'] == 2, stats
