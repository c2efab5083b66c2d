"""The BASELINE model definitions, written against the plugin surface exactly as a user of the reference would.

* ``F0Model``  - README stack Linear/Sigmoid 600-512-128-32-1 (README.rst:53-97; configs C1-C3).
* ``RNNSPSS``  - Linear-512 / sigmoid / GRU-512 / Linear-256 / sigmoid / Linear-out, the layer layout of
                 models/RNN_SPSS.py:32-42 with the GRU cell of models/f0_test_model.py:32-39 (configs C4-C5).
* ``GRUF0Model`` - the reference's shipped F0 model, models/f0_test_model.py:21-107: 609-dim input, Linear-256 / sigmoid /
                 GRU-64 x 3 / Linear-64 / sigmoid / Linear-3 (lf0 + deltas).
* ``LSTMAcousticModel`` - the reference's shipped acoustic model, models/RNN_SPSS.py:20-139: 609-dim input (labels +
                 counters), Linear-512 / sigmoid / 8 x LSTM-512 / Linear-256 / sigmoid / Linear-199, four output streams.
* ``VAEF0Model`` - a ``BaseVAE`` (base_models.py:288-381) built from ``GRUF0Model``: a GRU-64 encoder over the lf0 deltas gives an
                 utterance-level latent that is appended to every frame of the decoder's input.
``SequentialWithRecurrent`` returns ``(output, hiddens)`` (utils.py:418), so all of them unpack it.
"""
import os

import torch
import torch.nn as nn

from . import data
from . import losses
from . import metrics
from . import ops
from . import utils
from . import viz
from . import functional as F_hip
from .base_models import BaseSPSS, BaseVAE


def _has_delta_params(normalisers, name):
    norm = normalisers.get(name)
    return norm is not None and getattr(norm, 'delta_params_torch', None) is not None


class F0Model(BaseSPSS):
    def __init__(self, input_dim=600, hidden_dims=(512, 128, 32), output_dim=1, target_name='lf0', precision=None,
                 fused_upsample=True, fused_loss=True, phone_rate=None):
        super(F0Model, self).__init__()
        self.fused_loss = fused_loss
        self.phone_rate = phone_rate          # order of operations of THIS model (base_models.BaseModel.phone_rate)
        dims = (input_dim,) + tuple(hidden_dims) + (output_dim,)
        mods = []
        for i in range(len(dims) - 1):
            mods.append(nn.Linear(dims[i], dims[i + 1]))
            if i < len(dims) - 2:
                mods.append(nn.Sigmoid())
        self.layers = utils.SequentialWithRecurrent(*mods, precision=precision)
        self.target_name = target_name
        self.fused_upsample = fused_upsample

    def normaliser_sources(self):
        return {
            'lab': data.MinMaxNormaliser('lab'),
            self.target_name: data.MeanVarianceNormaliser(self.target_name),
        }

    def predict(self, features):
        target = features.get('normalised_' + self.target_name)
        max_len = target.shape[1] if target is not None else None
        norm_lab_at_frame_rate = utils.upsample_to_repetitions(features['normalised_lab'], features['dur'],
                                                               max_len=max_len, fused=self.fused_upsample, phone_rate=self.phone_rate)
        pred_norm, _ = self.layers(norm_lab_at_frame_rate, seq_len=features['n_frames'])
        outputs = {'pred_norm_' + self.target_name: pred_norm}
        if self.target_name in self.normalisers:
            outputs['pred_' + self.target_name] = self.normalisers[self.target_name].denormalise(pred_norm.detach())
        return outputs

    def loss(self, features, output_features):
        return losses.mse(output_features['pred_norm_' + self.target_name],
                          features['normalised_' + self.target_name], features['n_frames'])

    def bf16_table_features(self):
        from . import functional as F_hip
        precision = self.layers.precision or F_hip.get_precision()
        # 'bf16': the table's bf16 copy; 'bf16x3': its [hi | lo] pair planes (data.add_bf16_table) - made once per batch by the loader
        return ('normalised_lab',) if precision == 'bf16' else ('normalised_lab:x3',) if precision == 'bf16x3' else ()

    def step_input_keys(self, features):
        # With the loader's operand table of this precision in the batch the FUSED steps read the table, never the fp32 feature - but
        # only they do: any other path of the stack (a batch too small for the fused 'bf16x3' step, a stack that is not the README's)
        # casts or splits the fp32 feature inside the step.  Decided by the very predicates the forward pass uses.
        from . import ops
        precision = self.layers.precision or utils.F_hip.get_precision()
        suffix = {'bf16': data.BF16_TABLE_SUFFIX, 'bf16x3': data.X3_TABLE_SUFFIX}.get(precision)
        lab, target = features.get('normalised_lab'), features.get('normalised_' + self.target_name)
        table = features.get('normalised_lab' + suffix) if suffix is not None else None
        if table is None or lab is None or target is None or not self.fused_loss or not self.fused_upsample:
            return None
        rows, k = lab.shape[0] * lab.shape[1] + ops.PHONE_RATE_EXTRA, lab.shape[2]
        if precision == 'bf16':
            reads_table = self.layers._fused_mse_spec(target, precision) is not None and tuple(table.shape) == (rows, ops.pad_ld(k))
        else:
            reads_table = False
            if ops.phone_rate_choice(self.phone_rate) and tuple(table.shape) == (rows, 2 * ops.pad_ld(k)):
                x = utils.upsample_to_repetitions(lab, features['dur'], max_len=target.shape[1], fused=True, table_bf16=table, phone_rate=True)
                reads_table = (isinstance(x, utils.UpsampledSequence) and
                               self.layers._fused_x3_params(x, target, features['n_frames'], precision) is not None)
        if not reads_table:
            return None
        return [k_ for k_, v in features.items() if isinstance(v, torch.Tensor) and k_ not in ('normalised_lab', 'lab')]

    def forward(self, features):
        """``predict`` + ``loss`` (base_models.py:279-285) with the stack's tail and the loss fused when a target is at hand
        (``SequentialWithRecurrent.forward_mse``); identical outputs otherwise."""
        target = features.get('normalised_' + self.target_name)
        if target is None or not self.fused_loss:
            return super(F0Model, self).forward(features)
        # the loader's operand table of the phone rows, if the batch carries the one this precision reads (bf16_table_features)
        x3 = (self.layers.precision or utils.F_hip.get_precision()) == 'bf16x3'
        table = features.get('normalised_lab' + (data.X3_TABLE_SUFFIX if x3 else data.BF16_TABLE_SUFFIX))
        x = utils.upsample_to_repetitions(features['normalised_lab'], features['dur'], max_len=target.shape[1],
                                          fused=self.fused_upsample, table_bf16=table, phone_rate=self.phone_rate)
        loss, pred_norm = self.layers.forward_mse(x, target, seq_len=features['n_frames'])
        outputs = {'pred_norm_' + self.target_name: pred_norm}
        if self.target_name in self.normalisers:
            outputs['pred_' + self.target_name] = self.normalisers[self.target_name].denormalise(pred_norm.detach())
        return loss, outputs


class RNNSPSS(BaseSPSS):
    def __init__(self, input_dim=600, hidden_dim=512, post_dim=256, output_dim=80, target_name='mcep', precision=None,
                 fused_upsample=True, phone_rate=None):
        super(RNNSPSS, self).__init__()
        self.phone_rate = phone_rate
        self.layers = utils.SequentialWithRecurrent(
            nn.Linear(input_dim, hidden_dim),
            nn.Sigmoid(),
            utils.RecurrentCuDNNWrapper(nn.GRU(hidden_dim, hidden_dim, batch_first=True), precision=precision),
            nn.Linear(hidden_dim, post_dim),
            nn.Sigmoid(),
            nn.Linear(post_dim, output_dim),
            precision=precision)
        self.target_name = target_name
        self.fused_upsample = fused_upsample

    def normaliser_sources(self):
        return {
            'lab': data.MinMaxNormaliser('lab'),
            self.target_name: data.MeanVarianceNormaliser(self.target_name),
        }

    def predict(self, features):
        target = features.get('normalised_' + self.target_name)
        max_len = target.shape[1] if target is not None else None
        norm_lab_at_frame_rate = utils.upsample_to_repetitions(features['normalised_lab'], features['dur'],
                                                               max_len=max_len, fused=self.fused_upsample, phone_rate=self.phone_rate)
        # max_len: the padded frame axis is the longest utterance (collate_fn, data.py:183-193), so the GRU wrapper need not read
        # seq_len back to crop its output (utils.py:383) - no host sync in the step, which makes it capturable as a HIP graph
        layout = utils.FrameLayout.for_batch(features, max_len) if max_len is not None else None
        pred_norm, _ = self.layers(norm_lab_at_frame_rate, seq_len=features['n_frames'], max_len=max_len, layout=layout)
        outputs = {'pred_norm_' + self.target_name: pred_norm}
        if self.target_name in self.normalisers:
            outputs['pred_' + self.target_name] = self.normalisers[self.target_name].denormalise(pred_norm.detach())
        return outputs

    def loss(self, features, output_features):
        return losses.mse(output_features['pred_norm_' + self.target_name],
                          features['normalised_' + self.target_name], features['n_frames'])


# ---------------------------------------------------------------------------------------------------------------------------------
# The reference's two shipped models (models/RNN_SPSS.py, models/f0_test_model.py) are instances of ONE scheme: labels + counters
# -> a layer stack -> a prediction that is split into output STREAMS, each with a masked loss, optionally a delta-feature
# trajectory (MLPG) and a streaming metric.  A stream is a row of a table; the generic model below reads the table.
# ---------------------------------------------------------------------------------------------------------------------------------
class Stream(object):
    """One output stream.  ``name``: feature name ('lf0'); ``dim``: columns of the prediction; ``loss``: 'mse' against
    ``normalised_<name>_deltas`` (a delta stream: static + delta + delta-delta, denormalised and turned into a trajectory by MLPG)
    or 'sigmoid_bce' against ``<name>`` (a probability stream) or 'ce' against ``<name>`` as integer class indices, (B, T) or
    (B, T, 1) (a categorical stream of ``dim`` classes, losses.ce: the logits go out as ``<name>_logits``, the predicted class as
    ``<name>``, (B, T) int64) or any callable ``(predictions, targets, seq_len)`` - typically a ``losses.sequence_loss``-wrapped
    function - which makes a delta stream exactly as 'mse' does (target, output key, normaliser, trajectory, metrics) and is called
    where ``losses.mse`` would be.  ``metric`` = (registered name, factory, kind): kind 'trajectory'
    feeds (target, trajectory, n_frames), 'voiced_trajectory' adds a voicing mask (the predicted probability stream ``voicing`` >
    0.5, or the feature of that name when the model predicts none), 'accuracy' feeds the hit rate of a probability or categorical
    stream.  ``trajectory_weight`` > 0 (delta streams only) adds a loss on what is listened to, the MLPG trajectory (trajectory /
    minimum-generation-error training): the stream's loss becomes ``delta loss + trajectory_weight * trajectory_loss(normalised
    trajectory, normalised_<name>, n_frames)`` with the gradient flowing through MLPG (``viz.synthesis.mlpg_trajectory``);
    ``trajectory_loss`` is a callable ``(predictions, targets, seq_len)``, default ``losses.mse``.
    ``loss='mdn'`` (with ``n_components`` = K and an optional floor ``min_log_std`` under the log standard deviations) makes a
    mixture-density delta stream: it owns ``width`` = K (1 + 2 dim) prediction columns (``losses.mdn``'s layout), is scored by
    ``losses.mdn`` against ``normalised_<name>_deltas`` and is a delta stream for target, normaliser, trajectory and metrics.  Its raw
    parameters go out as ``<name>_mdn``, the most probable component's mean as ``normalised_<name>_deltas`` and its per-frame
    variance as ``normalised_<name>_deltas_variance`` (``losses.mdn_select``, both detached); MLPG then runs on the denormalised mean
    under the PER-FRAME variances ``variance * std_dev^2``.  Such a stream takes no trajectory loss.  In ``eval()`` mode after
    ``StreamModel.sample_mixtures(temperature, noise_scale)`` the component is DRAWN per frame instead (``losses.mdn_sample``: the
    same two keys, plus the component as ``<name>_component``); ``select_mixtures()`` restores the default.
    ``gv_weight`` > 0 (delta streams only) adds a global-variance term on the same differentiable trajectory, against over-smoothing:
    ``gv_weight * losses.gv(normalised trajectory, normalised_<name>, n_frames, log=gv_log)``; with ``trajectory_weight`` as well the
    trajectory is solved and normalised once.
    ``loss='gaussian'`` (with an optional floor ``min_log_std``) makes a delta stream that predicts its own variance (the single
    Gaussian per frame of Hashimoto et al. 2016): it owns ``width`` = 2 dim columns, ``[means | log standard deviations s]``, is
    scored by ``losses.gaussian`` against ``normalised_<name>_deltas`` and is a delta stream for target, normaliser, trajectory and
    metrics.  Its raw slice goes out as ``<name>_gaussian`` (what the loss reads), the means slice as ``normalised_<name>_deltas``
    and ``exp(2 max(s, min_log_std))`` as ``normalised_<name>_deltas_variance``; MLPG runs on the denormalised means under the
    per-frame variances ``variance * std_dev^2``, as for an 'mdn' stream.  Unlike that one it TAKES ``trajectory_weight`` and
    ``gv_weight``: the mean and the variance are differentiable functions of the weights, and the trajectory then comes from
    ``viz.synthesis.mlpg_trajectory(..., variance_grad=True)``, whose backward trains both (csrc/mlpg.hip, mg_mlpg_grad_mv_f32);
    without a weight the two outputs are detached."""

    def __init__(self, name, dim, loss='mse', metric=None, voicing='vuv', trajectory_weight=0., trajectory_loss=None, n_components=1,
                 min_log_std=None, gv_weight=0., gv_log=True):
        self.name, self.dim, self.loss, self.metric, self.voicing = name, dim, loss, metric, voicing
        self.trajectory_weight, self.trajectory_loss = float(trajectory_weight), trajectory_loss
        self.gv_weight, self.gv_log = float(gv_weight), bool(gv_log)
        self.n_components, self.min_log_std = int(n_components), None if min_log_std is None else float(min_log_std)
        if self.is_mdn and self.n_components < 1:
            raise ValueError('stream %r: an \'mdn\' stream needs n_components >= 1, got %r' % (name, n_components))
        if self.is_gaussian and self.n_components != 1:
            raise ValueError('stream %r: n_components belongs to an \'mdn\' stream: a \'gaussian\' stream is one Gaussian per frame, got '
                             'n_components=%r' % (name, n_components))
        if not self.is_mdn and not self.is_gaussian and (self.n_components != 1 or min_log_std is not None):
            raise ValueError('stream %r: n_components and min_log_std belong to an \'mdn\' stream: a %r stream has no mixture'
                             % (name, loss))
        if self.is_mdn and (self.trajectory_weight > 0. or trajectory_loss is not None):
            raise ValueError('stream %r: a trajectory loss needs a delta stream with a differentiable prediction (loss \'mse\' or a '
                             'callable): the selected mean of an \'mdn\' stream is not a differentiable function of the weights'
                             % (name,))
        if self.trajectory_weight < 0.:
            raise ValueError('stream %r: trajectory_weight must not be negative, got %r' % (name, trajectory_weight))
        if (self.trajectory_weight > 0. or trajectory_loss is not None) and not self.is_delta:
            raise ValueError('stream %r: a trajectory loss needs a delta stream (loss \'mse\' or a callable): a %r stream has no '
                             'MLPG trajectory' % (name, loss))
        if trajectory_loss is not None and not callable(trajectory_loss):
            raise TypeError('stream %r: trajectory_loss must be a callable (predictions, targets, seq_len), got %r' % (name, trajectory_loss))
        if self.gv_weight < 0. or self.gv_weight != self.gv_weight:
            raise ValueError('stream %r: gv_weight must not be negative, got %r' % (name, gv_weight))
        if self.gv_weight > 0. and self.is_mdn:
            raise ValueError('stream %r: a global-variance loss needs a delta stream with a differentiable prediction (loss \'mse\' or a '
                             'callable): the selected mean of an \'mdn\' stream is not a differentiable function of the weights'
                             % (name,))
        if self.gv_weight > 0. and not self.is_delta:
            raise ValueError('stream %r: a global-variance loss needs a delta stream (loss \'mse\' or a callable): a %r stream has no '
                             'MLPG trajectory' % (name, loss))

    @property
    def is_delta(self):
        return self.loss == 'mse' or self.loss == 'mdn' or self.loss == 'gaussian' or callable(self.loss)

    @property
    def is_mdn(self):
        return self.loss == 'mdn'

    @property
    def is_gaussian(self):
        return self.loss == 'gaussian'

    @property
    def width(self):
        """Columns of the prediction the stream owns: ``dim``, K (1 + 2 dim) for a mixture-density stream, 2 dim for a 'gaussian' one."""
        if self.is_gaussian:
            return 2 * self.dim
        return losses.mdn_width(self.n_components, self.dim) if self.is_mdn else self.dim

    @property
    def is_categorical(self):
        return self.loss == 'ce'

    @property
    def output_key(self):
        if self.is_categorical:
            return self.name + '_logits'
        return 'normalised_%s_deltas' % self.name if self.is_delta else self.name

    @property
    def trains_trajectory(self):
        return self.trajectory_weight > 0.

    @property
    def trains_gv(self):
        return self.gv_weight > 0.

    @property
    def differentiable_trajectory(self):
        """The stream's trajectory feeds a loss term: it comes from the differentiable MLPG solve."""
        return self.trains_trajectory or self.trains_gv


# The delta streams' MLPG launches on streams of their own (StreamModel._with_trajectories); 0 = one after the other on the current stream
TRAJECTORY_STREAMS = os.environ.get('MORGANA_TRAJECTORY_STREAMS', '1') != '0'
_traj_streams = {}


def _trajectory_streams(device, n):
    pool = _traj_streams.setdefault(device.index, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device))
    return pool[:n]


class StreamModel(BaseSPSS):
    """``layers`` (a ``SequentialWithRecurrent`` whose last Linear is as wide as the streams together) + a stream table ->
    ``predict`` / ``loss`` / ``forward`` as the shipped models define them: input = upsampled labels concatenated with the frame
    counters, per-stream outputs under the reference's keys, loss = mean of the streams' masked losses, trajectories and metrics on
    the device whenever the normalisers carry delta parameters (i.e. under ``ExperimentBuilder``; ``generate=False`` turns both off).
    ``fused_loss``: the split, the sigmoid and all masked losses as one pass over the prediction (``losses.multi_stream``); refused
    for a table with a callable loss or a trajectory loss, which that kernel cannot run.
    A stream with ``trajectory_weight`` > 0 or ``gv_weight`` > 0 gets its trajectory from the differentiable MLPG (one forward solve,
    on the current stream) and a trajectory and / or global-variance term in ``loss``; metrics read the detached trajectory.
    ``speaker_id_list`` (a file of speaker names): the delta streams are normalised PER SPEAKER
    (``data.SpeakerDependentMeanVarianceNormaliser``); trajectories are then denormalised with ``features['speaker_index']`` and MLPG
    runs under each utterance's own delta variances (``ops.mlpg``'s per-item mode).  None changes nothing."""

    def __init__(self, layers, streams, fused_upsample=True, fused_loss=False, generate=True, speaker_id_list=None):
        super(StreamModel, self).__init__()
        self.layers = layers
        self.streams = tuple(streams)
        custom = [st.name for st in self.streams if callable(st.loss)]
        if fused_loss and custom:
            raise ValueError('StreamModel: fused_loss=True cannot score the stream(s) %s with a callable loss: the one-pass multi-stream '
                             'kernel runs no user code (use fused_loss=False)' % ', '.join(custom))
        weighted = [st.name for st in self.streams if st.trains_trajectory]
        if fused_loss and weighted:
            raise ValueError('StreamModel: fused_loss=True cannot score the stream(s) %s with a trajectory loss: the one-pass multi-stream '
                             'kernel has no trajectory term (use fused_loss=False)' % ', '.join(weighted))
        varied = [st.name for st in self.streams if st.trains_gv]
        if fused_loss and varied:
            raise ValueError('StreamModel: fused_loss=True cannot score the stream(s) %s with a global-variance loss: the one-pass '
                             'multi-stream kernel has no global-variance term (use fused_loss=False)' % ', '.join(varied))
        mixtures = [st.name for st in self.streams if st.is_mdn]
        if fused_loss and mixtures:
            raise ValueError('StreamModel: fused_loss=True cannot score the stream(s) %s with a mixture-density loss: the one-pass '
                             'multi-stream kernel has no MDN term (use fused_loss=False)' % ', '.join(mixtures))
        gaussians = [st.name for st in self.streams if st.is_gaussian]
        if fused_loss and gaussians:
            raise ValueError('StreamModel: fused_loss=True cannot score the stream(s) %s with a Gaussian likelihood: the one-pass '
                             'multi-stream kernel has no such term (use fused_loss=False)' % ', '.join(gaussians))
        self.speaker_id_list = speaker_id_list
        self.fused_upsample, self.fused_loss, self.generate = fused_upsample, fused_loss, generate
        registered = {st.metric[0]: st.metric[1]() for st in self.streams if st.metric is not None}
        if registered:
            self.metrics.add_metrics('all', **registered)

    def normaliser_sources(self):
        sources = {'dur': data.MeanVarianceNormaliser('dur'), 'lab': data.MinMaxNormaliser('lab'),
                   'counters': data.MinMaxNormaliser('counters')}
        for st in self.streams:
            if st.is_delta and self.speaker_id_list is not None:
                sources[st.name] = data.SpeakerDependentMeanVarianceNormaliser(st.name, self.speaker_id_list, use_deltas=True)
            elif st.is_delta:
                sources[st.name] = data.MeanVarianceNormaliser(st.name, use_deltas=True)
            if st.is_delta and self._gv_generation is not None:      # the prior's statistics (data.fit_global_variance writes them)
                sources[st.name + data.GV_SUFFIX] = (
                    data.SpeakerDependentMeanVarianceNormaliser(st.name + data.GV_SUFFIX, self.speaker_id_list)
                    if self.speaker_id_list is not None else data.MeanVarianceNormaliser(st.name + data.GV_SUFFIX))
        return sources

    # -- generation under a global-variance prior ------------------------------------------------------------------------------------
    _gv_generation = None         # (gv_weight, max_iter) while generate_with_gv is in force

    def generate_with_gv(self, gv_weight=1., max_iter=48):
        """In ``eval()`` mode every delta stream's trajectory from now on is generated under the global-variance prior of its
        ``{name}_gv`` normaliser (``ops.mlpg_gv``: mean and std_dev of the per-utterance variance of the static feature, fitted by
        ``data.fit_global_variance``; per speaker with ``speaker_id_list``) instead of being the plain MLPG solution, and
        ``normaliser_sources()`` lists those normalisers.  In ``train()`` mode nothing changes, and neither do the differentiable
        trajectories of a trajectory or global-variance LOSS.  Returns the model."""
        if not any(st.is_delta for st in self.streams):
            raise ValueError('generate_with_gv: the model has no delta stream to generate a trajectory for (streams: %s)'
                             % ', '.join(st.name for st in self.streams))
        gv_weight, max_iter = float(gv_weight), int(max_iter)
        if not 0. <= gv_weight < float('inf'):
            raise ValueError('generate_with_gv: gv_weight must be finite and >= 0, got %r' % gv_weight)
        if max_iter < 3:
            raise ValueError('generate_with_gv: max_iter must be at least 3, got %r' % max_iter)
        self._gv_generation = (gv_weight, max_iter)
        return self

    def generate_without_gv(self):
        """Back to the plain MLPG solution, the default.  Returns the model."""
        self._gv_generation = None
        return self

    def _gv_trajectory(self, name, pred_deltas, variances, seq_len, index=None):
        """``ops.mlpg_gv`` under the ``{name}_gv`` normaliser: row ``index[b]`` of its tables for utterance b when it is per speaker."""
        gv_weight, max_iter = self._gv_generation
        prior = self.normalisers.get(name + data.GV_SUFFIX) if hasattr(self.normalisers, 'get') else None
        if prior is None or not prior.params:
            raise KeyError('generate_with_gv: the normalisers hold no parameters for %r (fit them with data.fit_global_variance and load '
                           'them through normaliser_sources())' % (name + data.GV_SUFFIX))
        if isinstance(prior, data._SpeakerDependentNormaliser):
            if index is None:
                raise KeyError("the normaliser of %r is speaker-dependent: the batch needs features['%s'] (the loaders write it)"
                               % (name + data.GV_SUFFIX, data.SPEAKER_INDEX_KEY))
            mean, std_dev = (ops.item_rows(table, index) for table in prior.tables(pred_deltas.device))
        else:
            mean, std_dev = (prior.params_torch[key].to(device=pred_deltas.device, dtype=torch.float32) for key in ('mean', 'std_dev'))
        if seq_len is not None:
            seq_len = seq_len.reshape(-1).to(device=pred_deltas.device, dtype=torch.int64)
        return ops.mlpg_gv(pred_deltas, variances, mean, std_dev ** 2, viz.synthesis.DEFAULT_WINDOWS, padding_size=100, seq_len=seq_len,
                           gv_weight=gv_weight, max_iter=max_iter)

    # -- generation from mixture-density streams -------------------------------------------------------------------------------------
    _mixture_sampling = None      # (temperature, noise_scale) while sample_mixtures is in force

    def sample_mixtures(self, temperature=1., noise_scale=0.):
        """In ``eval()`` mode every 'mdn' stream from now on DRAWS its component per frame (``losses.mdn_sample`` with these two
        arguments) instead of taking the most probable one: each ``predict`` is another rendition.  The drawn mean and variance go out
        under the keys of the selected ones (MLPG, denormalisation and metrics read them unchanged), the component as
        ``<name>_component``.  In ``train()`` mode nothing changes: the most probable component, as before.  Returns the model."""
        if not any(st.is_mdn for st in self.streams):
            raise ValueError("sample_mixtures: the model has no 'mdn' stream to draw from (streams: %s)"
                             % ', '.join('%s: %s' % (st.name, st.loss if not callable(st.loss) else 'callable') for st in self.streams))
        self._mixture_sampling = ops.mdn_sample_arguments('sample_mixtures', temperature, noise_scale)
        return self

    def select_mixtures(self):
        """Back to the most probable component of every frame (``losses.mdn_select``), the default.  Returns the model."""
        self._mixture_sampling = None
        return self

    # -- pieces ----------------------------------------------------------------------------------------------------------------------
    def _run_layers(self, features):
        norm_counters = features['normalised_counters']
        norm_lab_at_frame_rate = utils.upsample_to_repetitions(features['normalised_lab'], features['dur'],
                                                               max_len=norm_counters.shape[1], fused=self.fused_upsample,
                                                               phone_rate=self.phone_rate)
        model_inputs = utils.concat_frame_features(norm_lab_at_frame_rate, norm_counters)
        prediction, _ = self.layers(model_inputs, seq_len=features['n_frames'], max_len=norm_counters.shape[1])
        return prediction

    def _split(self, prediction, probabilities=None, classes=None, seq_len=None):
        """Per-stream outputs under the reference's keys; ``probabilities``: the sigmoid of the probability streams when a fused
        loss pass has computed it already; ``classes``: {stream name: predicted class} of the categorical streams likewise;
        ``seq_len``: the valid frames a mixture-density stream's selection reads (None: all of them)."""
        parts = torch.split(prediction, [st.width for st in self.streams], dim=-1) if len(self.streams) > 1 else (prediction,)
        outputs = {}
        for st, part in zip(self.streams, parts):
            if st.is_mdn:
                outputs[st.name + '_mdn'] = part          # what the loss reads (the column slice, in place)
                if self._mixture_sampling is not None and not self.training:
                    temperature, noise_scale = self._mixture_sampling
                    outputs[st.name + '_component'], outputs[st.output_key], outputs[st.output_key + '_variance'] = losses.mdn_sample(
                        part, st.n_components, st.dim, seq_len=seq_len, min_log_std=st.min_log_std, temperature=temperature,
                        noise_scale=noise_scale)
                else:
                    _, outputs[st.output_key], outputs[st.output_key + '_variance'] = losses.mdn_select(
                        part, st.n_components, st.dim, seq_len=seq_len, min_log_std=st.min_log_std)
            elif st.is_gaussian:
                outputs[st.name + '_gaussian'] = part     # what the loss reads (the column slice, in place)
                mean, log_std = part[..., :st.dim], part[..., st.dim:]
                if st.min_log_std is not None:
                    log_std = torch.clamp(log_std, min=st.min_log_std)
                variance = torch.exp(2. * log_std)
                if not st.differentiable_trajectory:      # nothing downstream trains them: MLPG and the metrics read values
                    mean, variance = mean.detach(), variance.detach()
                outputs[st.output_key], outputs[st.output_key + '_variance'] = mean, variance
            elif st.is_delta:
                outputs[st.output_key] = part
            elif st.is_categorical:
                outputs[st.output_key] = part
                outputs[st.name] = torch.argmax(part.detach(), dim=-1) if classes is None else classes[st.name]
            else:
                outputs[st.output_key] = torch.sigmoid(part) if probabilities is None else probabilities
        return outputs

    def _generating(self):
        return self.generate and all(_has_delta_params(self.normalisers, st.name) for st in self.streams if st.is_delta)

    def _trajectory(self, name, pred_norm_deltas, seq_len=None, speaker_index=None, differentiable=False, norm_variance=None,
                    variance_grad=False):
        """Denormalised deltas -> most probable static trajectory under the global delta variances, padding 100
        (models/RNN_SPSS.py:107-118, models/f0_test_model.py:83-89), without leaving the device.  With a speaker-dependent
        normaliser: each utterance under the delta variances of its own speaker (row ``speaker_index[b]`` of the tables).
        ``differentiable``: the same solve with the gradient flowing back to ``pred_norm_deltas`` (a stream with a trajectory loss).
        ``norm_variance`` (B, T, D): per-frame variances in the normalised space (a mixture-density stream's selected component);
        MLPG then runs under ``norm_variance * std_dev^2`` per frame instead of the global ``std_dev^2``.
        ``variance_grad`` (a 'gaussian' stream, with ``differentiable`` and ``norm_variance``): the gradient flows back to
        ``norm_variance`` as well (``viz.synthesis.mlpg_trajectory(..., variance_grad=True)``)."""
        normaliser = self.normalisers[name]
        if norm_variance is not None and differentiable and not variance_grad:
            raise ValueError('stream %r: per-frame variances have no differentiable trajectory' % (name,))
        if not differentiable:
            pred_norm_deltas = pred_norm_deltas.detach()
        if isinstance(normaliser, data._SpeakerDependentNormaliser):
            if speaker_index is None:
                raise KeyError("the normaliser of %r is speaker-dependent: the batch needs features['%s'] (the loaders write it)"
                               % (name, data.SPEAKER_INDEX_KEY))
            pred_deltas = normaliser.denormalise(pred_norm_deltas, speaker_index, deltas=True)
            index = normaliser.speaker_index(speaker_index, pred_deltas.device)
            std_dev = ops.item_rows(normaliser.tables(pred_deltas.device, deltas=True)[1], index)
            if self._gv_generation is not None and not self.training:
                variances = std_dev ** 2 if norm_variance is None else norm_variance.detach() * (std_dev ** 2)[:, None, :]
                return self._gv_trajectory(name, pred_deltas.detach(), variances, seq_len, index)
            if differentiable and variance_grad:
                return viz.synthesis.mlpg_trajectory(pred_deltas, norm_variance * (std_dev ** 2)[:, None, :], padding_size=100,
                                                     seq_len=seq_len, variance_grad=True)
            if differentiable:
                return viz.synthesis.mlpg_trajectory(pred_deltas, std_dev ** 2, padding_size=100, seq_len=seq_len)
            variances = std_dev ** 2 if norm_variance is None else norm_variance.detach() * (std_dev ** 2)[:, None, :]
            return ops.mlpg(pred_deltas, variances, viz.synthesis.DEFAULT_WINDOWS, padding_size=100, seq_len=seq_len)
        pred_deltas = normaliser.denormalise(pred_norm_deltas, deltas=True)
        if self._gv_generation is not None and not self.training:
            std_dev = normaliser.delta_params_torch['std_dev'].to(device=pred_deltas.device, dtype=torch.float32)
            variances = std_dev ** 2 if norm_variance is None else norm_variance.detach() * std_dev ** 2
            return self._gv_trajectory(name, pred_deltas.detach(), variances, seq_len)
        if differentiable and variance_grad:
            std_dev = normaliser.delta_params_torch['std_dev'].to(device=pred_deltas.device, dtype=torch.float32)
            return viz.synthesis.mlpg_trajectory(pred_deltas, norm_variance * std_dev ** 2, padding_size=100, seq_len=seq_len,
                                                 variance_grad=True)
        if norm_variance is not None:
            std_dev = normaliser.delta_params_torch['std_dev'].to(device=pred_deltas.device, dtype=torch.float32)
            return ops.mlpg(pred_deltas, norm_variance.detach() * std_dev ** 2, viz.synthesis.DEFAULT_WINDOWS, padding_size=100,
                            seq_len=seq_len)
        if differentiable:
            std_dev = normaliser.delta_params_torch['std_dev'].to(device=pred_deltas.device, dtype=torch.float32)
            return viz.synthesis.mlpg_trajectory(pred_deltas, std_dev ** 2, padding_size=100, seq_len=seq_len)
        return viz.synthesis.MLPG(means=pred_deltas, variances=normaliser.delta_params_torch['std_dev'] ** 2, padding_size=100,
                                  seq_len=seq_len)

    _prepare_output = _trajectory      # the reference's name for it

    def _with_trajectories(self, outputs, n_frames, speaker_index=None):
        if self._generating():
            # a stream with a trajectory loss: the differentiable solve, on the current stream (its backward runs where autograd puts it)
            for st in self.streams:
                if st.is_delta and st.differentiable_trajectory:
                    if st.is_gaussian:
                        outputs[st.name] = self._trajectory(st.name, outputs[st.output_key], n_frames, speaker_index, differentiable=True,
                                                            norm_variance=outputs[st.output_key + '_variance'], variance_grad=True)
                    else:
                        outputs[st.name] = self._trajectory(st.name, outputs[st.output_key], n_frames, speaker_index, differentiable=True)
            delta = [st for st in self.streams if st.is_delta and not st.differentiable_trajectory]
            first = outputs[delta[0].output_key] if delta else None
            if len(delta) > 1 and TRAJECTORY_STREAMS and torch.is_tensor(first) and first.is_cuda:
                # The streams' trajectories are independent, and each MLPG launch is ONE dependent chain per (utterance, dimension) over
                # the frame axis on a few waves (lf0: 64 systems = one wave; mcep: 3,840): launched one after the other their chain
                # latencies add (the shipped acoustic model: 0.15 + 0.35 + 0.15 ms per step), side by side on streams of their own
                # they overlap.  Fork behind the current stream, join before anything reads a trajectory.
                main = torch.cuda.current_stream(first.device)
                pool = _trajectory_streams(first.device, len(delta))
                for st, side in zip(delta, pool):
                    side.wait_stream(main)
                    with torch.cuda.stream(side):
                        outputs[st.name] = self._trajectory(st.name, outputs[st.output_key], n_frames, speaker_index,
                                                            norm_variance=outputs.get(st.output_key + '_variance'))
                for st, side in zip(delta, pool):
                    main.wait_stream(side)
                    outputs[st.name].record_stream(main)
            else:
                for st in delta:
                    outputs[st.name] = self._trajectory(st.name, outputs[st.output_key], n_frames, speaker_index,
                                                        norm_variance=outputs.get(st.output_key + '_variance'))
        return outputs

    def _accumulate_metrics(self, features, outputs):
        if not self._generating():
            return
        n_frames = features['n_frames']
        predicted = {st.name for st in self.streams if not st.is_delta and not st.is_categorical}
        calls = {}
        for st in self.streams:
            if st.metric is None:
                continue
            metric_name, _, kind = st.metric
            if kind == 'accuracy' and st.is_categorical:
                hits = features[st.name].reshape(outputs[st.name].shape) == outputs[st.name]
                calls[metric_name] = (hits.type(torch.float).unsqueeze(-1), n_frames)
            elif kind == 'accuracy':
                calls[metric_name] = ((features[st.name] == (outputs[st.name] > 0.5)).type(torch.float), n_frames)
            elif kind == 'voiced_trajectory':
                voiced = (outputs[st.voicing] > 0.5) if st.voicing in predicted else features[st.voicing]
                calls[metric_name] = (features[st.name], outputs[st.name].detach(), voiced, n_frames)
            else:
                calls[metric_name] = (features[st.name], outputs[st.name].detach(), n_frames)
        self.metrics.accumulate(self.mode, **calls)

    def _target(self, features, st):
        return features[st.name] if st.is_categorical else features[st.output_key]

    def _trajectory_loss(self, features, output_features, st):
        """``trajectory_weight * trajectory_loss(normalise(trajectory), normalised target, n_frames) + gv_weight * losses.gv(the same
        three, log=gv_log)`` of a delta stream, whichever of the two weights is set: both sides through the stream's STATIC normaliser
        (per speaker when it is speaker-dependent), once, so the terms are on the scale of the delta loss next to them."""
        normaliser = self.normalisers[st.name]
        args = ()
        if isinstance(normaliser, data._SpeakerDependentNormaliser):
            speaker_index = features.get(data.SPEAKER_INDEX_KEY)
            if speaker_index is None:
                raise KeyError("the normaliser of %r is speaker-dependent: the batch needs features['%s'] (the loaders write it)"
                               % (st.name, data.SPEAKER_INDEX_KEY))
            args = (speaker_index,)
        target = features.get('normalised_' + st.name)
        if target is None:
            target = normaliser.normalise(features[st.name], *args)
        trajectory = normaliser.normalise(output_features[st.name], *args)
        total = None
        if st.trains_trajectory:
            score = st.trajectory_loss if st.trajectory_loss is not None else losses.mse
            total = st.trajectory_weight * score(trajectory, target, features['n_frames'])
        if st.trains_gv:
            term = st.gv_weight * losses.gv(trajectory, target, features['n_frames'], log=st.gv_log)
            total = term if total is None else total + term
        return total

    # -- the plugin surface ----------------------------------------------------------------------------------------------------------
    def predict(self, features):
        return self._with_trajectories(self._split(self._run_layers(features), seq_len=features['n_frames']), features['n_frames'],
                                       features.get(data.SPEAKER_INDEX_KEY))

    def loss(self, features, output_features):
        n_frames = features['n_frames']
        for st in self.streams:
            if st.trains_trajectory and not self._generating():
                raise RuntimeError("stream %r has trajectory_weight=%g, but there is no trajectory to score: the normaliser %r has no "
                                   "delta parameters (%s_deltas_mvn.json, or set_params(..., delta_params)) or the model was built with "
                                   "generate=False" % (st.name, st.trajectory_weight, st.name, st.name))
            if st.trains_gv and not self._generating():
                raise RuntimeError("stream %r has gv_weight=%g, but there is no trajectory to score: the normaliser %r has no "
                                   "delta parameters (%s_deltas_mvn.json, or set_params(..., delta_params)) or the model was built with "
                                   "generate=False" % (st.name, st.gv_weight, st.name, st.name))
        self._accumulate_metrics(features, output_features)
        total = 0.
        for st in self.streams:                           # delta streams first, then the probability streams: the reference's order
            if st.is_mdn:
                total = total + losses.mdn(output_features[st.name + '_mdn'], self._target(features, st), n_frames,
                                           n_components=st.n_components, min_log_std=st.min_log_std)
            elif st.is_gaussian:
                total = total + losses.gaussian(output_features[st.name + '_gaussian'], self._target(features, st), n_frames,
                                                min_log_std=st.min_log_std)
                if st.differentiable_trajectory:
                    total = total + self._trajectory_loss(features, output_features, st)
            elif st.is_delta:
                stream_loss = st.loss if callable(st.loss) else losses.mse
                total = total + stream_loss(output_features[st.output_key], self._target(features, st), n_frames)
                if st.differentiable_trajectory:
                    total = total + self._trajectory_loss(features, output_features, st)
        for st in self.streams:
            if not st.is_delta and not st.is_categorical:
                total = total + losses.bce(output_features[st.output_key].type(torch.float), self._target(features, st).type(torch.float),
                                           n_frames)
        for st in self.streams:                           # then the categorical streams, on their logits
            if st.is_categorical:
                total = total + losses.ce(output_features[st.output_key], self._target(features, st), n_frames)
        return total / float(len(self.streams)) if len(self.streams) > 1 else total

    def analysis_for_valid_batch(self, features, output_features, out_dir, sample_rate=16000, synthesiser=None, alpha=None, fft_size=None,
                                 frame_period=5., **kwargs):
        """Saves every stream's generated output per utterance under ``{out_dir}/feats/{stream}/{name}.npy``
        (``viz.io.save_batched_seqs``): the MLPG trajectory of a delta stream (present when the normalisers carry delta
        parameters, i.e. under ``ExperimentBuilder``), the probabilities of a 'sigmoid_bce' stream, the predicted classes of a 'ce'
        stream.  Nothing is written without an ``out_dir`` or without utterance names in ``features['name']``.

        models/RNN_SPSS.py:145-161 goes on to synthesise every utterance with WORLD.  Here everything up to the synthesiser runs on the
        device (``viz.synthesis.world_features``: the smoothed, voicing-gated F0, the spectral envelope of the mel-cepstrum, the
        full-band aperiodicity); the waveform synthesis itself is the caller's: ``synthesiser(f0, sp, ap, sample_rate) -> wav``, for
        example ``pyworld.synthesize`` (``pyworld`` is not a dependency of this package).  With a synthesiser, and the streams ``lf0``,
        ``vuv``, ``mcep`` and ``bap`` among the outputs, each utterance is written to ``{out_dir}/synth/{name}.wav`` at
        ``sample_rate``; ``alpha`` and ``fft_size`` as ``world_features`` takes them.  ``synthesiser=None`` (the default) writes
        exactly the feature files.  ``synthesiser='world'`` is the package's own synthesis (``viz.synthesis.synthesise_batch``,
        ``csrc/synth.hip``) at ``frame_period`` ms per frame: the whole batch in one pass, the spectra never leave the device and only
        the waveforms reach the host (``viz.synthesis.synthesise`` is the same synthesis as a callable, one utterance at a time)."""
        kwargs['sample_rate'] = sample_rate                     # models/RNN_SPSS.py:142: the base hooks see it
        super(StreamModel, self).analysis_for_valid_batch(features, output_features, out_dir, **kwargs)
        names = [st.name for st in self.streams if st.name in output_features]
        if out_dir is None or not names or features.get('name') is None:
            return
        # the classes of a categorical stream are (B, T): a trailing axis makes them a sequence feature that is cropped like the others
        outputs = [output_features[n].unsqueeze(-1) if output_features[n].ndim == 2 else output_features[n] for n in names]
        viz.io.save_batched_seqs(outputs, names=features['name'], out_dir=out_dir, seq_len=features['n_frames'], feat_names=names)
        if synthesiser is None:
            return
        missing = [n for n in ('lf0', 'vuv', 'mcep', 'bap') if n not in output_features]
        if missing:
            raise KeyError('analysis_for_valid_batch(synthesiser=...) needs the generated streams lf0, vuv, mcep and bap; %s %s not '
                           'among the outputs' % (', '.join(missing), 'is' if len(missing) == 1 else 'are'))
        synth_dir = os.path.join(out_dir, 'synth')
        os.makedirs(synth_dir, exist_ok=True)
        if isinstance(synthesiser, str):
            if synthesiser != 'world':
                raise ValueError("analysis_for_valid_batch: synthesiser=%r; the built-in synthesiser is 'world'" % (synthesiser,))
            waves = viz.synthesis.synthesise_batch(output_features['lf0'], output_features['vuv'], output_features['mcep'],
                                                   output_features['bap'], sample_rate, features['n_frames'], alpha=alpha,
                                                   fft_size=fft_size, frame_period=frame_period)
            for name, wav in zip(features['name'], waves):
                viz.io.save_wav(os.path.join(synth_dir, name + '.wav'), wav, sample_rate)
            return
        per_utterance = viz.synthesis.world_features(output_features['lf0'], output_features['vuv'], output_features['mcep'],
                                                     output_features['bap'], sample_rate, features['n_frames'], alpha=alpha,
                                                     fft_size=fft_size)
        for name, (f0, sp, ap) in zip(features['name'], per_utterance):
            viz.io.save_wav(os.path.join(synth_dir, name + '.wav'), synthesiser(f0, sp, ap, sample_rate), sample_rate)

    def forward(self, features):
        if not self.fused_loss:
            return super(StreamModel, self).forward(features)
        prediction = self._run_layers(features)
        targets = [self._target(features, st) for st in self.streams]
        kinds = [st.loss for st in self.streams]
        classes = None
        if 'ce' in kinds:
            loss, probabilities, by_index = losses.multi_stream(prediction, targets, kinds, features['n_frames'],
                                                                want_prob='sigmoid_bce' in kinds, widths=[st.width for st in self.streams],
                                                                want_argmax=True)
            classes = {self.streams[k].name: argmax for k, argmax in by_index.items()}
        else:
            loss, probabilities = losses.multi_stream(prediction, targets, kinds, features['n_frames'], want_prob=True)
        outputs = self._with_trajectories(self._split(prediction.detach(), probabilities, classes), features['n_frames'],
                                          features.get(data.SPEAKER_INDEX_KEY))
        self._accumulate_metrics(features, outputs)
        return loss, outputs


def _lstm_stack(input_dim, hidden_dim, post_dim, output_dim, num_layers, dropout_prob, precision):
    """models/RNN_SPSS.py:32-42 (the container order fixes the reference's state_dict keys)."""
    return utils.SequentialWithRecurrent(
        nn.Linear(input_dim, hidden_dim), nn.Sigmoid(), nn.Dropout(p=dropout_prob),
        *[utils.RecurrentCuDNNWrapper(nn.LSTM(hidden_dim, hidden_dim, dropout=dropout_prob, batch_first=True), precision=precision)
          for _ in range(num_layers)],
        nn.Linear(hidden_dim, post_dim), nn.Sigmoid(), nn.Dropout(p=dropout_prob),
        nn.Linear(post_dim, output_dim),
        precision=precision)


def _gru_f0_stack(input_dim, output_dim, dropout_prob, precision):
    """models/f0_test_model.py:28-45."""
    def gru(n_in):
        return utils.RecurrentCuDNNWrapper(nn.GRU(n_in, 64, batch_first=True), precision=precision)
    return utils.SequentialWithRecurrent(
        nn.Linear(input_dim, 256), nn.Sigmoid(), nn.Dropout(p=dropout_prob),
        gru(256), nn.Dropout(p=dropout_prob), gru(64), nn.Dropout(p=dropout_prob), gru(64), nn.Dropout(p=dropout_prob),
        nn.Linear(64, 64), nn.Sigmoid(), nn.Dropout(p=dropout_prob),
        nn.Linear(64, output_dim),
        precision=precision)


class LSTMAcousticModel(StreamModel):
    """The reference's shipped acoustic model (models/RNN_SPSS.py:20-139) as a stream table: lf0 / mcep / bap delta streams with
    masked MSE, a vuv probability stream with masked BCE, loss = their mean; LF0 RMSE in Hz over the frames the model calls voiced,
    V/UV accuracy, mel-cepstral and band-aperiodicity distortion (:44-48, :120-129).  Same constructor arguments and state_dict keys
    (``layers.0.weight`` ... ``layers.{3+k}.layer.weight_ih_l0`` ...).  ``trajectory_weight`` > 0 adds the trajectory loss of ``Stream``
    to the three delta streams, ``gv_weight`` > 0 its global-variance loss; either needs ``fused_loss=False``."""

    STREAMS = ('lf0', 'vuv', 'mcep', 'bap')

    def __init__(self, input_dim=600 + 9, output_dims=None, dropout_prob=0., num_layers=8, hidden_dim=512, post_dim=256,
                 precision=None, fused_upsample=True, fused_loss=True, generate=True, speaker_id_list=None, trajectory_weight=0.,
                 gv_weight=0.):
        if output_dims is None:
            output_dims = {'lf0': 1 * 3, 'vuv': 1, 'mcep': 60 * 3, 'bap': 5 * 3}
        self.input_dim, self.output_dims, self.dropout_prob, self.num_layers = input_dim, output_dims, dropout_prob, num_layers
        table = {'lf0': Stream('lf0', output_dims['lf0'], 'mse', ('LF0_RMSE_Hz', metrics.LF0Distortion, 'voiced_trajectory'),
                               trajectory_weight=trajectory_weight, gv_weight=gv_weight),
                 'vuv': Stream('vuv', output_dims['vuv'], 'sigmoid_bce', ('VUV_accuracy', metrics.Mean, 'accuracy')),
                 'mcep': Stream('mcep', output_dims['mcep'], 'mse', ('MCEP_distortion', metrics.MelCepDistortion, 'trajectory'),
                                trajectory_weight=trajectory_weight, gv_weight=gv_weight),
                 'bap': Stream('bap', output_dims['bap'], 'mse', ('BAP_distortion', metrics.Distortion, 'trajectory'),
                               trajectory_weight=trajectory_weight, gv_weight=gv_weight)}
        layers = _lstm_stack(input_dim, hidden_dim, post_dim, sum(output_dims.values()), num_layers, dropout_prob, precision)
        super(LSTMAcousticModel, self).__init__(layers, [table[name] for name in self.STREAMS], fused_upsample=fused_upsample,
                                                fused_loss=fused_loss, generate=generate, speaker_id_list=speaker_id_list)


class GRUF0Model(StreamModel):
    """The reference's shipped F0 model (models/f0_test_model.py:21-107) as a one-row stream table: the lf0 delta stream with masked
    MSE and the LF0 RMSE in Hz over the frames the DATA calls voiced (``features['vuv']``, :101-103).  Same constructor arguments and
    state_dict keys (``layers.0.weight``, ``layers.3.layer.weight_ih_l0`` ...).  ``n_components`` > 0 makes the lf0 stream a
    mixture-density stream of that many components (``Stream(loss='mdn')``; ``min_log_std``: its floor) and the last Linear
    ``n_components * (1 + 2 * output_dim)`` wide; 0 is the reference's model.  ``predict_variance=True`` makes it a 'gaussian' stream
    (``Stream(loss='gaussian')``: mean and log standard deviation per frame, the last Linear ``2 * output_dim`` wide), which composes
    with ``trajectory_weight``, ``gv_weight`` and ``min_log_std`` and is refused together with ``n_components`` > 0."""

    def __init__(self, dropout_prob=0., input_dim=600 + 9, output_dim=1 * 3, precision=None, fused_upsample=True, generate=True,
                 speaker_id_list=None, trajectory_weight=0., n_components=0, min_log_std=None, gv_weight=0., predict_variance=False):
        self.input_dim, self.output_dim = input_dim, output_dim
        if predict_variance and n_components > 0:
            raise ValueError('GRUF0Model: predict_variance=True is one Gaussian per frame; it does not go with n_components=%r (a '
                             'mixture-density stream)' % (n_components,))
        if predict_variance:
            stream = Stream('lf0', output_dim, 'gaussian', ('LF0_RMSE_Hz', metrics.LF0Distortion, 'voiced_trajectory'),
                            trajectory_weight=trajectory_weight, min_log_std=min_log_std, gv_weight=gv_weight)
        elif n_components > 0:
            stream = Stream('lf0', output_dim, 'mdn', ('LF0_RMSE_Hz', metrics.LF0Distortion, 'voiced_trajectory'),
                            trajectory_weight=trajectory_weight, n_components=n_components, min_log_std=min_log_std,
                            gv_weight=gv_weight)
        else:
            stream = Stream('lf0', output_dim, 'mse', ('LF0_RMSE_Hz', metrics.LF0Distortion, 'voiced_trajectory'),
                            trajectory_weight=trajectory_weight, min_log_std=min_log_std, gv_weight=gv_weight)
        layers = _gru_f0_stack(input_dim, stream.width, dropout_prob, precision)
        streams = [stream]
        super(GRUF0Model, self).__init__(layers, streams, fused_upsample=fused_upsample, fused_loss=False, generate=generate,
                                         speaker_id_list=speaker_id_list)


class VAEF0Model(StreamModel, BaseVAE):
    """``GRUF0Model`` as the decoder of a VAE (``BaseVAE``): the encoder, a GRU over ``normalised_lf0_deltas`` (valid frames only), gives
    mean | log_variance of an utterance-level latent through one Linear on its last state; the latent is sampled on the HIP path and
    appended to every frame of the decoder's input (``utils.concat_frame_features(..., latent)``: one gather pass, its gradient summed
    per utterance by the first layer's run).  Loss = the lf0 stream's masked MSE + ``kld_weight`` * KLD; ``kld`` is a metric of every
    collection.  State_dict keys: the decoder's ``layers.*`` as ``GRUF0Model`` (input ``input_dim + z_dim`` wide),
    ``encoder.0.layer.*`` and ``encoder_projection.0.*``.  ``encoder_pooling``: what of the encoder's output sequence goes into the
    projection - 'last' (the GRU's last state, the default), or the 'mean' / 'max' over each utterance's valid frames
    (``utils.pool_segments``); the parameters and their keys are the same in every case."""

    ENCODER_POOLINGS = ('last', 'mean', 'max')

    def __init__(self, z_dim=16, kld_weight=1., encoder_hidden=64, dropout_prob=0., input_dim=600 + 9, output_dim=1 * 3, precision=None,
                 fused_upsample=True, generate=True, speaker_id_list=None, trajectory_weight=0., gv_weight=0., encoder_pooling='last'):
        if encoder_pooling not in self.ENCODER_POOLINGS:
            raise ValueError('VAEF0Model: encoder_pooling must be one of %s, got %r' % (self.ENCODER_POOLINGS, encoder_pooling))
        self.input_dim, self.output_dim, self.encoder_pooling = input_dim, output_dim, encoder_pooling
        layers = _gru_f0_stack(input_dim + z_dim, output_dim, dropout_prob, precision)
        streams = [Stream('lf0', output_dim, 'mse', ('LF0_RMSE_Hz', metrics.LF0Distortion, 'voiced_trajectory'),
                          trajectory_weight=trajectory_weight, gv_weight=gv_weight)]
        super(VAEF0Model, self).__init__(layers, streams, fused_upsample=fused_upsample, fused_loss=False, generate=generate,
                                         speaker_id_list=speaker_id_list)
        self.z_dim, self.kld_weight = z_dim, kld_weight
        # the encoder's parameters go first in parameters() (and so in the optimiser's flat buffer): behind the decoder's 3-wide output
        # bias they would sit at offsets that are not 16-byte aligned, and the one-launch GRU-64 forward needs an aligned w_hh (with a
        # misaligned one the recurrence falls back to a launch per frame: 5.6 ms of a 64 x 1000 step instead of 0.8)
        layers = self._modules.pop('layers')
        self.encoder = utils.SequentialWithRecurrent(
            utils.RecurrentCuDNNWrapper(nn.GRU(output_dim, encoder_hidden, batch_first=True), precision=precision), precision=precision)
        self.encoder_projection = utils.SequentialWithRecurrent(nn.Linear(encoder_hidden, 2 * z_dim), precision=precision)
        self.layers = layers

    def encode(self, features):
        deltas = features['normalised_lf0_deltas']
        output, hiddens = self.encoder(deltas, seq_len=features['n_frames'], max_len=deltas.shape[1])
        if self.encoder_pooling == 'last':
            summary = hiddens[0][0]
        else:
            n_frames = features['n_frames'].reshape(-1)
            summary = utils.pool_segments(output, n_frames.reshape(-1, 1), self.encoder_pooling, seq_len=n_frames)[:, 0]
        statistics, _ = self.encoder_projection(summary)
        return statistics[:, :self.z_dim], statistics[:, self.z_dim:]

    def decode(self, latent, features):
        norm_counters = features['normalised_counters']
        norm_lab_at_frame_rate = utils.upsample_to_repetitions(features['normalised_lab'], features['dur'],
                                                               max_len=norm_counters.shape[1], fused=self.fused_upsample,
                                                               phone_rate=self.phone_rate)
        model_inputs = utils.concat_frame_features(norm_lab_at_frame_rate, norm_counters, latent)
        prediction, _ = self.layers(model_inputs, seq_len=features['n_frames'], max_len=norm_counters.shape[1])
        return self._with_trajectories(self._split(prediction, seq_len=features['n_frames']), features['n_frames'],
                                       features.get(data.SPEAKER_INDEX_KEY))

    forward = BaseVAE.forward
    predict = BaseVAE.predict

    def loss(self, features, output_features):
        kld = losses.KLD_standard_normal(output_features['mean'], output_features['log_variance'])
        if self.mode in self.metrics.collections:
            self.metrics.accumulate(self.mode, kld=kld)
        return StreamModel.loss(self, features, output_features) + self.kld_weight * kld


# ---------------------------------------------------------------------------------------------------------------------------------
# The first stage of the SPSS chain: the durations the acoustic models above read as ``dur`` / ``counters`` / ``n_frames``.
# ---------------------------------------------------------------------------------------------------------------------------------
class DurationModel(BaseSPSS):
    """Phone-rate duration model: ``normalised_lab`` (B, P, input_dim) -> ``normalised_dur`` (B, P, n_states), the stack of the shipped
    F0 model (Linear-256 / sigmoid / GRU-64 x 3 / Linear-64 / sigmoid / Linear-n_states) run once per phone with
    ``seq_len=features['n_phones']``, masked MSE against ``features['normalised_dur']`` (what ``collate_to_device`` writes for the
    ``dur`` normaliser the reference's shipped models list and never read).  ``n_states`` = 1 predicts phone durations, 5 HTS state
    durations.  With ``speaker_id_list`` the ``dur`` normaliser is per speaker.

    ``predict`` returns ``normalised_dur`` (with gradient) and - once the ``dur`` normaliser has parameters - the quantiser's detached
    ``dur`` int64 (B, P, n_states), ``phone_dur`` (B, P), ``n_frames`` (B,) and ``dur_flags`` int32 (B,) (``data.quantise_durations``
    with this model's ``rounding``, ``min_frames``, ``max_frames``: one launch).  After ``fit_to('n_frames')`` an ``eval()``-mode
    ``predict`` fits every utterance to ``features['n_frames']`` frames, so that acoustic metrics can score a prediction made with
    predicted durations against natural targets; ``train()`` mode never does.  Metric ``DUR_RMSE_frames``: RMSE in frames of the
    de-normalised real-valued prediction against ``features['dur']`` over the valid phones.

    The layers run through the wrappers one after the other (no ``max_len``: the three GRU-64 layers take the workgroup-local
    recurrence of csrc/gru_small.hip, which admits any B and any T >= 1, not the cross-workgroup wavefront), eager."""

    def __init__(self, input_dim=600, n_states=1, dropout_prob=0., precision=None, speaker_id_list=None, rounding='carry', min_frames=1,
                 max_frames=None):
        super(DurationModel, self).__init__()
        if int(n_states) < 1:
            raise ValueError('DurationModel: n_states must be at least 1, got %r' % (n_states,))
        ops.duration_arguments('DurationModel', 1., min_frames, max_frames, rounding)
        self.input_dim, self.n_states, self.speaker_id_list = input_dim, int(n_states), speaker_id_list
        self.rounding, self.min_frames, self.max_frames = rounding, min_frames, max_frames
        self.layers = _gru_f0_stack(input_dim, self.n_states, dropout_prob, precision)
        self.metrics.add_metrics('all', DUR_RMSE_frames=metrics.RMSE())

    def normaliser_sources(self):
        dur = (data.SpeakerDependentMeanVarianceNormaliser('dur', self.speaker_id_list) if self.speaker_id_list is not None
               else data.MeanVarianceNormaliser('dur'))
        return {'lab': data.MinMaxNormaliser('lab'), 'dur': dur}

    # -- fitting the utterance length ------------------------------------------------------------------------------------------------
    _fit_key = None               # the feature an eval()-mode predict fits every utterance's length to

    def fit_to(self, total_key='n_frames'):
        """In ``eval()`` mode every ``predict`` from now on hands the quantiser ``total=features[total_key]``: the durations of
        utterance b add up to that many frames (exactly, with 'carry' rounding, unless ``min_frames`` pushes the length out:
        ``ops.DUR_FLAG_PUSHED`` in ``dur_flags``).  ``fit_to(None)`` restores the default, the rounded predicted length.  In ``train()``
        mode nothing changes.  Returns the model."""
        if total_key is not None and not isinstance(total_key, str):
            raise TypeError('fit_to: total_key must be a feature name or None, got %r' % (total_key,))
        self._fit_key = total_key
        return self

    # -- pieces ----------------------------------------------------------------------------------------------------------------------
    def _dur_normaliser(self):
        norm = self.normalisers.get('dur') if hasattr(self.normalisers, 'get') else None
        return norm if norm is not None and norm.params else None

    def _speaker_args(self, normaliser, features):
        if not isinstance(normaliser, data._SpeakerDependentNormaliser):
            return None
        speaker_index = features.get(data.SPEAKER_INDEX_KEY)
        if speaker_index is None:
            raise KeyError("the normaliser of 'dur' is speaker-dependent: the batch needs features['%s'] (the loaders write it)"
                           % data.SPEAKER_INDEX_KEY)
        return speaker_index

    # -- the plugin surface ----------------------------------------------------------------------------------------------------------
    def predict(self, features):
        lab = features['normalised_lab']
        n_phones = features['n_phones'].reshape(-1)
        pred, _ = self.layers(lab, seq_len=n_phones)
        if pred.shape[1] != lab.shape[1]:                 # the wrappers crop to the longest item: back to the batch's phone axis
            pred = nn.functional.pad(pred, (0, 0, 0, lab.shape[1] - pred.shape[1]))
        outputs = {'normalised_dur': pred}
        normaliser = self._dur_normaliser()
        if normaliser is not None:
            total = None
            if self._fit_key is not None and not self.training:
                total = features[self._fit_key].reshape(-1)
            dur, phone_dur, n_frames, flags = data.quantise_durations(
                pred.detach(), n_phones=n_phones, normaliser=normaliser, speaker_index=self._speaker_args(normaliser, features),
                min_frames=self.min_frames, max_frames=self.max_frames, rounding=self.rounding, total=total)
            outputs.update(dur=dur, phone_dur=phone_dur, n_frames=n_frames, dur_flags=flags)
        return outputs

    def loss(self, features, output_features):
        pred = output_features['normalised_dur']
        normaliser = self._dur_normaliser()
        if normaliser is not None and 'dur' in features and self.mode in self.metrics.collections:
            speaker_index = self._speaker_args(normaliser, features)
            frames = normaliser.denormalise(pred.detach(), *(() if speaker_index is None else (speaker_index,)))
            self.metrics.accumulate(self.mode, DUR_RMSE_frames=(features['dur'].reshape(frames.shape).to(torch.float32), frames,
                                                                features['n_phones'].reshape(-1)))
        return losses.mse(pred, features['normalised_dur'], features['n_phones'])


_PHONE_LEVEL = ('lab',)


def _is_phone_level(key):
    base = key[len('normalised_'):] if key.startswith('normalised_') else key
    for suffix in (data.BF16_TABLE_SUFFIX, data.X3_TABLE_SUFFIX):
        if base.endswith(suffix):
            base = base[:-len(suffix)]
    return base in _PHONE_LEVEL


def with_predicted_durations(features, duration_outputs, normalisers, counters_kind='full', max_len=None):
    """The feature dict an acoustic ``StreamModel`` reads, built from a batch and a ``DurationModel``'s outputs for it: a NEW dict,
    ``features`` is untouched.  Written from ``duration_outputs``: ``dur`` int64 (B, P, 1), the phone durations in the shape the
    acoustic models read; with state durations (n_states > 1) ``state_dur`` int64 (B, P, S) as well; ``n_frames`` int64 (B,); and
    ``counters`` / ``normalised_counters`` (B, T, C), the frame-level positional features of the state durations where there are any,
    else of the phone durations (``ops.frame_counters``, ``counters_kind``; normalised with the operands of ``normalisers['counters']``,
    plain or speaker dependent, when there is one): one launch.  Kept from ``features``: everything that is not a batched sequence -
    names, ``n_phones``, ``speaker_index``, other per-item values - and the phone-level sequences (``lab`` / ``normalised_lab`` and their
    operand tables).  Dropped: every other batched sequence - the frame-level corpus features (targets, ``vuv``, natural ``counters``),
    which are as long as the natural durations - and ``normalised_dur``, ``n_frames_total``.

    ``max_len``: T, the frame axis of the counters (frames past an utterance's ``n_frames`` are zeros, longer utterances are cut).
    ``max_len=None`` takes the longest predicted utterance, which costs the one device -> host read of ``n_frames.max()``."""
    missing = [key for key in ('dur', 'phone_dur', 'n_frames') if key not in duration_outputs]
    if missing:
        raise KeyError('with_predicted_durations: duration_outputs lacks %s (a DurationModel writes them once its \'dur\' normaliser has '
                       'parameters)' % ', '.join(missing))
    state_dur, phone_dur, n_frames = (duration_outputs[key].detach() for key in ('dur', 'phone_dur', 'n_frames'))
    if state_dur.dim() == 2:
        state_dur = state_dur.unsqueeze(-1)
    batch_size = state_dur.shape[0]
    written = ('dur', 'state_dur', data.FRAME_COUNT_KEY, data.FRAME_COUNT_KEY + '_total', 'counters', 'normalised_counters',
               'normalised_dur')
    out = {}
    for key, value in features.items():
        if key in written:
            continue
        sequence = (isinstance(value, torch.Tensor) and value.dim() >= 2 and value.shape[0] == batch_size and
                    not (value.dim() == 2 and value.shape[1] == 1))
        if not sequence or _is_phone_level(key):
            out[key] = value
    out['dur'] = phone_dur.unsqueeze(-1)
    source = out['dur']
    if state_dur.shape[2] > 1:
        out['state_dur'] = source = state_dur
    out[data.FRAME_COUNT_KEY] = n_frames
    n_phones = features.get('n_phones')
    if n_phones is not None:
        n_phones = n_phones.reshape(-1).to(device=source.device, dtype=torch.int64)
    normaliser = normalisers.get('counters') if normalisers is not None else None
    kind, p0, p1, item_row = data._normaliser_operands(out, 'counters', normaliser, source.device)
    if max_len is None:
        max_len = int(n_frames.max().item())
    raw, norm = ops.frame_counters(source, t=int(max_len), kind=counters_kind, seq_len=n_frames, n_phones=n_phones, p0=p0, p1=p1,
                                   norm_kind=kind, item_row=item_row)
    out['counters'] = raw
    if norm is not None:
        out['normalised_counters'] = norm
    return out
