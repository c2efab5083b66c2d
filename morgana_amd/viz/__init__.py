"""The part of ``morgana.viz`` that sits on the training path: ``synthesis.MLPG`` (called by ``predict`` of the shipped models) and
``io.save_batched_seqs`` (called by their ``analysis_for_valid_batch``)."""
from . import synthesis  # noqa: F401
from . import io  # noqa: F401
