"""Import paths of the reference's module package (tgm/nn/modules/__init__.py) for the modules on the hot path."""
import sys

from .. import aggregation, attention, edgebank, mlp_mixer, poptrack, tcomem, time_encoding
from ..aggregation import Aggregator, ConcatMerge, LearnableSumMerge, MeanEmbdPooling, SumEmbdPooling
from ..attention import TemporalAttention
from ..edgebank import EdgeBankPredictor
from ..mlp_mixer import MLPMixer
from ..poptrack import PopTrackPredictor
from ..tcomem import tCoMemPredictor
from ..time_encoding import Time2Vec

for _m in (aggregation, attention, edgebank, mlp_mixer, poptrack, time_encoding):
    sys.modules[f'{__name__}.{_m.__name__.rsplit(".", 1)[1]}'] = _m
sys.modules[f'{__name__}.t_comem'] = tcomem  # the reference's file name
t_comem = tcomem

__all__ = ['Aggregator', 'ConcatMerge', 'EdgeBankPredictor', 'LearnableSumMerge', 'MLPMixer', 'MeanEmbdPooling', 'PopTrackPredictor', 'SumEmbdPooling',
           'TemporalAttention', 'Time2Vec', 'tCoMemPredictor']
