"""Import paths of the reference's module package (tgm/nn/modules/__init__.py) for the modules on the hot path."""
import sys

from .. import attention, edgebank, mlp_mixer, poptrack, tcomem, time_encoding
from ..attention import TemporalAttention
from ..edgebank import EdgeBankPredictor
from ..mlp_mixer import MLPMixer
from ..poptrack import PopTrackPredictor
from ..tcomem import tCoMemPredictor
from ..time_encoding import Time2Vec

for _m in (attention, edgebank, mlp_mixer, poptrack, time_encoding):
    sys.modules[f'{__name__}.{_m.__name__.rsplit(".", 1)[1]}'] = _m
sys.modules[f'{__name__}.t_comem'] = tcomem  # the reference's file name
t_comem = tcomem

__all__ = ['EdgeBankPredictor', 'MLPMixer', 'PopTrackPredictor', 'TemporalAttention', 'Time2Vec', 'tCoMemPredictor']
