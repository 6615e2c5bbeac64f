"""Import paths of the reference's module package (tgm/nn/modules/__init__.py) for the modules on the hot path."""
import sys

from .. import attention, edgebank, mlp_mixer, time_encoding
from ..attention import TemporalAttention
from ..edgebank import EdgeBankPredictor
from ..mlp_mixer import MLPMixer
from ..time_encoding import Time2Vec

for _m in (attention, edgebank, mlp_mixer, time_encoding):
    sys.modules[f'{__name__}.{_m.__name__.rsplit(".", 1)[1]}'] = _m

__all__ = ['EdgeBankPredictor', 'MLPMixer', 'TemporalAttention', 'Time2Vec']
