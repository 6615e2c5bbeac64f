"""Import paths of the reference's module package (tgm/nn/modules/__init__.py) for the modules on the hot path."""
import sys

from .. import attention, mlp_mixer, time_encoding
from ..attention import TemporalAttention
from ..mlp_mixer import MLPMixer
from ..time_encoding import Time2Vec

for _m in (attention, mlp_mixer, time_encoding):
    sys.modules[f'{__name__}.{_m.__name__.rsplit(".", 1)[1]}'] = _m

__all__ = ['MLPMixer', 'TemporalAttention', 'Time2Vec']
