"""Import paths of the reference's encoder package (tgm/nn/encoder/__init__.py:1-15) for the encoders on the hot path:
``from tgm.nn.encoder.tgn import GraphAttentionEmbedding, LastAggregator, ...`` is how examples/linkproppred/tgn.py:25-31 reaches
them.  The submodule names resolve to the modules that hold the implementations -- nothing is defined here."""
import sys

from .. import ctan, dygformer, gclstm, roland, tgat, tgcn, tgn, tpnet
from ..ctan import CTAN, CTANMemory
from ..dygformer import DyGFormer
from ..gclstm import GCLSTM
from ..roland import ROLAND
from ..tgat import TGAT
from ..tgcn import TGCN
from ..tpnet import RandomProjectionModule, TPNet
from ..tgn import GraphAttentionEmbedding, IdentityMessage, LastAggregator, MeanAggregator, TGNMemory

for _m in (ctan, dygformer, gclstm, roland, tgat, tgcn, tgn, tpnet):
    sys.modules[f'{__name__}.{_m.__name__.rsplit(".", 1)[1]}'] = _m

__all__ = ['CTAN', 'CTANMemory', 'DyGFormer', 'GCLSTM', 'GraphAttentionEmbedding', 'IdentityMessage', 'LastAggregator', 'MeanAggregator', 'ROLAND', 'RandomProjectionModule', 'TGAT', 'TGCN', 'TGNMemory', 'TPNet']
