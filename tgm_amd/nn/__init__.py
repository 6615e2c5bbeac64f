from ._paramver import invalidate_parameter_caches
from .attention import TemporalAttention
from .base import EncoderModule
from .ctan import CTAN, CTANMemory
from .edgebank import EdgeBankPredictor
from .gclstm import GCLSTM, ChebConv
from .graphproppred import GraphPredictor
from .linkproppred import LinkPredictor
from .nodeproppred import NodePredictor
from .dygformer import DyGFormer, NeighborCooccurrenceEncoder, TransformerEncoder
from .graphmixer import GraphMixerEncoder
from .mlp_mixer import FeedForwardNet, MLPMixer
from .ncn import NCNPredictor
from .poptrack import PopTrackPredictor
from .roland import ROLAND
from .tcomem import tCoMemPredictor
from .tgat import TGAT, MergeLayer
from ._snapshot import GCNGraph, gcn_graph
from .tgcn import TGCN, GCNConv
from .tgn import GraphAttentionEmbedding, IdentityMessage, LastAggregator, MeanAggregator, TGNMemory, TGNStep, TransformerConv, sampled_edge_list
from .time_encoding import Time2Vec
from .tpnet import RandomProjectionModule, TPNet
from . import decoder, encoder, modules  # noqa: E402,F401  (the reference's import paths: tgm.nn.encoder.tgn, tgm.nn.modules.attention, ...)

__all__ = [
    'CTAN', 'CTANMemory', 'ChebConv', 'DyGFormer', 'EdgeBankPredictor', 'EncoderModule', 'FeedForwardNet', 'GCLSTM', 'GCNConv', 'GCNGraph', 'GraphAttentionEmbedding', 'GraphMixerEncoder', 'GraphPredictor', 'IdentityMessage', 'LastAggregator', 'LinkPredictor',
    'MLPMixer', 'MeanAggregator', 'MergeLayer', 'NCNPredictor', 'NeighborCooccurrenceEncoder', 'NodePredictor', 'PopTrackPredictor', 'ROLAND', 'RandomProjectionModule', 'TGAT', 'TGCN',
    'TGNMemory', 'TGNStep', 'TPNet', 'TemporalAttention', 'Time2Vec', 'TransformerConv', 'TransformerEncoder', 'gcn_graph', 'invalidate_parameter_caches', 'sampled_edge_list', 'tCoMemPredictor',
]  # fmt: skip
