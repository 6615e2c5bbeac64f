import sys as _sys

from .base import BaseDGHook, DGHook, SeedableHook, StatefulHook, StatelessHook
from .dedup import DeduplicationHook
from .edge_list import SampledEdgeListHook
from .hook_manager import HookManager
from .negatives import HistoricalNegativeEdgeSamplerHook, RandomNegativeEdgeSamplerHook
from .recency import RecencyNeighborHook
from .uniform import NeighborSamplerHook
from .time_gap import TimeGapNeighborHook
from .registry import hook, list_hooks
from . import neighbors  # noqa: E402,F401  (the reference's import path: tgm.hooks.neighbors.recency)
from .analytics import BatchAnalyticsHook, NodeAnalyticsHook
from .device import DeviceTransferHook, PinMemoryHook
from .node_tracks import EdgeEventsSeenNodesTrackHook
from . import negatives, tgb_sampler  # noqa: E402
from .tgb_sampler import TGBNegativeEdgeSamplerHook, TGBTHGNegativeEdgeSamplerHook, TGBTKGNegativeEdgeSamplerHook
from ..core.neg_batch_list import NegBatchList

# the reference's import path, tgm.hooks.negatives.tgb_sampler (our negatives is one module, not a package)
negatives.tgb_sampler = tgb_sampler
_sys.modules[f'{__name__}.negatives.tgb_sampler'] = tgb_sampler
from .recipe import RecipeRegistry  # noqa: E402  (after the hooks it registers)

__all__ = [
    'BaseDGHook',
    'BatchAnalyticsHook',
    'DGHook',
    'DeduplicationHook',
    'DeviceTransferHook',
    'EdgeEventsSeenNodesTrackHook',
    'HistoricalNegativeEdgeSamplerHook',
    'HookManager',
    'NegBatchList',
    'NeighborSamplerHook',
    'NodeAnalyticsHook',
    'PinMemoryHook',
    'RandomNegativeEdgeSamplerHook',
    'RecencyNeighborHook',
    'RecipeRegistry',
    'SampledEdgeListHook',
    'SeedableHook',
    'StatefulHook',
    'StatelessHook',
    'TGBNegativeEdgeSamplerHook',
    'TGBTHGNegativeEdgeSamplerHook',
    'TGBTKGNegativeEdgeSamplerHook',
    'TimeGapNeighborHook',
    'hook',
    'list_hooks',
]
