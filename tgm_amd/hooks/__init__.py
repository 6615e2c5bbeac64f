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

__all__ = [
    'BaseDGHook',
    'BatchAnalyticsHook',
    'DGHook',
    'DeduplicationHook',
    'DeviceTransferHook',
    'EdgeEventsSeenNodesTrackHook',
    'HistoricalNegativeEdgeSamplerHook',
    'HookManager',
    'NeighborSamplerHook',
    'NodeAnalyticsHook',
    'PinMemoryHook',
    'RandomNegativeEdgeSamplerHook',
    'RecencyNeighborHook',
    'SampledEdgeListHook',
    'SeedableHook',
    'StatefulHook',
    'StatelessHook',
    'TimeGapNeighborHook',
    'hook',
    'list_hooks',
]
