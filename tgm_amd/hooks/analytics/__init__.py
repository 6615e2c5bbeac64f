"""Import paths of the reference's analytics package (tgm/hooks/analytics/__init__.py)."""
from .batch_analytics import BatchAnalyticsHook
from .node_analytics import NodeAnalyticsHook

__all__ = ['BatchAnalyticsHook', 'NodeAnalyticsHook']
