"""Sentinels shared with the reference (tgm/constants.py:3)."""
from typing import Final

PADDED_NODE_ID: Final[int] = -1
"""Node id marking an empty neighbor slot; never a valid node id."""

RECIPE_TGB_LINK_PRED: Final[str] = 'TGB_LINK_PROPERTY_PREDICTION'
"""Name of the recipe that sets a HookManager up for TGB link property prediction (``RecipeRegistry.build``)."""

METRIC_TGB_LINKPROPPRED: Final[str] = 'mrr'
"""The metric TGB's ``Evaluator`` reports for link property prediction."""

METRIC_TGB_NODEPROPPRED: Final[str] = 'ndcg'
"""The metric TGB's ``Evaluator`` reports for node property prediction."""
