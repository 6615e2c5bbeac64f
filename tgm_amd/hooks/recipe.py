"""Named set-ups of a HookManager (the reference's ``tgm/hooks/recipe.py``): ``RecipeRegistry.register(name)`` decorates a builder,
``RecipeRegistry.build(name, **kwargs)`` calls it.  One recipe ships: ``RECIPE_TGB_LINK_PRED``, the hooks of TGB link property prediction."""
from __future__ import annotations

import logging
from typing import Any, Callable, Dict

from ..constants import RECIPE_TGB_LINK_PRED
from ..core import DGraph
from ..exceptions import UndefinedRecipe
from .hook_manager import HookManager
from .negatives import RandomNegativeEdgeSamplerHook
from .tgb_sampler import TGBNegativeEdgeSamplerHook

logger = logging.getLogger(__name__)


class RecipeRegistry:
    """Registry of pre-defined recipes, each a callable that returns a ready-to-use object (usually a HookManager).

    User-defined recipes are registered with :meth:`register` and built with :meth:`build`.

    Raises:
        UndefinedRecipe: If build is called on a recipe that is not defined or registered.
    """

    _recipes: Dict[str, Callable] = {}

    @classmethod
    def register(cls, name: str) -> Callable:
        def decorator(func: Callable) -> Callable:
            cls._recipes[name] = func
            return func

        return decorator

    @classmethod
    def build(cls, name: str, **kwargs: Any) -> Any:
        if name not in cls._recipes:
            raise UndefinedRecipe(f'Undefined or not yet registered recipe: {name}. Please select from {cls._recipes}')
        logger.debug("Building recipe '%s' with kwargs=%s", name, {k: str(v) for k, v in kwargs.items()})
        return cls._recipes[name](**kwargs)


@RecipeRegistry.register(RECIPE_TGB_LINK_PRED)
def build_tgb_link_pred(dataset_name: str, train_dg: DGraph) -> HookManager:
    """Build a ready-to-use HookManager with the default hooks of the TGB linkproppred task.

    Args:
        dataset_name (str): The name of the TGB dataset (e.g. 'tgbl-wiki')
        train_dg (DGraph): The training graph; its destination ids bound the training negatives

    Returns:
        HookManager with registered keys: ['train', 'val', 'test']
    """
    dst = train_dg.edge_dst
    hm = HookManager(keys=['train', 'val', 'test'])
    hm.register('train', RandomNegativeEdgeSamplerHook(low=int(dst.min()), high=int(dst.max())))
    hm.register('val', TGBNegativeEdgeSamplerHook(dataset_name, split_mode='val'))
    hm.register('test', TGBNegativeEdgeSamplerHook(dataset_name, split_mode='test'))
    logger.info("Built %s HookManager recipe for dataset '%s'. Hooks registered: %s", RECIPE_TGB_LINK_PRED, dataset_name, list(hm.keys))
    return hm
