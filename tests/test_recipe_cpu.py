"""RecipeRegistry (the reference's tgm/hooks/recipe.py): register / build / UndefinedRecipe and the TGB link-prediction recipe."""
import pytest
import torch

import tgbneg_cases as tc
from tgm_amd import DGData, DGraph
from tgm_amd.constants import RECIPE_TGB_LINK_PRED
from tgm_amd.exceptions import TGMError, UndefinedRecipe
from tgm_amd.hooks import HookManager, RandomNegativeEdgeSamplerHook, RecipeRegistry, TGBNegativeEdgeSamplerHook


@pytest.fixture
def dg():
    edge_index = torch.IntTensor([[1, 10], [1, 11], [1, 12], [1, 13]])
    return DGraph(DGData.from_raw(torch.LongTensor([1, 1, 2, 2]), edge_index))


def test_undefined_recipe(dg):
    assert issubclass(UndefinedRecipe, TGMError)
    with pytest.raises(UndefinedRecipe, match='Undefined or not yet registered recipe: nope'):
        RecipeRegistry.build('nope', dataset_name='tgbl-foo', train_dg=dg)


def test_register_and_build():
    calls = []

    @RecipeRegistry.register('test_recipe_cpu_mine')
    def mine(value: str):
        calls.append(value)
        return HookManager(['global']), value

    try:
        hm, out = RecipeRegistry.build('test_recipe_cpu_mine', value='x')
        assert isinstance(hm, HookManager) and out == 'x' and calls == ['x'] and mine('y')[1] == 'y'  # the decorator hands the function back
    finally:
        del RecipeRegistry._recipes['test_recipe_cpu_mine']


def test_tgb_link_pred_recipe(dg):
    tc.ensure_tgb()
    assert RECIPE_TGB_LINK_PRED == 'TGB_LINK_PROPERTY_PREDICTION'
    hm = RecipeRegistry.build(RECIPE_TGB_LINK_PRED, dataset_name='tgbl-foo', train_dg=dg)
    assert list(hm.keys) == ['train', 'val', 'test']
    train, val, test = (hm._key_to_hooks[k] for k in ('train', 'val', 'test'))
    assert len(train) == len(val) == len(test) == 1
    assert isinstance(train[0], RandomNegativeEdgeSamplerHook) and (train[0].low, train[0].high) == (10, 13)
    assert isinstance(val[0], TGBNegativeEdgeSamplerHook) and val[0].split_mode == 'val'
    assert isinstance(test[0], TGBNegativeEdgeSamplerHook) and test[0].split_mode == 'test'
    with pytest.raises(ValueError, match='should only be registered for "tgbl-xxx" datasets'):
        RecipeRegistry.build(RECIPE_TGB_LINK_PRED, dataset_name='tgbn-trade', train_dg=dg)
