"""Import paths of the reference's decoder package: ``from tgm.nn.decoder.ncnpred import NCNPredictor``,
``from tgm.nn.decoder.linkproppred import LinkPredictor``.  The submodule names resolve to the modules that hold the implementations --
nothing is defined here."""
import sys

from .. import graphproppred, linkproppred, ncn, nodeproppred
from ..graphproppred import GraphPredictor
from ..linkproppred import LinkPredictor
from ..ncn import NCNPredictor
from ..nodeproppred import NodePredictor

for _m in (graphproppred, linkproppred, nodeproppred):
    sys.modules[f'{__name__}.{_m.__name__.rsplit(".", 1)[1]}'] = _m
sys.modules[f'{__name__}.ncnpred'] = ncn
ncnpred = ncn

__all__ = ['GraphPredictor', 'NodePredictor', 'LinkPredictor', 'NCNPredictor']
