"""Import path of the reference's decoder package: ``from tgm.nn.decoder.ncnpred import NCNPredictor``.  The submodule name resolves to
the module that holds the implementation -- nothing is defined here."""
import sys

from .. import ncn
from ..ncn import NCNPredictor

sys.modules[f'{__name__}.ncnpred'] = ncn
ncnpred = ncn

__all__ = ['NCNPredictor']
