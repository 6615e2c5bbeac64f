"""DensityOfStateEstimatorHook's CSR route (csrc/dos_large.hip) without a device: the struct mirror, the envelope and its mirror, the size of
the workspace, and the route the hook records for host tensors."""
import ctypes
import types

import pytest
import torch

from tgm_amd import _native
from tgm_amd.hooks import DensityOfStateEstimatorHook
from tgm_amd.hooks.analytics import dos as D


def test_struct_mirror():
    assert _native.load().tgmx_abi_sizeof(45) == ctypes.sizeof(_native.DosLarge) > 0


@pytest.mark.parametrize('args', [(4096, 1, 2, 2), (4097, 1, 2, 2), (1 << 22, 1024, 64, 65536), ((1 << 22) + 1, 1, 2, 2), (4097, 1025, 2, 2),
                                  (4097, 1, 1, 2), (4097, 1, 65, 2), (4097, 1, 2, 1), (4097, 1, 2, 65537)])  # fmt: skip
def test_envelope_and_its_mirror(args):
    lib = _native.load()
    inside = 4096 < args[0] <= 1 << 22 and args[1] <= 1024 and 2 <= args[2] <= 64 and 2 <= args[3] <= 65536
    assert bool(lib.tgmx_dos_large_supported(*args)) == D.large_supported(*args) == (lib.tgmx_dos_large_workspace_bytes(*args) > 0) == inside


def test_workspace_is_not_quadratic():
    # the largest call of the envelope against what the composed path's two dense [n, n] float32 matrices take at n = 65 536
    assert _native.load().tgmx_dos_large_workspace_bytes(1 << 22, 1024, 64, 65536) < 2 * 65536 * 65536 * 4


def test_host_path_is_recorded():
    hook = DensityOfStateEstimatorHook(4, 3, 5, seed=1)
    assert hook.last_path is None
    hook(None, types.SimpleNamespace(edge_src=torch.tensor([1, 2]), edge_dst=torch.tensor([2, 3])))
    assert hook.last_path == 'host'
