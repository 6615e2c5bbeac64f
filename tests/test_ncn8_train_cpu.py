"""The k = 8 NCNPredictor backward without a device: the entry points and their argument types, the workspace arithmetic (host only), and
the envelope of the native training path."""
import ctypes

import pytest
import torch

from tgm_amd import _native

P, I32, I64, SZ = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
BWD = ctypes.POINTER(_native.NcnBwd)


@pytest.mark.parametrize('name, restype, argtypes', [
    ('tgmx_ncn8_coef', I32, [I64, P, P, P, I32, I64, I64, P, P, P, I64, I64, P, I64, P, SZ, I32, P]),
    ('tgmx_ncn8_dx_pairs', I32, [P, I64, I32, P, I32, I64, I64, P, I64, P, P, SZ, P]),
    ('tgmx_ncn8_dx', I32, [P, I64, I32, P, P, P, I32, I64, I64, P, P, P, P, I64, P, I64, P, SZ, I32, P]),
    ('tgmx_ncn8_backward_workspace_bytes', SZ, [BWD, I64]),
    ('tgmx_ncn8_backward', I32, [BWD, I64, P]),
])  # fmt: skip
def test_entry_points_have_the_documented_types(name, restype, argtypes):
    f = getattr(_native.load(), name)
    assert f.restype is restype and list(f.argtypes) == argtypes


def test_backward_workspace_is_host_arithmetic():
    lib = _native.load()
    t = _native.NcnBwd()
    t.d_x = 256  # (never dereferenced: the workspace functions read sizes only)

    def need(N=1000, B=200, k=8, C=100, H=100, slab=0, E=3000):
        b = t.fwd
        b.N, b.B, b.E, b.k, b.C, b.H, b.out_ch, b.ldxs, b.ldh, b.tar_stride = N, B, E, k, C, H, 1, k * C, H, max(B, 1)
        return lib.tgmx_ncn8_backward_workspace_bytes(ctypes.byref(t), slab)

    assert need() >= 200 * 8 * 1024 * 4  # the whole batch in one slab of [8 B, ldT] floats
    assert need(slab=1) < need(slab=50) < need(slab=100) < need(slab=200) == need()  # grows with slab_pairs ...
    assert need(N=4000, slab=50) - need(N=2000, slab=50) >= 50 * 8 * 2000 * 4  # ... times N
    assert need(N=8000, B=500) > need(N=8000, B=500, slab=100) > 100 * 8 * 8000 * 4  # (past the LDS cap: count rows in the workspace too)
    for bad in (dict(k=4), dict(k=2), dict(N=0), dict(N=2**30), dict(B=-1), dict(B=2**30), dict(E=2**30), dict(H=8193), dict(slab=-1), dict(C=0)):
        assert need(**bad) == 0, bad
    assert need(B=0) > 0
    t.fwd.k, t.fwd.C = 8, 100
    assert lib.tgmx_ncn_backward_workspace_bytes(ctypes.byref(t)) == 0  # the k = 2 / 4 entry keeps refusing k = 8
    assert lib.tgmx_ncn8_backward_slab_pairs(1000, 200, 0) == 200 and lib.tgmx_ncn8_backward_slab_pairs(1000, 200, 3) == 3
    assert lib.tgmx_ncn8_backward_slab_pairs(10**6, 200, 0) == (256 << 20) // (32 * 1000000)  # the budget rule: 32 ldT bytes per pair


def test_envelope_of_the_native_training_path():
    from tgm_amd.nn import NCNPredictor, _ncn_train

    host = torch.zeros(3, 4)
    assert not _ncn_train.in_envelope(NCNPredictor(4, 8, 1, k=8), host)  # k = 8 is device-only
    assert _ncn_train.in_envelope(NCNPredictor(4, 8, 1, k=4), host)
