"""CTAN's training path without a GPU: the restated backward (``ctan_bwd_restate.py``) against float64 autograd through
``ctan_restate.ctan_forward`` -- the formulas are pinned before any kernel runs --, its float32 evaluation inside its own bound,
``TGMX_CTAN_BWD`` parsing, the envelope's decisions and the ABI additions."""
import ctypes

import pytest
import torch

import ctan_bwd_restate as br
import ctan_restate as cr
from oracle.tgat_bwd_ref import EPS


def _case(seed, U, M, T, D, S, num_iters, E):
    g = torch.Generator().manual_seed(seed)
    shapes = cr.expected_shapes(D, M, T, S)
    p = {k: (torch.eye(M) if k == 'aconv.eye' else torch.randn(*s, generator=g) * (0.3 if len(s) == 2 and s[1] > 1 else 0.5)) for k, s in shapes.items()}
    base = 1_700_000_000
    args = (torch.randn(U, M + S, generator=g), base + torch.randint(0, 2000, (U,), generator=g),
            torch.stack([torch.randint(0, U, (E,), generator=g), torch.randint(0, U, (E,), generator=g)]), base + torch.randint(0, 2000, (E,), generator=g),
            torch.randn(E, D, generator=g))  # fmt: skip
    cfg = dict(num_iters=num_iters, mean_delta_t=300.5, std_delta_t=450.25, epsilon=0.5, gamma=0.3)
    return p, args, cfg, torch.randn(U, M, generator=g)


def _autograd(p, args, cfg, weight):
    p64 = {k: v.double().requires_grad_(k in cr.PARAMS) for k, v in p.items()}
    x64 = args[0].double().requires_grad_(True)
    (cr.ctan_forward(p64, x64, *args[1:], **cfg) * weight.double()).sum().backward()
    grads = {k: p64[k].grad for k in cr.PARAMS}
    grads['node_x'] = x64.grad
    return grads


CASES = [(1, 30, 8, 4, 5, 2, 2, 200), (2, 12, 5, 3, 2, 1, 3, 90), (3, 7, 6, 2, 3, 1, 0, 20), (4, 7, 6, 2, 3, 1, 2, 0), (5, 1, 4, 2, 1, 1, 1, 5)]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'U%d-M%d-it%d-E%d' % (c[1], c[2], c[6], c[7]))
def test_restated_backward_matches_float64_autograd(case):
    p, args, cfg, weight = _case(*case)
    want = _autograd(p, args, cfg, weight)
    got = br.backward(br.forward_saved(p, *args, **cfg), weight)
    assert sorted(got) == sorted(want)
    for name, ref in want.items():
        ref = torch.zeros_like(got[name][0]) if ref is None else ref  # (a parameter no path reaches: num_iters = 0, E = 0)
        scale = max(float(ref.abs().max()), 1e-3)
        err = float((got[name][0] - ref).abs().max()) / scale
        assert got[name][0].shape == ref.shape and err <= 1e-10, (name, err)
        assert (got[name][1] >= got[name][0].abs() * (1 - 1e-12)).all(), name  # a magnitude dominates its value


def test_float32_evaluation_stays_inside_its_bound():
    """The same formulas in float32 (saved activations through float32, as the device keeps them): |f32 - f64| <= chain 2^-24 magnitude."""
    p, args, cfg, weight = _case(*CASES[0])
    sv = br.forward_saved(p, *args, **cfg)
    for key in ('xs',):
        sv[key] = [x.float().double() for x in sv[key]]
    for key in ('out', 'edge_attr', 'ep'):
        sv[key] = sv[key].float().double()
    f64, f32 = br.backward(sv, weight), br.backward(sv, weight, dtype=torch.float32)
    U, E = args[0].shape[0], args[2].shape[1]
    chain = br.backward_chain(U, E, 8, 10, 9, 2, int(torch.bincount(sv['tgt']).max()), int(torch.bincount(sv['src']).max()))
    for name, (val, mag) in f64.items():
        ratio = float(((f32[name][0].double() - val).abs() / (chain * EPS * mag).clamp_min(1e-300)).max())
        assert f32[name][0].dtype == torch.float32 and ratio <= 1.0, (name, ratio)


def test_chains_are_derived_from_the_split():
    assert br.per_wave(16) == 16 and br.per_wave(17) == 5 and br.per_wave(1500) == 375 and br.per_wave(0) == 0
    assert br.per_wave(torch.tensor([0, 16, 17, 65])).tolist() == [0, 16, 5, 17]
    assert br.dot_chain(4) == 7 and br.dot_chain(256) == 10 and br.dot_chain(130) == 9
    assert br.attend_chain(256, 1500) > br.attend_chain(256, 17) > br.attend_chain(4, 0) > 8
    assert br.source_chain(1500) == 375 + 4 + 8


def test_mode_parsing(monkeypatch):
    from tgm_amd.nn import _ctan_train

    for value, want in ((None, 'native'), ('', 'native'), ('py', 'py'), ('torch', 'torch'), ('PY', 'native'), ('1', 'native')):
        if value is None:
            monkeypatch.delenv('TGMX_CTAN_BWD', raising=False)
        else:
            monkeypatch.setenv('TGMX_CTAN_BWD', value)
        assert _ctan_train.mode() == want == br.parse_mode(value)


def test_in_envelope_decisions(monkeypatch):
    from tgm_amd.nn import _ctan_train
    from tgm_amd.nn.encoder import CTAN

    monkeypatch.delenv('TGMX_CTAN_BWD', raising=False)
    enc = CTAN(edge_dim=3, memory_dim=8, time_dim=4, node_dim=1, num_iters=2)
    x, msg = torch.randn(5, 9), torch.randn(6, 3)
    assert _ctan_train.in_envelope(enc, x, msg)
    assert _ctan_train.in_envelope(enc, x.requires_grad_(True), msg)
    assert not _ctan_train.in_envelope(enc, x[:0], msg)  # U = 0
    assert not _ctan_train.in_envelope(enc, x, msg.clone().requires_grad_(True))
    assert not _ctan_train.in_envelope(enc, x.double(), msg) and not _ctan_train.in_envelope(enc, x, msg.long())
    assert _ctan_train.in_envelope(CTAN(edge_dim=3, memory_dim=256, time_dim=4, node_dim=1), torch.randn(5, 257), msg)
    assert not _ctan_train.in_envelope(CTAN(edge_dim=3, memory_dim=260, time_dim=4, node_dim=1), torch.randn(5, 261), msg)
    monkeypatch.setenv('TGMX_CTAN_BWD', 'torch')
    assert not _ctan_train.in_envelope(enc, x, msg)
    monkeypatch.setenv('TGMX_CTAN_BWD', 'py')
    assert _ctan_train.in_envelope(enc, x, msg)
    monkeypatch.delenv('TGMX_CTAN_BWD')
    with monkeypatch.context() as m:
        m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
        assert not _ctan_train.in_envelope(enc, x, msg)
    half = CTAN(edge_dim=3, memory_dim=8, time_dim=4, node_dim=1).double()
    assert not _ctan_train.in_envelope(half, x, msg)
    strided = CTAN(edge_dim=3, memory_dim=8, time_dim=4, node_dim=1)
    strided.aconv.W = torch.nn.Parameter(torch.randn(8, 16)[:, ::2])
    assert not strided.aconv.W.is_contiguous() and not _ctan_train.in_envelope(strided, x, msg)


def test_abi_additions():
    from tgm_amd import _native

    lib = _native.load()
    assert lib.tgmx_abi_sizeof(35) == ctypes.sizeof(_native.CtanBwd) > 0 and lib.tgmx_version() == 7
    assert lib.tgmx_abi_sizeof(22) == ctypes.sizeof(_native.CtanFwd) and lib.tgmx_abi_sizeof(34) == 0
    assert _native.CtanFwd._fields_[-1][0] == 'x_save' and _native.CtanFwd().x_save is None  # appended; null = the inference behaviour
    for name in ('tgmx_ctan_backward', 'tgmx_ctan_backward_workspace_bytes', 'tgmx_ctan_attend_backward', 'tgmx_ctan_source_backward',
                 'tgmx_ctan_edge_attr_backward', 'tgmx_ctan_antisym_grad', 'tgmx_ctan_out_backward'):  # fmt: skip
        assert name in _native.SIGNATURES and hasattr(lib, name)
    assert lib.tgmx_ctan_backward_workspace_bytes(None) == 0  # a null block is refused, not read
