"""TransformerConv training for wide heads (csrc/tconv_bwd.hip): the deterministic attention backward against its float64 restatement
(oracle/tgn_bwd_ref.py: the cases, expected values and bounds n * 2^-24 * magnitude are the oracle's; the kernels' chains are no longer
than ``attend_chain`` counts, see the comment at the top of tconv_bwd.hip), and GraphAttentionEmbedding's one-node training path against
float64 autograd through oracle/tgn_ref.py with the device's dropout mask."""
import functools

import numpy as np
import pytest
import torch

from oracle import tgn_bwd_ref as ref
from test_tgat_bwd_blocks_gpu import DEV, Buf, _lib, _report, _same_bits

pytestmark = pytest.mark.gpu

# the issue's six, then the two widest lane pieces: (2, 256) -> 8 floats per lane, (5, 102) -> 16 (eight lanes per head, H C = 510)
ATTEND_CASES = [(1, 65, 0.0), (2, 86, 0.1), (2, 128, 0.5), (1, 256, 0.1), (3, 33, 0.5), (2, 64, 0.0), (2, 256, 0.1), (5, 102, 0.5)]


@pytest.mark.parametrize('H,C,p', ATTEND_CASES)
def test_attend_backward_det(H, C, p):
    lib, native = _lib()
    c = ref.attend_case(H, C, p)
    want, bound = ref.attend_bounds(c)
    U, E, HC = c['U'], c['E'], H * C
    d = {n: c[n].to(DEV).contiguous() for n in ('q', 'k', 'v', 'eproj', 'order', 'src', 'seg_lo', 'seg_hi', 'dout')}
    ws = torch.empty(int(lib.tgmx_tconv_attend_backward_det_workspace_bytes(U, E, H)), dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        bufs = dict(dq=Buf(U, HC), dk=Buf(U, HC), dv=Buf(U, HC), de=Buf(E, HC))  # NaN-filled: every element must be written
        native.check(lib.tgmx_tconv_attend_backward_det(d['q'].data_ptr(), d['k'].data_ptr(), d['v'].data_ptr(), d['eproj'].data_ptr(), d['order'].data_ptr(),
                                                        d['src'].data_ptr(), d['seg_lo'].data_ptr(), d['seg_hi'].data_ptr(), U, E, H, C, c['scale'],
                                                        d['dout'].data_ptr(), bufs['dq'].ptr, bufs['dk'].ptr, bufs['dv'].ptr, bufs['de'].ptr,
                                                        native.dropout_desc(p, ref.DROP_SEED, c['stream']), ws.data_ptr(), ws.numel(), native.stream_ptr()),
                     'attend_backward_det')  # fmt: skip
        torch.cuda.synchronize()
        for name, b in bufs.items():
            assert b.sentinels_intact(), f'{name}: a write past its last row'
        outs.append({name: b.view.clone() for name, b in bufs.items()})
    for name in ('dq', 'dk', 'dv', 'de'):
        assert _same_bits(outs[0][name], outs[1][name]), f'two launches differ ({name})'
    none = c['seg_hi'] == c['seg_lo']
    assert torch.equal(outs[0]['dq'].cpu()[none], torch.zeros(int(none.sum()), HC)), 'a target without edges: dq must be exactly 0'
    worst = {name: _report(f'attend_backward_det {(H, C, p)} {name}', outs[0][name], want[name], bound[name]) for name in ('dq', 'dk', 'dv', 'de')}
    assert max(worst.values()) <= 1.0, worst


M_, D_, T_, U_, E_ = 12, 5, 8, 30, 200


@functools.lru_cache(maxsize=None)
def _graph():
    """U = 30, E = 200 in shuffled order: target 0 has no incoming edge, target 1 has 70, source 2 feeds 70 edges."""
    rng = np.random.default_rng(5)
    src = np.concatenate([rng.integers(0, U_, 70), np.full(70, 2), rng.integers(0, U_, 60)])
    tgt = np.concatenate([np.full(70, 1), rng.integers(2, U_, 130)])
    perm = rng.permutation(E_)
    f = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt))
    return dict(edge_index=f(np.stack([src, tgt])[:, perm], np.int64), lu=f(rng.integers(0, 100, U_), np.int64), t=f(rng.integers(0, 130, E_), np.int64),
                msg=f(rng.random((E_, D_)), np.float32), x=f(rng.standard_normal((U_, M_)), np.float32))  # fmt: skip


def _layer(C, p, seed=0):
    from tgm_amd.nn import GraphAttentionEmbedding, Time2Vec

    torch.manual_seed(seed)
    enc = GraphAttentionEmbedding(M_, 2 * C, D_, Time2Vec(T_)).to(DEV).train()
    enc.conv.dropout = p
    with torch.no_grad():  # non-trivial Time2Vec so that its gradient is exercised at these small time deltas
        enc.time_enc.w.weight.copy_(torch.rand(T_, 1) * 0.3)
        enc.time_enc.w.bias.copy_(torch.rand(T_))
    return enc


def _run(enc, G):
    """One forward + backward of sum(z * G): (z, x.grad, {parameter name: grad or None})."""
    g = _graph()
    for q in enc.parameters():
        q.grad = None
    x = g['x'].to(DEV).requires_grad_(True)
    z = enc(x, g['lu'].to(DEV), g['edge_index'].to(DEV), g['t'].to(DEV), g['msg'].to(DEV))
    assert type(z.grad_fn).__name__ == 'TconvLayerFnBackward', 'the one-node path was not taken'
    (z * G.to(DEV)).sum().backward()
    return z.detach(), x.grad, {k: (None if v.grad is None else v.grad.clone()) for k, v in enc.named_parameters()}


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('C', [8, 86, 128])
def test_layer_gradients(C, p, monkeypatch):
    """The upstream gradient is randn / 8.  lin_key.bias has a mathematically zero gradient (the softmax is shift invariant), so what
    float32 leaves there is rounding alone: n 2^-24 sum_j |dk[j, c]| with n the roundings along a dk chain (a source feeding 70 edges: tens).
    The float64 reference puts sum_j |dk[j, c]| at 3.6 to 4.6 times the scale of G at these three widths, and the bar's absolute floor is
    2e-4 * 2e-3 = 6.7 * 2^-24: at unit scale that floor allows 1.5 roundings of the sum (measured there: 1.7 at C = 86, a failure by rounding
    alone), at 1 / 8 it allows 12.  Every other gradient's largest entry stays far above the 2e-3 floor, so its bar is relative as before."""
    from oracle.tgn_ref import graph_attention_embedding_ref

    if C <= 64:
        monkeypatch.setenv('TGMX_TGN_BWD', 'native')
    g, enc = _graph(), _layer(C, p)
    G = torch.randn(U_, 2 * C, generator=torch.Generator().manual_seed(C)) / 8
    z, dx, grads = _run(enc, G)
    ep = {k: v.detach().cpu().double().requires_grad_(True) for k, v in enc.state_dict().items()}
    xr = g['x'].double().requires_grad_(True)
    drop = (p, enc.conv._drop_seed, enc.conv._drop_calls) if p else None
    zr = graph_attention_embedding_ref(ep, xr, g['lu'], g['edge_index'], g['t'], g['msg'].double(), dropout=drop)
    assert zr.dtype == torch.float64
    err = ((z.cpu().double() - zr.detach()).abs() / zr.detach().abs().clamp(min=1)).max().item()
    print(f'[tconv_train] C = {C}, p = {p}: output {err / 1e-5:.4f}x the 1e-5 bar')
    assert err <= 1e-5
    (zr * G.double()).sum().backward()
    worst = {}
    for name, got, r in [('x', dx, xr.grad)] + [(k, grads[k], ep[k].grad) for k in grads]:
        assert got is not None and r is not None, name
        worst[name] = ((got.cpu().double() - r).abs().max() / r.abs().max().clamp(min=2e-3)).item()
        assert name == 'conv.lin_key.bias' or float(r.abs().max()) > 2e-3, f'{name}: the floor took over the bar'
    print(f'[tconv_train] C = {C}, p = {p}: worst gradient {max(worst.values()) / 2e-4:.4f}x the 2e-4 bar ({max(worst, key=worst.get)})')
    assert max(worst.values()) <= 2e-4, worst


def test_same_bits():
    g, enc = _graph(), _layer(86, 0.0)
    G = torch.randn(U_, 172, generator=torch.Generator().manual_seed(1))
    z0, dx0, g0 = _run(enc, G)
    z1, dx1, g1 = _run(enc, G)
    with torch.no_grad():
        z_ng = enc(g['x'].to(DEV), g['lu'].to(DEV), g['edge_index'].to(DEV), g['t'].to(DEV), g['msg'].to(DEV))
    assert _same_bits(z0, z_ng), 'the saving forward and the inference forward differ'
    assert _same_bits(dx0, dx1) and all(_same_bits(g0[k], g1[k]) for k in g0), 'two forward + backward runs differ'


def test_frozen_tails():
    enc = _layer(86, 0.1)
    G = torch.randn(U_, 172, generator=torch.Generator().manual_seed(2))
    _, dx0, g0 = _run(enc, G)
    frozen = [enc.conv.lin_edge.weight, enc.time_enc.w.weight, enc.time_enc.w.bias]
    for q in frozen:
        q.requires_grad_(False)
    enc.conv._drop_calls -= 1  # the same dropout stream as the unfrozen run
    _, dx1, g1 = _run(enc, G)
    assert all(q.grad is None for q in frozen)
    assert _same_bits(dx0, dx1)
    assert all(_same_bits(g0[k], g1[k]) for k in g0 if g1[k] is not None) and sum(v is not None for v in g1.values()) == 8


@pytest.mark.parametrize('H,C', [(2, 260), (4, 130), (8, 65)])
def test_outside_the_envelope(H, C):
    from tgm_amd.nn.tgn import TransformerConv

    lib, _ = _lib()
    assert lib.tgmx_tconv_train_supported(H, C) == 0 and lib.tgmx_tconv_train_supported(2, 256) == 1 and lib.tgmx_tconv_train_supported(8, 64) == 1
    g = _graph()
    conv = TransformerConv(M_, C, heads=H, edge_dim=T_ + D_).to(DEV).train()
    with pytest.raises(NotImplementedError, match='envelope'):
        conv(g['x'].to(DEV).requires_grad_(True), g['edge_index'].to(DEV), torch.randn(E_, T_ + D_, device=DEV))
