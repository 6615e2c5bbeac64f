"""TPNet's native training path, the parts that need no GPU: the float64 restatement of the backward (``tpnet_bwd_restate.py``) pinned to
float64 autograd -- through ``tpnet_restate.tpnet_forward`` with no dropout, through the restatement's own masked forward with it -- the
partial row against the six gradients, the argument block's ctypes mirror, and the envelope and mode decisions case by case."""
import ctypes

import pytest
import torch

import tpnet_bwd_restate as br
import tpnet_restate as tr

F64 = torch.float64


def _case(k, E, L, rp_cfg, seed, dN=3, dT=2, dE=4):
    """A small TPNet as a float64 state_dict plus host inputs: sequence 1 all pads, a zero time gap, pads elsewhere."""
    g = torch.Generator().manual_seed(seed)
    B, N = 3, 11
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    od, sd = 0, {}
    if rp_cfg is not None:
        nl, dim = rp_cfg['num_layer'], 5
        NR = 2 * (nl + 1) if rp_cfg['concat'] else nl + 1
        od = NR * NR
        for i in range(nl + 1):
            sd[f'random_projections.random_projections.{i}'] = r(N, dim) * 0.6
        sd.update({'random_projections.mlp.0.weight': r(4 * od, od) * 0.3, 'random_projections.mlp.0.bias': r(4 * od) * 0.3,
                   'random_projections.mlp.2.weight': r(od, 4 * od) * 0.3, 'random_projections.mlp.2.bias': r(od) * 0.3})  # fmt: skip
    W = dN + dT + dE + 2 * od
    sd.update({'time_encoder.w.weight': r(dT, 1), 'time_encoder.w.bias': r(dT), 'projection_layer.0.weight': r(2 * E, W) * 0.4,
               'projection_layer.0.bias': r(2 * E) * 0.4, 'projection_layer.2.weight': r(E, 2 * E) * 0.4, 'projection_layer.2.bias': r(E) * 0.4})  # fmt: skip
    Ht, Hc = k // 2, 4 * E
    shapes = ((k,), (k,), (Ht, k), (Ht,), (k, Ht), (k,), (E,), (E,), (Hc, E), (Hc,), (E, Hc), (E,))
    for l in range(L):
        for n, s in zip(br.LAYER_NAMES, shapes):
            sd[f'mlp_mixers.{l}.{n}'] = r(*s) * 0.5 + (1.0 if n.endswith('norm.weight') else 0.0)
    nids = torch.randint(0, N, (2 * B, k), generator=g)
    nids[torch.rand(2 * B, k, generator=g) < 0.3] = -1
    nids[1] = -1
    t = torch.randint(60, 99, (B,), generator=g)
    nt = torch.randint(0, 60, (2 * B, k), generator=g)
    nt[0, 0] = t[0]  # a zero gap: lg = 0
    nids[0, 0] = 2
    args = dict(node_x=r(N, dN), src=torch.randint(0, N, (B,), generator=g), dst=torch.randint(0, N, (B,), generator=g), edge_time=t, nbr_nids=nids,
                nbr_time=nt, nbr_edge_x=r(2 * B, k, dE))  # fmt: skip
    return sd, args, dict(dN=dN, dT=dT, dE=dE, od=od), (Ht, Hc), r(2 * B, E)


def _close(got, want, tag):
    scale = max(want.abs().max().item(), 1e-300) if want.numel() else 1.0
    err = (got - want).abs().max().item() if want.numel() else 0.0
    assert err <= 1e-10 * scale, (tag, err, scale)


RP = {'none': None, 'concat': dict(num_layer=1, concat=True, scale=True), 'cross': dict(num_layer=2, concat=False, scale=True)}


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'dropout'])
@pytest.mark.parametrize('rp', ['none', 'concat', 'cross'])
@pytest.mark.parametrize('k,E,L', [(1, 5, 1), (2, 2, 2), (5, 6, 0), (5, 6, 3)])
def test_chain_matches_float64_autograd(k, E, L, rp, masked):
    """(E = 1 is left to ``test_graphmixer_train_cpu``'s block test: the channel LayerNorm of one channel cancels exactly, and a gradient that
    is all cancellation needs the block's magnitudes for its scale, which the chain here does not carry.)"""
    sd, args, dims, (Ht, Hc), w = _case(k, E, L, RP[rp], 31 * k + E + L)
    Q = args['nbr_nids'].shape[0]
    masks = [br.layer_masks(0.3, 5, 128, l, Q, k, E, Ht, Hc) for l in range(L)] if masked else None
    trainable = lambda n: n.split('.')[-1] in ('weight', 'bias')  # (the tables are frozen buffers)
    leaf = {n: v.clone().requires_grad_(trainable(n)) for n, v in sd.items()}
    pos = (args['node_x'], args['src'], args['dst'], args['edge_time'], args['nbr_nids'], args['nbr_time'], args['nbr_edge_x'])
    if masked:
        zs, zd = br.forward(leaf, L, RP[rp], *pos, masks=masks)
    else:  # the checker's own forward; the restatement's saves what the backward needs and must agree with it
        zs, zd = tr.tpnet_forward(leaf, L, RP[rp], *pos)
    (torch.cat([zs, zd]) * w).sum().backward()
    keep = {}
    again = br.forward(sd, L, RP[rp], *pos, masks=masks, keep=keep)
    _close(torch.cat(again), torch.cat([zs, zd]).detach(), 'forward')
    assert keep['pad'][1].all() and keep['lg'][0, 0] == 0
    got = br.backward(sd, L, dims, keep, w, masks)
    names = [n for n in sd if trainable(n)]
    assert sorted(got) == sorted(names)
    for n in names:
        _close(got[n], leaf[n].grad if leaf[n].grad is not None else torch.zeros_like(leaf[n]), n)


@pytest.mark.parametrize('K,C,Q', [(1, 3, 2), (2, 1, 1), (7, 5, 3)])
def test_partial_rows_sum_to_the_six_gradients(K, C, Q):
    g = torch.Generator().manual_seed(K + C)
    Ht = K // 2
    shapes = ((K,), (K,), (Ht, K), (Ht,), (K, Ht), (K,))
    P = [torch.randn(s, generator=g, dtype=F64) for s in shapes]
    x, d = torch.randn(Q, K, C, generator=g, dtype=F64), torch.randn(Q, K, C, generator=g, dtype=F64)
    m0, m1 = br.layer_masks(0.5, 3, 64, 0, Q, K, C, Ht, 1)[:2]
    r = br.partial_rows(P, x, d, m0, m1)
    assert r['part'].shape == (Q, br.part_floats(K, Ht)) and (r['part_m'] >= r['part'].abs() * (1 - 1e-12)).all()
    grads = br.part_to_grads(r['part'].sum(0), K, Ht)
    assert sorted(grads) == sorted(br.LAYER_NAMES[:6])
    for n in br.LAYER_NAMES[:6]:
        _close(grads[n], r[n], n)
    mags = br.part_to_grads(r['part_m'].sum(0), K, Ht)
    for n in br.LAYER_NAMES[:6]:
        _close(mags[n], r[n + '_m'], n + '_m')


def test_time_rows_and_mean_backward_restated():
    lg = torch.tensor([0.0, 1.5, 2.0], dtype=F64)
    pad = torch.tensor([False, False, True])
    tw, tb = torch.tensor([0.5, 2.0], dtype=F64), torch.tensor([0.1, -0.3], dtype=F64)
    d = torch.tensor([[1.0, 2.0], [3.0, -1.0], [5.0, 5.0]], dtype=F64)
    r = br.time_rows(d, lg, pad, tw, tb)['rows']
    assert not r[2].any() and not r[0, :2].any()  # the pad row; the zero gap has no weight gradient
    want = -torch.sin(1.5 * tw + tb) * d[1]
    assert torch.allclose(r[1, 2:], want, rtol=0, atol=1e-15) and torch.allclose(r[1, :2], want * 1.5, rtol=0, atol=1e-15)
    dz = br.mean_backward(torch.tensor([[2.0, 4.0], [6.0, 8.0]], dtype=F64), 2)
    assert torch.equal(dz, torch.tensor([[1.0, 2.0], [1.0, 2.0], [3.0, 4.0], [3.0, 4.0]], dtype=F64))


def test_argument_block_mirror_and_abi_version():
    from tgm_amd import _native

    lib = _native.load()
    assert lib.tgmx_abi_sizeof(38) == ctypes.sizeof(_native.TPNetBwd) > 0
    assert lib.tgmx_abi_sizeof(18) == ctypes.sizeof(_native.TPNetFwd) == 1248  # tgmx_tpnet_fwd_t: byte for byte as it was
    assert lib.tgmx_version() == 7
    for name in ('tgmx_tpnet_forward_train', 'tgmx_tpnet_backward', 'tgmx_tpnet_backward_workspace_bytes', 'tgmx_tpnet_token_backward',
                 'tgmx_tpnet_token_mix_train', 'tgmx_tpnet_time_backward', 'tgmx_tpnet_mean_backward', 'tgmx_tpnet_train_supported'):  # fmt: skip
        assert name in _native.SIGNATURES and hasattr(lib, name)


def test_envelope_function():
    """One function for the token forward and the token backward: the forward's LDS, the backward's at its chunk width, and the partial row
    of 2 K Ht + 3 K + Ht floats within 24 registers a thread of that chunk."""
    from tgm_amd.nn._tpnet_train import part_floats, train_supported

    def fits(K, C, Ht):
        if 4 * (K * C + (K + Ht) * 128) > 65536:
            return False
        threads = next((t for t in (128, 64, 32) if 4 * (4 * K + 2 * Ht) * (t + 1) <= 65536), 0)
        return threads > 0 and part_floats(K, Ht) <= 24 * threads

    for K, C, Ht in [(32, 172, 16), (32, 172, 15), (1, 1, 0), (7, 65, 3), (20, 172, 10), (40, 172, 20), (36, 100, 18), (32, 400, 16), (64, 8, 32), (20, 172, 26),
                     (124, 8, 0), (125, 8, 0)]:  # fmt: skip
        assert train_supported(K, C, Ht) == fits(K, C, Ht), (K, C, Ht)
    assert train_supported(32, 172, 16) and not train_supported(40, 172, 20) and not train_supported(32, 400, 16)
    assert not train_supported(0, 4, 0) and not train_supported(4, 0, 0) and not train_supported(4, 4, -1)
    assert part_floats(32, 16) == 1136 == br.part_floats(32, 16)


def test_mode(monkeypatch):
    from tgm_amd.nn import _tpnet_train as tt

    assert tt.DEFAULT in ('native', 'torch')
    for value, want in ((None, tt.DEFAULT), ('', tt.DEFAULT), ('py', 'py'), ('torch', 'torch'), ('native', 'native'), ('PY', tt.DEFAULT), ('1', tt.DEFAULT)):
        if value is None:
            monkeypatch.delenv('TGMX_TPNET_BWD', raising=False)
        else:
            monkeypatch.setenv('TGMX_TPNET_BWD', value)
        assert tt.mode() == want == br.parse_mode(value, tt.DEFAULT), value


def test_in_envelope_case_by_case(monkeypatch):
    """The decision reads shapes, dtypes, devices and flags only, so host tensors can stand in (``forward`` itself refuses them)."""
    from tgm_amd.nn import RandomProjectionModule, TPNet
    from tgm_amd.nn import _tpnet_train as tt

    monkeypatch.setenv('TGMX_TPNET_BWD', 'native')
    make = lambda levels=2, **kw: TPNet(**{**dict(node_feat_dim=3, edge_x_dim=4, time_feat_dim=2, output_dim=6, num_neighbors=5), **kw},
                                        random_projections=None if levels is None else RandomProjectionModule(9, levels, 1e-5, 0, use_matrix=False, enforce_dim=4))
    call = lambda B=2: dict(node_x=torch.randn(9, 3), nbr_x=torch.randn(2 * B, 5, 4), B=B)
    m = make()
    assert tt.in_envelope(m, call())
    assert not tt.in_envelope(m, call(0))  # no pair
    for key in ('node_x', 'nbr_x'):
        a = call()
        a[key] = a[key].requires_grad_(True)
        assert not tt.in_envelope(m, a)
    with torch.no_grad():
        assert not tt.in_envelope(m, call())
    with torch.autocast('cpu', dtype=torch.bfloat16):
        assert not tt.in_envelope(m, call())
    monkeypatch.setenv('TGMX_TPNET_BWD', 'torch')
    assert not tt.in_envelope(m, call())
    monkeypatch.setenv('TGMX_TPNET_BWD', 'py')
    assert tt.in_envelope(m, call())
    monkeypatch.setenv('TGMX_TPNET_BWD', 'native')
    for p in m.parameters():
        p.requires_grad_(False)
    assert not tt.in_envelope(m, call())  # nothing to train
    m.time_encoder.w.bias.requires_grad_(True)  # the time encoder is trainable here
    assert tt.in_envelope(m, call())
    m.mlp_mixers[1].channel_norm.eps = 1e-6  # _check_native() refuses
    assert not tt.in_envelope(m, call())
    m.mlp_mixers[1].channel_norm.eps = 1e-5
    m.mlp_mixers[0].token_feedforward.ffn[4].p = 0.3  # a site with its own p
    assert not tt.in_envelope(m, call())
    m.mlp_mixers[0].token_feedforward.ffn[4].p = m.dropout
    assert tt.in_envelope(m, call())
    assert not tt.in_envelope(make().double(), call())
    assert tt.in_envelope(make(None), call()) and tt.in_envelope(make(3), call()) and not tt.in_envelope(make(4), call())  # at most 4 tables
    assert tt.in_envelope(make(num_layers=0), call()) and tt.in_envelope(make(num_layers=8), call()) and not tt.in_envelope(make(num_layers=9), call())
    wide = make(num_neighbors=40, output_dim=172)  # outside the token kernels' envelope
    assert not tt.in_envelope(wide, dict(node_x=torch.randn(9, 3), nbr_x=torch.randn(4, 40, 4), B=2))

    class OtherTime(torch.nn.Module):
        def __init__(self, dim):
            super().__init__()
            self.lin = torch.nn.Linear(1, dim)

    assert not tt.in_envelope(make(time_encoder=OtherTime), call())
