"""DyGFormer's native training path, the parts that need no GPU: the float64 restatement of the backward (``dygformer_bwd_restate.py``)
pinned to float64 autograd -- through ``dygformer_restate``'s forward with no dropout, through the restatement's own masked forward with
it -- the argument block's ctypes mirror, the attention backward's envelope and the mode decision."""
import ctypes

import pytest
import torch

import dygformer_bwd_restate as br
import dygformer_restate as dr

F64 = torch.float64


def small_case(seed=3, P=3, L=4, patch=2, C=3, H=2, dN=2, dE=3, dT=2, E=4, layers=2, N=6):
    g = torch.Generator().manual_seed(seed)
    D = 4 * C
    shapes = {'time_encoder.w.weight': [dT, 1], 'time_encoder.w.bias': [dT], br.CO + '0.weight': [C, 1], br.CO + '0.bias': [C], br.CO + '2.weight': [C, C],
              br.CO + '2.bias': [C]}  # fmt: skip
    for n, d in zip(br.CHANNELS, (dN, dE, dT, C)):
        shapes[f'projection_layer.{n}.weight'], shapes[f'projection_layer.{n}.bias'] = [C, patch * d], [C]
    lshapes = ([D], [D], [3 * D, D], [3 * D], [D, D], [D], [D], [D], [4 * D, D], [4 * D], [D, 4 * D], [D])
    for l in range(layers):
        shapes.update({f'transformers.{l}.{n}': s for n, s in zip(br.LAYER_NAMES, lshapes)})
    shapes['output_layer.weight'], shapes['output_layer.bias'] = [E, D], [E]
    sd = {n: torch.randn(s, generator=g, dtype=F64) * 0.5 + (1.0 if 'norm_layers' in n and n.endswith('weight') else 0.0) for n, s in shapes.items()}
    k = L - 1
    nids = torch.randint(0, N, (2 * P, k), generator=g)
    nids[torch.rand(2 * P, k, generator=g) < 0.3] = -1
    nids[1] = -1  # one sequence all pads
    src, dst = torch.randint(0, N, (P,), generator=g), torch.randint(0, N, (P,), generator=g)
    dst[0] = src[0]
    inputs = dict(node_x=torch.randn(N, dN, generator=g, dtype=F64), src=src, dst=dst, edge_time=torch.randint(50, 60, (P,), generator=g),
                  nbr_nids=nids, nbr_time=torch.randint(0, 50, (2 * P, k), generator=g), nbr_edge_x=torch.randn(2 * P, k, dE, generator=g, dtype=F64))  # fmt: skip
    return sd, inputs, dict(patch=patch, layers=layers, H=H, P=P, T=2 * (L // patch), D=D, E=E)


def _close(got, want, tag):
    scale = want.abs().max().item() if want.numel() else 0.0
    err = (got - want).abs().max().item() if want.numel() else 0.0
    assert err <= 1e-10 * max(scale, 1e-300), (tag, err, scale)


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'dropout'])
def test_encoder_backward_matches_float64_autograd(masked):
    sd, i, m = small_case()
    args = (i['node_x'], i['src'], i['dst'], i['edge_time'], i['nbr_nids'], i['nbr_time'], i['nbr_edge_x'])
    masks = br.site_masks(0.5, 7, 64, m['layers'], m['P'], m['H'], m['T'], m['D']) if masked else None
    P = {n: v.clone().requires_grad_(True) for n, v in sd.items()}
    if masked:
        zs, zd = br.encoder_forward(P, m['patch'], m['layers'], m['H'], *args, masks=masks)
    else:  # with no masks the forward differentiated is dygformer_restate's, and the restatement's own equals it
        zs, zd = dr.dygformer_forward(P, m['patch'], m['layers'], m['H'], *args)
        es, ed = br.encoder_forward(sd, m['patch'], m['layers'], m['H'], *args)
        _close(es, zs.detach(), 'forward src')
        _close(ed, zd.detach(), 'forward dst')
    g = torch.Generator().manual_seed(1)
    ws, wd = torch.randn(zs.shape, generator=g, dtype=F64), torch.randn(zd.shape, generator=g, dtype=F64)
    ((zs * ws).sum() + (zd * wd).sum()).backward()
    got = br.encoder_backward(sd, m['patch'], m['layers'], m['H'], *args, ws, wd, masks=masks)
    assert set(got) == set(sd) and len(got) == 2 + 4 + 8 + 2 + 12 * m['layers']
    for n, p in P.items():
        assert p.grad is not None and p.grad.abs().max() > 0, n
        _close(got[n], p.grad, n)


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'dropout'])
@pytest.mark.parametrize('B,T,d,H', [(1, 1, 4, 1), (2, 5, 6, 2), (3, 17, 12, 3)])
def test_layer_backward_matches_float64_autograd(B, T, d, H, masked):
    g = torch.Generator().manual_seed(10 * T + d)
    shapes = ([d], [d], [3 * d, d], [3 * d], [d, d], [d], [d], [d], [4 * d, d], [4 * d], [d, 4 * d], [d])
    w = {n: (torch.randn(s, generator=g, dtype=F64) * 0.5 + (1.0 if n.endswith('.weight') and 'norm' in n else 0.0)).requires_grad_(True)
         for n, s in zip(br.LAYER_NAMES, shapes)}  # fmt: skip
    x = torch.randn(B, T, d, generator=g, dtype=F64).requires_grad_(True)
    up = torch.randn(B, T, d, generator=g, dtype=F64)
    masks = br.site_masks(0.5, 3, 128, 1, B, H, T, d)[0] if masked else None
    out = br.layer_forward(w, x, H, masks)
    if not masked:
        _close(out.detach(), dr.transformer_layer({n: v.detach() for n, v in w.items()}, '', x.detach(), H), 'forward')
    (out * up).sum().backward()
    dx, got = br.layer_backward({n: v.detach() for n, v in w.items()}, x.detach(), up, H, masks)
    _close(dx, x.grad, 'dx')
    for n in br.LAYER_NAMES:
        if T == 1 and n in br.LAYER_NAMES[2:4]:  # one token: the softmax is constant, nothing reaches q and k -- compare against the scale of dv
            assert (got[n] - w[n].grad).abs().max() <= 1e-10 * max(1.0, w[n].grad.abs().max().item()), n
        else:
            _close(got[n], w[n].grad, n)


def test_attention_backward_drops_what_the_mask_drops():
    g = torch.Generator().manual_seed(5)
    B, T, H, dh = 2, 5, 2, 3
    qkv = torch.randn(B, T, 3 * H * dh, generator=g, dtype=F64)
    mask = br.site_masks(0.5, 9, 0, 1, B, H, T, H * dh)[0][0]
    datt = torch.zeros(B, T, H * dh, dtype=F64)
    datt[0, 2, 1] = 1.0  # one-hot: group 0, row 2, head 0
    dv = br.attention_backward(qkv, datt, H, mask)[..., 2 * H * dh :]
    dropped = mask[0, 0, 2] == 0
    assert dropped.any() and (~dropped).any()
    assert (dv[0, dropped][:, 1] == 0).all() and (dv[0, ~dropped][:, 1] != 0).all()
    assert (dv[1] == 0).all() and (dv[0][:, dh:] == 0).all()


def test_abi_and_envelope():
    from tgm_amd import _native

    lib = _native.load()
    assert lib.tgmx_version() == 7
    assert lib.tgmx_abi_sizeof(37) == ctypes.sizeof(_native.DyGFormerBwd) > 0
    assert lib.tgmx_abi_sizeof(16) == ctypes.sizeof(_native.DyGFormerFwd)
    assert lib.tgmx_abi_sizeof(36) == ctypes.sizeof(_native.GraphMixerBwd)
    from tgm_amd.nn import _dygformer_train as tr

    for T, dh in ((64, 100), (1, 1), (64, 1), (2, 100)):
        assert tr.train_supported(T, dh), (T, dh)
    for T, dh in ((129, 4), (4, 129), (0, 4), (4, 0), (64, 128), (128, 32)):
        assert not tr.train_supported(T, dh), (T, dh)


def test_abi_sizeof_16_is_unchanged():
    from tgm_amd import _native

    # tgmx_dygformer_fwd_t as the parent commit laid it out: 2 + 4 + 4 + 2 pointers / int64, 10 int32, 6 + 8 + 2 pointers, 8 layers of 12,
    # table + ch[4] + ldch[4], 7 scratch pointers, 3 leading dimensions, out
    assert _native.load().tgmx_abi_sizeof(16) == 8 * (2 + 4 + 4 + 2) + 4 * 10 + 8 * (6 + 8 + 2) + 8 * 12 * 8 + 8 * 9 + 8 * 7 + 8 * 3 + 8 == 1192


def test_mode_parsing(monkeypatch):
    from tgm_amd.nn import _dygformer_train as tr

    monkeypatch.delenv('TGMX_DYGFORMER_BWD', raising=False)
    assert tr.mode() == tr.DEFAULT and tr.DEFAULT in ('native', 'torch')
    for v in ('native', 'py', 'torch'):
        monkeypatch.setenv('TGMX_DYGFORMER_BWD', v)
        assert tr.mode() == v
    for v in ('', 'Native', 'hip', '1'):
        monkeypatch.setenv('TGMX_DYGFORMER_BWD', v)
        assert tr.mode() == tr.DEFAULT


def test_cpu_tensors_keep_their_behaviour():
    """Nothing about the training path changes what a CPU call does: it raises as before."""
    from tgm_amd import _native
    from tgm_amd.nn import TransformerEncoder

    m = TransformerEncoder(8, 2, dropout=0.0)
    with pytest.raises(_native.NativeLibraryError):
        m(torch.randn(2, 3, 8))
