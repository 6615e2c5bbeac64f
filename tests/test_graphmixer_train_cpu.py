"""GraphMixer's native training path, the parts that need no GPU: the float64 restatement of the backward (``graphmixer_bwd_restate.py``)
pinned to float64 autograd -- through ``graphmixer_restate``'s forward with no dropout, through the restatement's own masked forward with
it -- the argument block's ctypes mirror, and the envelope and mode decisions case by case."""
import ctypes

import pytest
import torch

import graphmixer_bwd_restate as br
import graphmixer_restate as gr

F64 = torch.float64


def _layer_sd(K, C, ft, fc, g, prefix=''):
    Ht, Hc = int(ft * K), int(fc * C)
    shapes = ((K,), (K,), (Ht, K), (Ht,), (K, Ht), (K,), (C,), (C,), (Hc, C), (Hc,), (C, Hc), (C,))
    return {prefix + n: torch.randn(s, generator=g, dtype=F64) * 0.5 + (1.0 if n.endswith('norm.weight') else 0.0) for n, s in zip(br.LAYER_NAMES, shapes)}


def _close(got, want, tag, mag=None):
    """Within 1e-10 of the gradient's largest entry.  A gradient that is exactly 0 because its terms cancel has no such scale (C = 1: the
    channel LayerNorm's x-hat is 0, float64 autograd leaves ~1e-14 of d channel_norm.weight and of everything below it): where the largest
    entry is below 1e-10 of the restated MAGNITUDE's (the size of the cancelling terms), that magnitude is the scale."""
    scale = want.abs().max().item() if want.numel() else 0.0
    if mag is not None and mag.numel() and scale <= 1e-10 * mag.max().item():
        scale = mag.max().item()
    err = (got - want).abs().max().item() if want.numel() else 0.0
    assert err <= 1e-10 * max(scale, 1e-300), (tag, err, scale)


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'dropout'])
@pytest.mark.parametrize('C', [1, 13])
@pytest.mark.parametrize('K', [1, 2, 5])
def test_mixer_backward_matches_float64_autograd(K, C, masked):
    g = torch.Generator().manual_seed(100 * K + C)
    S, ft, fc = 4, (0.5 if K < 5 else 1.3), 2.1  # (K = 1: Ht = 0)
    sd = _layer_sd(K, C, ft, fc, g)
    Ht, Hc = int(ft * K), int(fc * C)
    P = [sd[n].clone().requires_grad_(True) for n in br.LAYER_NAMES]
    x = torch.randn(S, K, C, generator=g, dtype=F64).requires_grad_(True)
    w = torch.randn(S, K, C, generator=g, dtype=F64)
    masks = br.layer_masks(0.5, 11, 64, 0, S, K, C, Ht, Hc) if masked else br.unit_masks(S, K, C, Ht, Hc)
    keep = {}
    out = br.mixer_forward(P, x, masks, keep=keep)
    if not masked:  # with unit masks the forward is graphmixer_restate's
        _close(out.detach(), gr.mixer_forward(sd, '', x.detach()), 'forward')
    (out * w).sum().backward()
    got = br.mixer_backward([p.detach() for p in P], x.detach(), keep['z1'], w, masks)
    _close(got['dx'], x.grad, 'dx', got['dx_m'])
    for n, p in zip(br.LAYER_NAMES, P):
        _close(got[n], p.grad if p.grad is not None else torch.zeros_like(p), n, got[n + '_m'])
        assert (got[n + '_m'] >= got[n].abs() * (1 - 1e-12)).all(), n  # a magnitude bounds its value


def _encoder_case(K, D, L, seed, all_pad=True):
    g = torch.Generator().manual_seed(seed)
    S, T, F_, E, N = 6, 3, 2, 4, 9
    ft, fc = (0.5 if K < 5 else 1.3), 2.1
    sd = {'time_encoder.w.weight': torch.randn(T, 1, generator=g, dtype=F64), 'time_encoder.w.bias': torch.randn(T, generator=g, dtype=F64),
          'projection_layer.weight': torch.randn(D, D + T, generator=g, dtype=F64) * 0.5, 'projection_layer.bias': torch.randn(D, generator=g, dtype=F64),
          'output_layer.weight': torch.randn(E, D + F_, generator=g, dtype=F64) * 0.5, 'output_layer.bias': torch.randn(E, generator=g, dtype=F64)}  # fmt: skip
    for l in range(L):
        sd.update(_layer_sd(K, D, ft, fc, g, f'mlp_mixers.{l}.'))
    nids = torch.randint(0, N, (S, K), generator=g)
    nids[torch.rand(S, K, generator=g) < 0.3] = -1
    if all_pad:
        nids[2] = -1
    nids[3] = 5  # and one seed with every slot valid
    args = dict(nbr_edge_x=torch.randn(S, K, D, generator=g, dtype=F64), seed_times=torch.randint(50, 99, (S,), generator=g),
                nbr_edge_time=torch.randint(0, 50, (S, K), generator=g), nbr_nids=nids, seeds=torch.randint(0, N, (S,), generator=g),
                tg_lists=[[1, 2], [], [3], [4, 4, 0], [], [8]], node_feat=torch.randn(N, F_, generator=g, dtype=F64))  # fmt: skip
    return sd, args, (int(ft * K), int(fc * D)), torch.randn(S, E, generator=g, dtype=F64)


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'dropout'])
@pytest.mark.parametrize('L', [0, 1, 3])
@pytest.mark.parametrize('K,D', [(1, 13), (2, 1), (5, 13)])
def test_encoder_backward_matches_float64_autograd(K, D, L, masked):
    sd, args, (Ht, Hc), w = _encoder_case(K, D, L, 7 * K + D + L)
    assert (args['nbr_nids'][2] == -1).all() and (args['nbr_nids'][3] != -1).all()
    S = args['nbr_nids'].shape[0]
    masks = [br.layer_masks(0.1, 5, 128, l, S, K, D, Ht, Hc) for l in range(L)] if masked else None
    leaf = {k: v.clone().requires_grad_(not k.startswith('time_encoder')) for k, v in sd.items()}
    if masked:
        out = br.encoder_forward(leaf, L, masks=masks, **args)
    else:  # the checker's own forward; the restatement's saves what the backward needs and must agree with it
        out = gr.encoder_forward(leaf, L, args['nbr_edge_x'], args['seed_times'], args['nbr_edge_time'], args['nbr_nids'], args['seeds'], args['tg_lists'],
                                 args['node_feat'])  # fmt: skip
    (out * w).sum().backward()
    keep = {}
    again = br.encoder_forward(sd, L, masks=masks, keep=keep, **args)
    _close(again, out.detach(), 'forward')
    got = br.encoder_backward(sd, L, keep, w, masks)
    names = [k for k in sd if not k.startswith('time_encoder')]
    assert sorted(got) == sorted(names)
    for n in names:
        grad = leaf[n].grad if leaf[n].grad is not None else torch.zeros_like(leaf[n])
        _close(got[n][0], grad, n, got[n][1])
        assert (got[n][1] >= got[n][0].abs() * (1 - 1e-12)).all(), n


def test_tail_backward_restated():
    nids = torch.tensor([[-1, -1, -1], [4, -1, 2], [1, 2, 3]])
    dcat = torch.tensor([[1.0, 2.0], [3.0, 4.0], [6.0, 9.0]], dtype=F64)
    dz = br.tail_backward(dcat, nids, 3).view(3, 3, 2)
    assert not dz[0].any() and torch.equal(dz[1], torch.tensor([[1.5, 2.0], [0.0, 0.0], [1.5, 2.0]], dtype=F64))
    assert torch.equal(dz[2], torch.tensor([[2.0, 3.0]] * 3, dtype=F64))


def test_argument_block_mirror_and_abi_version():
    from tgm_amd import _native

    lib = _native.load()
    assert lib.tgmx_abi_sizeof(36) == ctypes.sizeof(_native.GraphMixerBwd) > ctypes.sizeof(_native.MixerLayerGrad) * _native.MIXER_MAX_LAYERS
    assert lib.tgmx_version() == 7
    assert lib.tgmx_abi_sizeof(14) == ctypes.sizeof(_native.GraphMixerFwd) and lib.tgmx_abi_sizeof(13) == ctypes.sizeof(_native.MixerLayer)


def test_lds_envelope_function():
    """One function for both token kernels: the forward's 4 (K C + (K + Ht) 128) bytes and the backward's 4 (4 K + 2 Ht) 33 at its narrowest
    pass of 32 channels, 64 KiB each."""
    from tgm_amd.nn._graphmixer_train import train_supported

    fits = lambda K, C, Ht: 4 * (K * C + (K + Ht) * 128) <= 65536 and 4 * (4 * K + 2 * Ht) * 33 <= 65536
    for K, C, Ht in [(20, 172, 10), (20, 627, 10), (20, 628, 10), (64, 172, 32), (20, 172, 26), (100, 8, 20), (124, 8, 0), (125, 8, 0), (110, 8, 28), (110, 8, 29), (1, 1, 0),
                     (5, 13, 6), (30, 200, 15)]:  # fmt: skip
        assert train_supported(K, C, Ht) == fits(K, C, Ht), (K, C, Ht)
    assert train_supported(20, 172, 10) and not train_supported(64, 172, 32) and not train_supported(20, 628, 10)
    assert not train_supported(0, 4, 0) and not train_supported(4, 0, 0) and not train_supported(4, 4, -1)


def test_mode(monkeypatch):
    from tgm_amd.nn import _graphmixer_train as gt

    assert gt.DEFAULT in ('native', 'torch')
    for value, want in ((None, gt.DEFAULT), ('', gt.DEFAULT), ('py', 'py'), ('torch', 'torch'), ('native', 'native'), ('PY', gt.DEFAULT), ('1', gt.DEFAULT)):
        if value is None:
            monkeypatch.delenv('TGMX_GRAPHMIXER_BWD', raising=False)
        else:
            monkeypatch.setenv('TGMX_GRAPHMIXER_BWD', value)
        assert gt.mode() == want == br.parse_mode(value, gt.DEFAULT), value


def test_in_envelope_case_by_case(monkeypatch):
    """The decision reads shapes, dtypes, devices and flags only, so host tensors can stand in (``forward`` itself refuses them)."""
    from tgm_amd.nn import GraphMixerEncoder, MLPMixer
    from tgm_amd.nn import _graphmixer_train as gt

    monkeypatch.setenv('TGMX_GRAPHMIXER_BWD', 'native')
    dims = dict(time_dim=4, embed_dim=3, num_tokens=5, node_dim=2, edge_dim=6)
    enc = GraphMixerEncoder(**dims)
    x, ex = torch.randn(9, 2), torch.randn(6, 5, 6)
    assert gt.in_envelope(enc, x, ex, 6)
    assert not gt.in_envelope(enc, x, ex, 0)  # no seed
    assert not gt.in_envelope(enc, x.clone().requires_grad_(True), ex, 6) and not gt.in_envelope(enc, x, ex.clone().requires_grad_(True), 6)
    assert not gt.in_envelope(enc, x.double(), ex, 6) and not gt.in_envelope(enc, x, ex.double(), 6) and not gt.in_envelope(enc, x, ex.half(), 6)
    with torch.no_grad():
        assert not gt.in_envelope(enc, x, ex, 6)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        assert not gt.in_envelope(enc, x, ex, 6)
    monkeypatch.setenv('TGMX_GRAPHMIXER_BWD', 'torch')
    assert not gt.in_envelope(enc, x, ex, 6)
    monkeypatch.setenv('TGMX_GRAPHMIXER_BWD', 'py')
    assert gt.in_envelope(enc, x, ex, 6)
    monkeypatch.setenv('TGMX_GRAPHMIXER_BWD', 'native')
    enc.time_encoder.w.weight.requires_grad_(True)  # an unfrozen time encoder
    assert not gt.in_envelope(enc, x, ex, 6)
    enc.time_encoder.w.weight.requires_grad_(False)
    assert gt.in_envelope(enc, x, ex, 6)
    for p in enc.parameters():
        p.requires_grad_(False)
    assert not gt.in_envelope(enc, x, ex, 6)  # nothing to train
    enc.output_layer.bias.requires_grad_(True)
    assert gt.in_envelope(enc, x, ex, 6)
    enc.mlp_mixers[1].channel_norm.eps = 1e-6  # _check_native() refuses
    assert not gt.in_envelope(enc, x, ex, 6)
    enc.mlp_mixers[1].channel_norm.eps = 1e-5
    enc.mlp_mixers[0].channel_feedforward.ffn[2].p = 0.3  # a site with its own p
    assert not gt.in_envelope(enc, x, ex, 6)
    enc.mlp_mixers[0].channel_feedforward.ffn[2].p = enc.dropout
    assert gt.in_envelope(enc, x, ex, 6)
    assert gt.in_envelope(enc.double().float(), x, ex, 6) and not gt.in_envelope(GraphMixerEncoder(**dims).double(), x, ex, 6)
    wide = GraphMixerEncoder(**{**dims, 'num_tokens': 64, 'edge_dim': 172})  # outside the token kernels' LDS
    assert not gt.in_envelope(wide, x, torch.randn(6, 64, 172), 6)
    assert gt.in_envelope(GraphMixerEncoder(**dims, num_layers=0), x, ex, 6)
    # MLPMixer alone: its input may ask for a gradient
    m = MLPMixer(5, 6, dropout=0.2)
    xm = torch.randn(3, 5, 6)
    assert gt.mixer_in_envelope(m, xm) and gt.mixer_in_envelope(m, xm.clone().requires_grad_(True))
    assert not gt.mixer_in_envelope(m, xm[:0]) and not gt.mixer_in_envelope(m, xm.double()) and not gt.mixer_in_envelope(MLPMixer(64, 172), torch.randn(2, 64, 172))
    with torch.no_grad():
        assert not gt.mixer_in_envelope(m, xm)


def test_next_drop_streams():
    from tgm_amd.nn import MLPMixer
    from tgm_amd.nn import _graphmixer_train as gt

    m = MLPMixer(5, 6, dropout=0.2).train()
    a, b = gt.next_drop(m, m.dropout), gt.next_drop(m, m.dropout)
    assert a[0] == b[0] == pytest.approx(0.2) and a[1] == b[1] == torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
    assert b[2] - a[2] == 64 and a[2] % 64 == 0 and a[2] > 0  # one block of 64 streams per forward call: 4 sites x up to 8 layers fit
    assert gt.next_drop(m.eval(), m.dropout) == (0.0, 0, 0) and gt.next_drop(m.train(), 0.0) == (0.0, 0, 0)
