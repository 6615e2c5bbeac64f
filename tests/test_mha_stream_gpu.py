"""Attention past 128 tokens (csrc/mha_stream.hip) against float64: the forward and backward kernels through ctypes at the block edges
(64 keys a block forward, 64 own / 32 streamed rows backward), the running-maximum rescale, and the modules that route to them under
``TGMX_DYGFORMER_LONG=native``.  Bars: forward 1e-5 of max(1, |ref|), gradients 1e-4 of each gradient's largest entry; every case also
holds the float32 restatement of the same inputs to half the bar, so the room is the inputs', not the kernel's.
"""
import math

import pytest
import torch

import dygformer_bwd_restate as br
import dygformer_restate as dr
from test_dygformer_gpu import cpu_restated, gathered, pair_rows, wiki_batches
from test_dygformer_train_gpu import DEV, desc, layer_module, layer_reference, lib, stream, up4

pytestmark = pytest.mark.gpu
FWD_BAR, GRAD_BAR = 1e-5, 1e-4


@pytest.fixture(autouse=True)
def long_route(monkeypatch):
    monkeypatch.setenv('TGMX_DYGFORMER_LONG', 'native')


def padded(t, ld, rows=0):
    """[n, c] -> [n + rows, ld] on the device, NaN outside the data"""
    out = torch.full((t.shape[0] + rows, ld), float('nan'))
    out[: t.shape[0], : t.shape[1]] = t
    return out.to(DEV)


def forward(qkv, B, T, H, dh, drop=None, want_lse=True):
    """qkv [B, T, 3 d] on the host -> (rc, out [B T + 2, ldo] and lse [B, H, T] as the device left them, both NaN-filled before)"""
    d = H * dh
    q = padded(qkv.reshape(B * T, 3 * d), up4(3 * d) + 4)
    out = torch.full((B * T + 2, up4(d) + 4), float('nan'), device=DEV)
    lse = torch.full((B, H, T), float('nan'), device=DEV)
    rc = lib().tgmx_mha_stream_train(q.data_ptr(), q.stride(0), B, T, H, dh, out.data_ptr(), out.stride(0), lse.data_ptr() if want_lse else None, drop,
                                     stream())
    return rc, out, lse


def check_forward(tag, qkv, B, T, H, dh, mask=None, drop=None):
    d = H * dh
    rc, out, lse = forward(qkv, B, T, H, dh, drop)
    assert rc == 0
    again = forward(qkv, B, T, H, dh, drop)[1]
    got = out[: B * T, :d].cpu()
    assert torch.equal(got, again[: B * T, :d].cpu())  # two launches, the same bits
    assert torch.isnan(out[B * T :]).all() and torch.isnan(out[:, d:]).all()  # nothing written past the data
    r64 = br.attention_forward(qkv.double(), H, mask).reshape(B * T, d)
    r32 = br.attention_forward(qkv, H, None if mask is None else mask.float()).reshape(B * T, d)
    e, n = dr.rel_err(got, r64), dr.rel_err(r32, r64)
    q, k, _ = (br._heads(t, H) for t in qkv.double().split(d, dim=-1))
    l64 = torch.logsumexp(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1)
    el = dr.rel_err(lse.cpu(), l64)
    print(f'{tag}: out vs float64 {e:.3e} (float32 restatement {n:.3e}), lse {el:.3e}')
    assert n <= FWD_BAR / 2 and e <= FWD_BAR and el <= FWD_BAR
    return out, lse


@pytest.mark.parametrize('B,T,H,dh', [(2, 129, 1, 4), (1, 129, 3, 5), (2, 191, 3, 4), (1, 191, 1, 128), (1, 193, 1, 100), (1, 193, 3, 128),
                                      (2, 257, 1, 5), (1, 257, 3, 100)])  # fmt: skip
def test_forward_kernel_matches_float64(B, T, H, dh):
    qkv = torch.randn(B, T, 3 * H * dh, generator=torch.Generator().manual_seed(T + dh))
    out, _ = check_forward(f'B {B} T {T} H {H} dh {dh}', qkv, B, T, H, dh)
    rc, plain, lse = forward(qkv, B, T, H, dh, want_lse=False)  # inference: no lse, the same bits
    assert rc == 0 and torch.isnan(lse).all() and torch.equal(plain[: B * T, : H * dh], out[: B * T, : H * dh])


def test_running_maximum_is_rescaled():
    """Scores 7.5 x (key block) + noise, exact in float32: every block moves every row's maximum, the largest sits in the last block
    (one key), and row 0 has all scores equal.  A missing or wrong rescale shows at once."""
    T, dh = 257, 4
    g = torch.Generator().manual_seed(1)
    half = lambda n, s: torch.randint(-s, s + 1, (T, n), generator=g).float() / s
    q = torch.cat([torch.full((T, 1), 2.0), half(3, 2)], dim=1)
    q[0] = 0
    k = torch.cat([(7.5 * (torch.arange(T) // 64).float())[:, None], half(3, 4)], dim=1)
    qkv = torch.cat([q, k, torch.randn(T, dh, generator=g)], dim=1)[None]
    s = q @ k.t() / 2
    assert 29 < float(s.max()) < 33 and int(s[1:].argmax(dim=1).min()) == T - 1
    check_forward('rising maxima', qkv, 1, T, 1, dh)


@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('B,T,H,dh', [(2, 129, 2, 5), (1, 129, 1, 100), (1, 257, 2, 5), (1, 257, 1, 100)])
def test_backward_kernel_matches_float64_autograd(B, T, H, dh, p):
    d, seed, st = H * dh, 77, 64 * T
    g = torch.Generator().manual_seed(T + dh)
    qkv, datt = torch.randn(B, T, 3 * d, generator=g), torch.randn(B, T, d, generator=g)
    mask = br.site_masks(p, seed, st, 1, B, H, T, d)[0][0] if p else None
    out, lse = check_forward(f'B {B} T {T} H {H} dh {dh} p {p}', qkv, B, T, H, dh, mask, desc(p, seed, st))  # the forward under that mask, first
    q, do = padded(qkv.reshape(B * T, 3 * d), up4(3 * d) + 4), padded(datt.reshape(B * T, d), out.stride(0), rows=2)

    def run():
        dqkv, delta = torch.full_like(q, float('nan')), torch.empty((B, H, T), device=DEV)
        rc = lib().tgmx_mha_stream_backward(q.data_ptr(), q.stride(0), out.data_ptr(), do.data_ptr(), out.stride(0), lse.data_ptr(), B, T, H, dh,
                                            dqkv.data_ptr(), delta.data_ptr(), desc(p, seed, st), stream())
        assert rc == 0
        return dqkv.cpu()

    dqkv = run()
    assert torch.equal(dqkv[:, : 3 * d], run()[:, : 3 * d])  # two runs, the same bits
    assert torch.isnan(dqkv[:, 3 * d :]).all()  # the padding columns are not touched
    refs = []
    for dt in (torch.float64, torch.float32):
        x = qkv.to(dt).requires_grad_(True)
        (br.attention_forward(x, H, None if mask is None else mask.to(dt)) * datt.to(dt)).sum().backward()
        refs.append(x.grad.reshape(B * T, 3 * d))
    for i, name in enumerate(('dQ', 'dK', 'dV')):
        sl = slice(i * d, (i + 1) * d)
        e, n = br.max_ratio(dqkv[:, sl], refs[0][:, sl]), br.max_ratio(refs[1][:, sl], refs[0][:, sl])
        print(f'B {B} T {T} H {H} dh {dh} p {p} {name}: vs float64 {e:.3e} (float32 restatement {n:.3e})')
        assert n <= GRAD_BAR / 2 and e <= GRAD_BAR


@pytest.mark.parametrize('p', [0.0, 0.5])
def test_transformer_encoder_trains_on_the_long_route(p):
    B, T, d, H = 2, 129, 20, 2
    m = layer_module(d, H, p, 5)
    x = (torch.randn(B, T, d, generator=torch.Generator().manual_seed(T)).to(DEV) * 1.2 + 0.2).requires_grad_(True)
    up = torch.randn(B, T, d, generator=torch.Generator().manual_seed(9)).to(DEV)
    y = m(x)
    assert type(y.grad_fn).__name__ == 'LayerFunctionBackward'
    (y * up).sum().backward()
    masks = br.site_masks(p, torch.initial_seed(), 64 * m.__dict__['_tgmx_drop_calls'], 1, B, H, T, d)[0] if p else None
    y64, dx64, d64 = layer_reference(m, x.detach(), up, H, masks, torch.float64)
    y32, dx32, d32 = layer_reference(m, x.detach(), up, H, masks, torch.float32)
    assert dr.rel_err(y32, y64) <= FWD_BAR / 2 and dr.rel_err(y, y64) <= FWD_BAR
    for name, got, r64, r32 in [('dx', x.grad, dx64, dx32)] + [(n, q.grad, d64[n], d32[n]) for n, q in m.named_parameters()]:
        e, n32 = br.max_ratio(got, r64), br.max_ratio(r32, r64)
        print(f'p {p} {name}: vs float64 {e:.3e} (float32 restatement {n32:.3e})')
        assert n32 <= GRAD_BAR / 2 and e <= GRAD_BAR
    if not p:
        with torch.no_grad():
            assert torch.equal(m.eval()(x.detach()), y.detach())  # the inference call's bits


@pytest.mark.parametrize('route', ['native', 'torch'])
def test_encoder_with_272_tokens_per_pair(route, monkeypatch):
    from tgm_amd.nn import DyGFormer

    monkeypatch.setenv('TGMX_DYGFORMER_LONG', route)
    torch.manual_seed(3)
    b = wiki_batches(E=1000, bs=50, k=135, D=5)[8]
    m = DyGFormer(6, 5, 8, output_dim=7, num_layers=1, device=DEV, max_input_sequence_length=136, patch_size=1, channel_embedding_dim=4, num_heads=2)
    m = m.to(DEV).eval()
    assert not m._native_ok(136) and m._native_long_ok(136) == (route == 'native')
    took_native, orig = [], m._forward_native
    monkeypatch.setattr(m, '_forward_native', lambda *a, **k: took_native.append(1) or orig(*a, **k))
    node_x = torch.randn(400, 6, device=DEV)
    nids, nt, nx = gathered(b, *pair_rows(b, False))
    with torch.no_grad():
        zs, zd = m(node_x, torch.stack([b.edge_src, b.edge_dst]), b.edge_time, nids, nt, nx)
    assert took_native == ([1] if route == 'native' else [])  # the one-call forward ran / the same call composes
    r = cpu_restated(m, node_x, b.edge_src, b.edge_dst, b.edge_time, nids, nt, nx)
    if route == 'native':
        r32 = cpu_restated(m, node_x, b.edge_src, b.edge_dst, b.edge_time, nids, nt, nx, dtype=torch.float32)
        assert max(dr.rel_err(r32[0], r[0]), dr.rel_err(r32[1], r[1])) <= FWD_BAR / 2
        assert max(dr.rel_err(zs, r[0]), dr.rel_err(zd, r[1])) <= FWD_BAR


def test_envelope_edges_and_refusals():
    from tgm_amd import _native

    ok = lib().tgmx_mha_stream_supported
    assert [ok(128, 4), ok(129, 1), ok(4096, 128), ok(4097, 4), ok(129, 129), ok(129, 0)] == [0, 1, 1, 0, 0, 0]
    for T, dh in ((128, 4), (4097, 4), (129, 129)):
        qkv = torch.zeros(1, T, 3 * dh)
        rc, out, lse = forward(qkv, 1, T, 1, dh)
        assert rc == _native.E_UNSUPPORTED and torch.isnan(out).all() and torch.isnan(lse).all()
        q, dqkv = padded(qkv[0], up4(3 * dh)), torch.full((T, up4(3 * dh)), float('nan'), device=DEV)
        zeros = torch.zeros_like(out)
        rc = lib().tgmx_mha_stream_backward(q.data_ptr(), q.stride(0), zeros.data_ptr(), zeros.data_ptr(), out.stride(0), zeros.data_ptr(), 1, T, 1, dh,
                                            dqkv.data_ptr(), lse.data_ptr(), None, stream())
        assert rc == _native.E_UNSUPPORTED and torch.isnan(dqkv).all() and torch.isnan(lse).all()
