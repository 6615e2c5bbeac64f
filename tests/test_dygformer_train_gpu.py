"""DyGFormer's native training path on the device: the attention backward alone at every edge of its kernel, its envelope, the mean /
time / co-occurrence tails alone, the whole model and ``TransformerEncoder`` alone against the float64 restatement
(``dygformer_bwd_restate.py``) with and without dropout, the forward's bits, the dispatch decisions and the binding of a call's weights.

The bar on every gradient is the project's: 1e-4 of the tensor's largest entry against float64.  Each comparison prints the figure and
its ratio to a float32 run of the same restatement before it asserts (DESIGN.md 3.5 records them).

The co-occurrence table's ReLU: where float64 and float32 disagree on the sign of ``w1 c + b1`` the gradient jumps, so the weights come
from ``dygformer_restate.hashed_state_dict`` with seeds (found on the host) for which ``min |w1 c + b1| > 1e-3`` over c = 0 .. L and all
channels; every test asserts that on the host before comparing.  A condition on the inputs, not a tolerance.
"""
import functools

import numpy as np
import pytest
import torch

import dygformer_bwd_restate as br
import dygformer_restate as dr
from test_dygformer_gpu import pair_rows, wiki_batches

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-4
F64 = torch.float64


def up4(n):
    return (n + 3) // 4 * 4


def lib():
    from tgm_amd import _native

    return _native.load()


def stream():
    from tgm_amd import _native

    return _native.stream_ptr()


def desc(p, seed, st):
    from tgm_amd import _native

    return _native.dropout_desc(p, seed, st)


def report(tag, got, ref64, ref32=None):
    """max |got - ref| / max |ref| against float64, printed with its ratio to the float32 restatement's, then held to the bar."""
    e = br.max_ratio(got, ref64)
    n = br.max_ratio(ref32, ref64) if ref32 is not None else float('nan')
    print(f'{tag}: HIP vs float64 {e:.3e}' + (f', float32 restatement vs float64 {n:.3e}, ratio {e / n if n > 0 else float("inf"):.2f}' if ref32 is not None else ''))
    assert e <= BAR, (tag, e)
    return e


# ---- the attention backward alone ---------------------------------------------------------------------------------------------------------------
def mha_backward(qkv, datt, B, T, H, dh, drop=None):
    """qkv [B T, ldq], datt [B T, ldo] on the device -> (rc, dqkv [B T, ldq])"""
    dqkv = torch.full_like(qkv, float('nan'))
    rc = lib().tgmx_mha_small_backward(qkv.data_ptr(), qkv.stride(0), datt.data_ptr(), datt.stride(0), B, T, H, dh, dqkv.data_ptr(), drop, stream())
    return rc, dqkv


def mha_forward(qkv, B, T, H, dh, drop=None):
    out = torch.zeros((B * T, up4(H * dh)), device=DEV)
    rc = lib().tgmx_mha_small_train(qkv.data_ptr(), qkv.stride(0), B, T, H, dh, out.data_ptr(), out.stride(0), drop, stream())
    assert rc == 0
    return out


def attention_case(B, T, H, dh, seed):
    g = torch.Generator().manual_seed(seed)
    d = H * dh
    qkv = torch.randn(B, T, 3 * d, generator=g) * 1.3
    datt = torch.randn(B, T, d, generator=g)
    pad = lambda t, ld: torch.cat([t.reshape(B * T, -1), torch.full((B * T, ld - t.shape[-1]), 7.0)], dim=1).to(DEV).contiguous()
    return qkv, datt, pad(qkv, up4(3 * d)), pad(datt, up4(d))


@pytest.mark.parametrize('H,dh', [(1, 1), (1, 3), (2, 4), (3, 5), (2, 100)])
@pytest.mark.parametrize('T', [1, 2, 15, 16, 17, 33, 64])
def test_attention_backward_matches_the_restatement(T, H, dh):
    d = H * dh
    for B in (1, 3):
        qkv, datt, qkv_d, datt_d = attention_case(B, T, H, dh, 1000 * T + 10 * d + B)
        for p in (0.0, 0.5):
            seed, st = 77, 64 * (T + B)
            mask = None if not p else br.site_masks(p, seed, st, 1, B, H, T, d)[0][0]
            rc, dqkv = mha_backward(qkv_d, datt_d, B, T, H, dh, desc(p, seed, st))
            assert rc == 0
            _, again = mha_backward(qkv_d, datt_d, B, T, H, dh, desc(p, seed, st))
            got = dqkv[:, : 3 * d].cpu()
            assert torch.equal(got, again[:, : 3 * d].cpu())  # two runs, the same bits
            assert torch.isnan(dqkv[:, 3 * d :]).all()  # the padding columns are not touched
            r64 = br.attention_backward(qkv.double(), datt.double(), H, None if mask is None else mask).reshape(B * T, 3 * d)
            r32 = br.attention_backward(qkv, datt, H, None if mask is None else mask.float()).reshape(B * T, 3 * d)
            for i, name in enumerate(('dQ', 'dK', 'dV')):
                sl = slice(i * d, (i + 1) * d)
                report(f'T {T} H {H} dh {dh} B {B} p {p} {name}', got[:, sl], r64[:, sl], r32[:, sl])
            # the forward with the same mask
            att = mha_forward(qkv_d, B, T, H, dh, desc(p, seed, st))[:, :d].cpu()
            report(f'T {T} H {H} dh {dh} B {B} p {p} att', att, br.attention_forward(qkv.double(), H, mask).reshape(B * T, d))
            if not p:
                plain = torch.zeros_like(datt_d)
                assert lib().tgmx_mha_small(qkv_d.data_ptr(), qkv_d.stride(0), B, T, H, dh, plain.data_ptr(), plain.stride(0), stream()) == 0
                assert torch.equal(plain[:, :d].cpu(), att)  # NULL descriptor: the inference kernel's bits


@pytest.mark.parametrize('T,H,dh', [(17, 2, 4), (64, 2, 100), (33, 3, 5)])
def test_attention_backward_dropped_probabilities_give_exact_zeros(T, H, dh):
    B, d, p, seed, st = 3, H * dh, 0.5, 5, 192
    qkv, _, qkv_d, _ = attention_case(B, T, H, dh, T + dh)
    b0, i0, h0, c0 = B - 1, T // 2, H - 1, dh - 1
    datt = torch.zeros((B * T, up4(d)), device=DEV)
    datt[b0 * T + i0, h0 * dh + c0] = 1.0
    rc, dqkv = mha_backward(qkv_d, datt, B, T, H, dh, desc(p, seed, st))
    assert rc == 0
    dv = dqkv[:, 2 * d : 3 * d].cpu().reshape(B, T, d)
    dropped = br.site_masks(p, seed, st, 1, B, H, T, d)[0][0][b0, h0, i0] == 0  # [T]: the columns of row i0 that were dropped
    assert dropped.any() and (~dropped).any()
    col = dv[b0, :, h0 * dh + c0]
    assert (col[dropped] == 0).all() and (col[~dropped] > 0).all()  # dV[j, c0] = (P o m)[i0, j]
    other = dv.clone()
    other[b0, :, h0 * dh + c0] = 0
    assert (other == 0).all()


def test_attention_backward_refuses_outside_its_envelope():
    from tgm_amd import _native
    from tgm_amd.nn import _dygformer_train as tr

    for T, dh in ((80, 100), (128, 5), (64, 128), (128, 32), (129, 4), (4, 129)):
        assert not tr.train_supported(T, dh)
        qkv = torch.zeros((T, up4(3 * dh)), device=DEV)
        datt = torch.zeros((T, up4(dh)), device=DEV)
        rc, _ = mha_backward(qkv, datt, 1, T, 1, dh)
        assert rc == _native.E_UNSUPPORTED, (T, dh, rc)
    assert tr.train_supported(128, 4) and tr.train_supported(64, 100)


# ---- TransformerEncoder alone ---------------------------------------------------------------------------------------------------------------------
def layer_module(d, H, p, seed):
    from tgm_amd.nn import TransformerEncoder

    torch.manual_seed(seed)
    m = TransformerEncoder(d, H, dropout=p).to(DEV).train()
    with torch.no_grad():
        for q in m.parameters():
            q.add_(0.05 * torch.randn_like(q))
    return m


def layer_reference(m, x, up, H, masks, dtype):
    w = {n: v.detach().cpu().to(dtype) for n, v in m.state_dict().items()}
    dx, d = br.layer_backward(w, x.cpu().to(dtype), up.cpu().to(dtype), H, masks if masks is None else [t.to(dtype) for t in masks])
    return br.layer_forward(w, x.cpu().to(dtype), H, masks if masks is None else [t.to(dtype) for t in masks]), dx, d


def check_layer(m, x, H, p, tag, native=True):
    B, T, d = x.shape
    x = x.clone().requires_grad_(True)
    up = torch.randn(B, T, d, generator=torch.Generator().manual_seed(9)).to(DEV)
    y = m(x)
    assert (type(y.grad_fn).__name__ == 'LayerFunctionBackward') == native, type(y.grad_fn).__name__
    (y * up).sum().backward()
    masks = None
    if p and native:
        masks = br.site_masks(p, torch.initial_seed(), 64 * m.__dict__['_tgmx_drop_calls'], 1, B, H, T, d)[0]
    y64, dx64, d64 = layer_reference(m, x.detach(), up, H, masks, F64)
    y32, dx32, d32 = layer_reference(m, x.detach(), up, H, masks, torch.float32)
    report(f'{tag} out', y.detach(), y64, y32)
    worst = report(f'{tag} dx', x.grad, dx64, dx32)
    for n, q in m.named_parameters():
        worst = max(worst, report(f'{tag} {n}', q.grad, d64[n], d32[n]))
    return worst


@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('H', [1, 2])
@pytest.mark.parametrize('B,T,d', [(1, 1, 4), (3, 17, 20), (2, 64, 200)])
def test_transformer_encoder_alone_trains_natively(B, T, d, H, p):
    from tgm_amd.nn import _dygformer_train as tr

    native = tr.train_supported(T, d // H)  # (64 tokens at head dimension 200 are outside: that case composes, and has to match as well)
    assert native == ((T, d // H) != (64, 200))
    m = layer_module(d, H, p, B * T + d + H)
    x = torch.randn(B, T, d, generator=torch.Generator().manual_seed(T)).to(DEV) * 1.2 + 0.2
    if native or not p:
        check_layer(m, x, H, p, f'layer B {B} T {T} d {d} H {H} p {p}', native=native)
    else:  # composed with torch's own dropout: no masks to regenerate, the dispatch is what there is to check
        y = m(x.clone().requires_grad_(True))
        assert type(y.grad_fn).__name__ != 'LayerFunctionBackward' and torch.isfinite(y).all()
    with torch.no_grad():  # eval, no gradients: the inference kernel; with p = 0 the training forward returned its bits
        e = m.eval()(x)
    if not p and native:
        assert torch.equal(e, m.train()(x.clone().requires_grad_(True)).detach())


@pytest.mark.parametrize('T,d,H', [(64, 128, 1), (128, 32, 1)], ids=['T64_dh128', 'T128_dh32'])
def test_outside_the_training_envelope_the_layer_composes_and_matches(T, d, H):
    m = layer_module(d, H, 0.0, T + d)
    x = torch.randn(2, T, d, generator=torch.Generator().manual_seed(T)).to(DEV)
    check_layer(m, x, H, 0.0, f'composed layer T {T} d {d}', native=False)


# ---- the tails alone ---------------------------------------------------------------------------------------------------------------------------------
# (L, C) -> seed with min |w1 c + b1| > 1e-3 (found on the host; asserted where used)
CO_SEEDS = {(1, 1): 1, (1, 6): 1, (1, 50): 1, (2, 1): 1, (2, 6): 1, (2, 50): 2, (8, 1): 1, (8, 6): 1, (8, 50): 2, (33, 1): 1, (33, 6): 1, (33, 50): 2}
MODEL_SEEDS = {'odd': 1, 'example': 13, 'single': 1}  # the same for the whole models' hashed weights


def co_weights(L, C):
    sd = dr.hashed_state_dict({br.CO + '0.weight': [C, 1], br.CO + '0.bias': [C], br.CO + '2.weight': [C, C], br.CO + '2.bias': [C]}, CO_SEEDS[(L, C)])
    assert br.relu_margin(sd, L) > 1e-3
    return sd


def tail_inputs(P, L, seed, device=DEV):
    """Pair-major host tensors: ids [2 P, L], dt [2 P, L] (float32 values), and what the device reads.  The time gaps stay below 80: the
    sine's argument fma(dt, w, b) is formed in float32 as the forward forms it, so it carries 2^-24 |arg| of rounding -- 5e-6 at 80; at
    gaps of 1000 it is 6e-5, and a float32 run of the restatement itself misses the bar on a cancelling sum of 16 terms."""
    g = torch.Generator().manual_seed(seed)
    k, S = L - 1, 2 * P + 1
    nids = torch.randint(0, 5, (S, k), generator=g, dtype=torch.int32)
    nids[torch.rand(S, k, generator=g) < 0.3] = -1
    nt = torch.randint(960, 1000, (S, k), generator=g)
    src, dst = torch.randint(0, 5, (P,), generator=g, dtype=torch.int32), torch.randint(0, 5, (P,), generator=g, dtype=torch.int32)
    dst[0] = src[0]
    t = torch.randint(1000, 1040, (P,), generator=g)
    perm = torch.randperm(S, generator=g)
    src_rows, dst_rows = perm[:P].int(), perm[P : 2 * P].int()
    if P > 1:
        src_rows[1] = S + 5  # out of range: all pads
    else:
        dst_rows[0] = -1
    ids = torch.full((2 * P, L), -1, dtype=torch.int64)
    dt = torch.zeros((2 * P, L), dtype=torch.float32)
    for p in range(P):
        for side, (seeds, rows) in enumerate(((src, src_rows), (dst, dst_rows))):
            q, r = 2 * p + side, int(rows[p])
            ids[q, 0] = int(seeds[p])
            if 0 <= r < S:
                ids[q, 1:] = nids[r].long()
                dt[q, 1:] = (t[p] - nt[r]).float()
    dev = lambda v: v.to(device).contiguous()
    return dict(ids=ids, dt=dt, src=dev(src), dst=dev(dst), t=dev(t), nids=dev(nids), nt=dev(nt), src_rows=dev(src_rows), dst_rows=dev(dst_rows), S=S)


@pytest.mark.parametrize('C', [1, 6, 50])
@pytest.mark.parametrize('dT', [1, 7])
@pytest.mark.parametrize('L', [1, 2, 8, 33])
@pytest.mark.parametrize('P', [1, 3])
def test_mean_time_and_cooccurrence_tails(P, L, dT, C):
    from tgm_amd import _native
    from tgm_amd.nn import _dygformer_train as tr

    i = tail_inputs(P, L, 100 * P + L)
    n, k, D = 2 * P * L, L - 1, 4 * C
    g = torch.Generator().manual_seed(L + dT + C)
    st, ptr = stream(), _native.ptr
    # the patch mean (patch 1: Np = L)
    ldm = up4(D)
    dmean = torch.randn(2 * P, ldm, generator=g)
    dx = torch.full((n, ldm), float('nan'), device=DEV)
    dmean_d = dmean.to(DEV)
    assert lib().tgmx_dygformer_mean_backward(dmean_d.data_ptr(), ldm, P, L, D, dx.data_ptr(), ldm, st) == 0
    report(f'P {P} L {L} C {C} mean', dx[:, :D].cpu(), br.mean_backward(dmean[:, :D].double(), P, L).reshape(n, D))
    # the time channel
    ldt = up4(dT)
    tw = torch.from_numpy((0.05 / 10 ** np.linspace(0, 3, dT)).astype(np.float32))  # |arg| < 5: its float32 rounding stays below 3e-7
    tb = torch.randn(dT, generator=g) * 0.3
    dtime = torch.randn(n, ldt, generator=g)
    rows = torch.full((n, 2 * dT), float('nan'), device=DEV)
    tw_d, tb_d, dtime_d = tw.to(DEV), tb.to(DEV), dtime.to(DEV)
    assert lib().tgmx_dygformer_time_backward(dtime_d.data_ptr(), ldt, i['src'].data_ptr(), i['dst'].data_ptr(), i['t'].data_ptr(), P, ptr(i['nids']),
                                              ptr(i['nt']), i['S'], k, i['src_rows'].data_ptr(), i['dst_rows'].data_ptr(), tw_d.data_ptr(), tb_d.data_ptr(),
                                              dT, rows.data_ptr(), st) == 0  # fmt: skip
    rows = rows.cpu()
    valid = (i['ids'] != -1).unsqueeze(-1).double()
    assert (rows.reshape(2 * P, L, 2 * dT)[i['ids'] == -1] == 0).all()  # pad slots give 0
    assert (rows.reshape(2 * P, L, 2 * dT)[:, 0, :dT] == 0).all()  # slot 0: dt = 0
    dw, db = br.time_backward(dtime[:, :dT].reshape(2 * P, L, dT).double(), i['dt'].double().unsqueeze(-1), valid, tw.double(), tb.double())
    dw32, db32 = br.time_backward(dtime[:, :dT].reshape(2 * P, L, dT), i['dt'].unsqueeze(-1), valid.float(), tw, tb)
    # a condition on the inputs, as the ReLU one: a gradient that is one or two terms next to a zero of the sine has no digits to compare in
    # float32, whoever computes it -- the float32 restatement itself has to be well inside the bar
    assert max(br.max_ratio(dw32, dw), br.max_ratio(db32, db)) <= BAR / 4
    report(f'P {P} L {L} dT {dT} d time weight', rows[:, :dT].double().sum(dim=0).reshape(-1, 1), dw, dw32)
    report(f'P {P} L {L} dT {dT} d time bias', rows[:, dT:].double().sum(dim=0), db, db32)
    # the co-occurrence encoder
    sd = co_weights(L, C)
    counts = torch.full((n, 2), -7, dtype=torch.int32, device=DEV)
    assert lib().tgmx_dygformer_cooccurrence(i['src'].data_ptr(), i['dst'].data_ptr(), P, ptr(i['nids']), i['S'], k, i['src_rows'].data_ptr(),
                                             i['dst_rows'].data_ptr(), None, None, None, None, 0, None, counts.data_ptr(), None, 0, st) == 0  # fmt: skip
    cs, cd = dr.cooccurrence_counts(i['ids'][0::2].numpy(), i['ids'][1::2].numpy())
    want = torch.from_numpy(np.stack([cs, cd], axis=1).reshape(n, 2))  # pair-major
    assert torch.equal(counts.cpu().long(), want)
    assert int(want.max()) > 1 or L <= 2  # ids drawn from 5 values: counts above 1
    ldf = up4(C)
    dfeat = torch.randn(n, ldf, generator=g)
    w = {name: v.to(DEV).contiguous() for name, v in sd.items()}
    w2T = w[br.CO + '2.weight'].t().contiguous()
    grads = {name: torch.full_like(v, float('nan')) for name, v in w.items()}
    dfeat_d = dfeat.to(DEV)
    for run in range(2):
        tr.cooccurrence_backward(counts.data_ptr(), dfeat_d.data_ptr(), ldf, n, L, C, w[br.CO + '0.weight'].data_ptr(), w[br.CO + '0.bias'].data_ptr(),
                                 w2T.data_ptr(), grads[br.CO + '0.weight'].data_ptr(), grads[br.CO + '0.bias'].data_ptr(),
                                 grads[br.CO + '2.weight'].data_ptr(), grads[br.CO + '2.bias'].data_ptr(), torch.device(DEV))  # fmt: skip
        if run == 0:
            first = {name: v.clone() for name, v in grads.items()}
    assert all(torch.equal(first[name], grads[name]) for name in grads)
    r64 = br.cooccurrence_backward(dfeat[:, :C].double(), want, L, *(sd[br.CO + s].double() for s in ('0.weight', '0.bias', '2.weight')))
    r32 = br.cooccurrence_backward(dfeat[:, :C], want, L, *(sd[br.CO + s] for s in ('0.weight', '0.bias', '2.weight')))
    for name in grads:
        report(f'P {P} L {L} C {C} {name}', grads[name], r64[name], r32[name])


# ---- the whole model ------------------------------------------------------------------------------------------------------------------------------
CASES = {
    'odd': dict(dims=dict(node_feat_dim=3, edge_x_dim=13, time_feat_dim=7, channel_embedding_dim=5, output_dim=9, patch_size=2, num_layers=3, num_heads=2,
                          max_input_sequence_length=6), bs=9, E=360, batch=25),  # fmt: skip
    'example': dict(dims=dict(node_feat_dim=128, edge_x_dim=172, time_feat_dim=100, channel_embedding_dim=50, output_dim=172, patch_size=1, num_layers=2,
                              num_heads=2, max_input_sequence_length=32), bs=24, E=960, batch=30),  # fmt: skip
    'single': dict(dims=dict(node_feat_dim=2, edge_x_dim=3, time_feat_dim=2, channel_embedding_dim=2, output_dim=3, patch_size=1, num_layers=2, num_heads=1,
                             max_input_sequence_length=1), bs=1, E=0, batch=0),  # fmt: skip
}


def hashed_model(name, p, seed=None):
    from tgm_amd.nn import DyGFormer

    c = CASES[name]
    m = DyGFormer(**c['dims'], dropout=p, device='cpu')
    shapes = {n: list(v.shape) for n, v in m.state_dict().items()}
    sd = dr.hashed_state_dict(shapes, MODEL_SEEDS[name] if seed is None else seed)
    m.load_state_dict(sd, strict=True)
    return m, sd


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """The device inputs of ``encode_pairs`` (hop 0 of a sampler batch, source rows and NEGATIVE destination rows) and the gathered host
    copies the restatement takes."""
    c = CASES[name]
    d = c['dims']
    k = d['max_input_sequence_length'] - 1
    torch.manual_seed(11)
    node_x = torch.randn(400, d['node_feat_dim'])
    if name == 'single':  # L = 1: no neighbour slots at all
        src, dst, t = torch.tensor([3], dtype=torch.int32), torch.tensor([8], dtype=torch.int32), torch.tensor([50])
        nids, nt, nx = torch.zeros((3, 0), dtype=torch.int32), torch.zeros((3, 0), dtype=torch.int64), torch.zeros((3, 0, d['edge_x_dim']))
        sr, dr_ = torch.tensor([0], dtype=torch.int32), torch.tensor([2], dtype=torch.int32)
    else:
        b = wiki_batches(E=c['E'], bs=c['bs'], k=k, D=d['edge_x_dim'])[c['batch']]
        sr, dr_ = pair_rows(b, True)
        src, dst, t, nids, nt, nx = b.edge_src, b.neg, b.edge_time, b.nbr_nids[0], b.nbr_edge_time[0], b.nbr_edge_x[0]
        assert 0 < float((nids[torch.cat([sr, dr_]).long()] == -1).float().mean()) < 1  # pads, and not only pads
    dev = tuple(v.to(DEV) for v in (node_x, src, dst, t, nids, nt, nx, sr, dr_))
    rows = torch.cat([sr, dr_]).long().cpu()
    host = (node_x, src.cpu(), dst.cpu(), t.cpu(), nids.cpu()[rows], nt.cpu()[rows], nx.cpu()[rows])
    return dev, host


def shapes_of(name):
    d = CASES[name]['dims']
    P = case_inputs(name)[0][1].numel()
    T = 2 * d['max_input_sequence_length'] // d['patch_size']
    return P, d['num_heads'], T, 4 * d['channel_embedding_dim']


@functools.lru_cache(maxsize=None)
def reference(name, p, seed, first_stream, dtype):
    """(zs, zd, gradients by name) of the restatement under the upstream weights of :func:`upstream`; with p = 0 in float64 the gradients
    are float64 AUTOGRAD of ``dygformer_restate.dygformer_forward``, otherwise the hand-written backward with the regenerated masks."""
    d = CASES[name]['dims']
    _, sd = hashed_model(name, p)
    assert br.relu_margin(sd, d['max_input_sequence_length']) > 1e-3
    host = case_inputs(name)[1]
    P, H, T, D = shapes_of(name)
    masks = br.site_masks(p, seed, first_stream, d['num_layers'], P, H, T, D, dtype)
    ws, wd = upstream(P, d['output_dim'])
    if not p and dtype == F64:
        leaves = {n: v.double().requires_grad_(True) for n, v in sd.items()}
        zs, zd = dr.dygformer_forward(leaves, d['patch_size'], d['num_layers'], H, *host)
        ((zs * ws.double()).sum() + (zd * wd.double()).sum()).backward()
        return zs.detach(), zd.detach(), {n: v.grad for n, v in leaves.items()}
    zs, zd = br.encoder_forward(sd, d['patch_size'], d['num_layers'], H, *host, masks=masks, dtype=dtype)
    return zs, zd, br.encoder_backward(sd, d['patch_size'], d['num_layers'], H, *host, ws.to(dtype), wd.to(dtype), masks=masks, dtype=dtype)


def upstream(P, E):
    g = torch.Generator().manual_seed(21)
    return torch.randn(P, E, generator=g), torch.randn(P, E, generator=g)


def run_model(m, name):
    node_x, src, dst, t, nids, nt, nx, sr, dr_ = case_inputs(name)[0]
    zs, zd = m.encode_pairs(node_x, src, dst, t, nids, nt, nx, sr, dr_)
    return zs, zd


def train_step(m, name):
    """Forward and backward under the fixed upstream weights: (zs, zd, gradients by name)."""
    m.zero_grad(set_to_none=True)
    zs, zd = run_model(m, name)
    ws, wd = (v.to(DEV) for v in upstream(zs.shape[0], zs.shape[1]))
    ((zs * ws).sum() + (zd * wd).sum()).backward()
    return zs.detach(), zd.detach(), {n: (None if q.grad is None else q.grad.clone()) for n, q in m.named_parameters()}


def compare_model(tag, got, name, p, seed=0, first_stream=0):
    zs, zd, grads = got
    rs, rd, r64 = reference(name, p, seed, first_stream, F64)
    ts, td, r32 = reference(name, p, seed, first_stream, torch.float32)
    report(f'{tag} forward', torch.cat([zs, zd]), torch.cat([rs, rd]), torch.cat([ts, td]))
    worst = 0.0
    assert len(grads) == 2 + 4 + 8 + 2 + 12 * CASES[name]['dims']['num_layers']
    for n, g in grads.items():
        assert g is not None, n
        worst = max(worst, report(f'{tag} {n}', g, r64[n], r32[n]))
    print(f'{tag}: worst gradient ratio {worst:.3e}')


@pytest.mark.parametrize('name', list(CASES))
def test_model_gradients_match_float64_autograd(name):
    m, _ = hashed_model(name, 0.0)
    m = m.to(DEV).train()
    got = train_step(m, name)
    compare_model(f'{name} p 0', got, name, 0.0)


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('name', ['odd', 'example'])
def test_model_with_dropout_matches_the_restatement_with_regenerated_masks(name, p):
    torch.manual_seed(1234)
    m, _ = hashed_model(name, p)
    m = m.to(DEV).train()
    first = train_step(m, name)
    assert m.__dict__['_tgmx_drop_calls'] == 1
    compare_model(f'{name} p {p}', first, name, p, torch.initial_seed(), 64)
    second = train_step(m, name)  # the call counter moves on: other masks
    assert not torch.equal(first[0], second[0])
    compare_model(f'{name} p {p} call 2', second, name, p, torch.initial_seed(), 128)
    torch.manual_seed(1234)  # the same seed and the same call index reproduce the first call
    m.__dict__['_tgmx_drop_calls'] = 0
    again = train_step(m, name)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert all(torch.equal(first[2][n], again[2][n]) for n in first[2])


# ---- forward bits, dispatch, the binding of a call's weights ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['odd', 'example'])
def test_forward_bits_and_backward_bits(name, monkeypatch):
    m, _ = hashed_model(name, 0.0)
    m = m.to(DEV).train()
    monkeypatch.delenv('TGMX_DYGFORMER_BWD', raising=False)
    with torch.no_grad():
        es, ed = (v.clone() for v in run_model(m, name))
    a = train_step(m, name)
    assert torch.equal(a[0], es) and torch.equal(a[1], ed)  # grad-enabled at dropout 0 = the no-grad forward, bit for bit
    b = train_step(m, name)
    monkeypatch.setenv('TGMX_DYGFORMER_BWD', 'py')
    c = train_step(m, name)
    monkeypatch.setenv('TGMX_DYGFORMER_BWD', 'native')
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
        for n in a[2]:
            assert torch.equal(a[2][n], other[2][n]), n
    with torch.no_grad():
        fs, fd = run_model(m.eval(), name)
    assert torch.equal(fs, es) and torch.equal(fd, ed)


def test_dispatch(monkeypatch):
    from tgm_amd.nn import _dygformer_train as tr

    name = 'odd'
    monkeypatch.delenv('TGMX_DYGFORMER_BWD', raising=False)
    if tr.DEFAULT != 'native':
        monkeypatch.setenv('TGMX_DYGFORMER_BWD', 'native')
    m, _ = hashed_model(name, 0.0)
    m = m.to(DEV).train()
    fn = lambda mod=m: type(run_model(mod, name)[0].grad_fn).__name__
    assert fn() == 'DyGFormerFunctionBackward'
    node_x, src, dst, t, nids, nt, nx, sr, dr_ = case_inputs(name)[0]
    zs, _ = m.encode_pairs(node_x.clone().requires_grad_(True), src, dst, t, nids, nt, nx, sr, dr_)
    assert type(zs.grad_fn).__name__ != 'DyGFormerFunctionBackward'  # a gradient for node_x: composed
    a = m._inputs(node_x, src, dst, t, nids, nt, nx, sr, dr_)
    assert tr.in_envelope(m, a)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        assert not tr.in_envelope(m, a)  # autocast: composed
    monkeypatch.setenv('TGMX_DYGFORMER_BWD', 'torch')
    assert fn() != 'DyGFormerFunctionBackward'
    monkeypatch.setenv('TGMX_DYGFORMER_BWD', 'native')
    m2, _ = hashed_model(name, 0.1)
    m2 = m2.to(DEV).train()
    assert fn(m2) == 'DyGFormerFunctionBackward'
    m2.transformers[1].dropout.p = 0.3  # a layer's rate edited to differ
    assert fn(m2) != 'DyGFormerFunctionBackward'
    m2.transformers[1].dropout.p = 0.1
    assert fn(m2) == 'DyGFormerFunctionBackward'

    class MyTime(torch.nn.Module):
        def __init__(self, dim):
            super().__init__()
            self.w = torch.nn.Linear(1, dim)

        def forward(self, t):
            return torch.cos(self.w(t.unsqueeze(-1)))

    from tgm_amd.nn import DyGFormer

    m3 = DyGFormer(**CASES[name]['dims'], dropout=0.0, time_encoder=MyTime, device=DEV).to(DEV).train()
    assert fn(m3) != 'DyGFormerFunctionBackward'


def test_frozen_encoders_skip_their_tails():
    name = 'odd'
    m, _ = hashed_model(name, 0.0)
    m = m.to(DEV).train()
    full = train_step(m, name)[2]
    for frozen in ('time_encoder', 'co_occurrence_encoder'):
        for q in getattr(m, frozen).parameters():
            q.requires_grad_(False)
        part = train_step(m, name)[2]
        for n, g in part.items():
            if n.startswith(frozen):
                assert g is None, n
            else:
                assert torch.equal(g, full[n]), n
        for q in getattr(m, frozen).parameters():
            q.requires_grad_(True)


def test_a_call_keeps_the_weights_of_its_own_forward():
    """forward A, optimizer step, forward B, backward B, backward A: A is differentiated with A's weights."""
    name = 'odd'
    m, _ = hashed_model(name, 0.0)
    m = m.to(DEV).train()
    alone = train_step(m, name)[2]
    m.zero_grad(set_to_none=True)
    zs, zd = run_model(m, name)
    ws, wd = (v.to(DEV) for v in upstream(zs.shape[0], zs.shape[1]))
    loss_a = (zs * ws).sum() + (zd * wd).sum()
    with torch.no_grad():
        for q in m.parameters():
            q.add_(0.01 * torch.ones_like(q))  # an optimizer step (in place: the parameters' versions move on)
    zs2, zd2 = run_model(m, name)
    ((zs2 * ws).sum() + (zd2 * wd).sum()).backward()
    m.zero_grad(set_to_none=True)
    loss_a.backward()
    for n, q in m.named_parameters():
        assert torch.equal(q.grad, alone[n]), n
