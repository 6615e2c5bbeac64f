"""TPNet's native training path on the device (``tgm_amd/nn/_tpnet_train.py``, ``csrc/tpnet_bwd.hip``).

The new kernels alone, through ctypes, against the float64 restatement of ``tests/tpnet_bwd_restate.py``: outputs pre-filled with NaN inside
``Buf`` allocations whose sentinel columns and tail must stay intact, every case launched twice and compared bit for bit, and the assertion
err / bound <= 1 with bound = chain * 2^-24 * magnitude (``pytest -rP`` prints the worst ratio).  The token kernel at K in {1, 2, 7, 32}
(Ht = K // 2: K = 1 has no hidden unit), C in {1, 64, 65, 172} (one ragged chunk, one full, two with a ragged second -- three at K = 32,
whose chunk is 64 channels), Q in {1, 5}, with and without dropout, and once on columns that are constant over the K tokens; the time rows at
1, 63, 64, 65, 257 rows; the mean backward.

End to end against float64 autograd through the restatement at the project's bar for gradients (each within 1e-4 of its largest entry), on
the first batch of a stream (every slot padded) and a later one; then bit equality with the no-grad forward, repeat runs, the py mode, the
dispatch, frozen parameters, call sharing across an optimizer step, inputs overwritten before the backward, and dropout with the
regenerated masks.
"""
import copy
import functools

import pytest
import torch

import tpnet_bwd_restate as br
import tpnet_restate as tr
from oracle.tgat_bwd_ref import EPS
from test_tgat_bwd_blocks_gpu import Buf, _report, _same_bits
from test_tpnet_gpu import gathered, pair_rows, wiki_batches

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-4
F64 = torch.float64


@pytest.fixture(autouse=True)
def _native_mode(monkeypatch):
    """Every test here is about the native path, whichever way the default points."""
    monkeypatch.setenv('TGMX_TPNET_BWD', 'native')


def _lib():
    from tgm_amd import _native

    return _native.load(), _native


def up4(n):
    return (n + 3) // 4 * 4


# ---- the token kernel alone ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _token_case(K, C, Q, p, constant=False):
    g = torch.Generator().manual_seed(1000 * K + 10 * C + Q)
    Ht = K // 2
    P = [torch.randn(s, generator=g) * 0.5 + o for s, o in (((K,), 1.0), ((K,), 0.0), ((Ht, K), 0.0), ((Ht,), 0.0), ((K, Ht), 0.0), ((K,), 0.0))]
    x, dz1 = torch.randn(Q, K, C, generator=g) * 1.5, torch.randn(Q, K, C, generator=g)
    if constant:  # the K tokens of a sequence identical in every column, as in an all-pad TPNet sequence
        x = x[:, :1, :].expand(Q, K, C).contiguous()
    m = br.layer_masks(p, 77, 192, 1, Q, K, C, Ht, 1)
    want = br.partial_rows([t.double() for t in P], x.double(), dz1.double(), m[0], m[1])
    return P, x, dz1, Ht, want


def _launch_token(K, C, Q, p, with_part=True, constant=False):
    lib, nat = _lib()
    P, x, dz1, Ht, _ = _token_case(K, C, Q, p, constant)
    npart = br.part_floats(K, Ht)
    dP = [t.to(DEV).contiguous() for t in P]
    xb, db = Buf(Q * K, C, ld=up4(C) + 4, data=x.view(Q * K, C).to(DEV), fill=0.0), Buf(Q * K, C, ld=C + 1, data=dz1.view(Q * K, C).to(DEV), fill=0.0)
    dx, part = Buf(Q * K, C, ld=up4(C) + 8), Buf(Q, up4(npart) + 4)
    rc = lib.tgmx_tpnet_token_backward(xb.ptr, xb.ld, db.ptr, db.ld, Q, K, C, dP[0].data_ptr(), dP[1].data_ptr(), nat.ptr(dP[2]) if Ht else None,
                                       nat.ptr(dP[3]) if Ht else None, Ht, nat.ptr(dP[4]) if Ht else None, 1e-5, dx.ptr, dx.ld,
                                       part.ptr if with_part else None, part.ld, nat.dropout_desc(p, 77, 192 + 4), nat.dropout_desc(p, 77, 192 + 5),
                                       nat.stream_ptr())  # fmt: skip
    nat.check(rc, 'tgmx_tpnet_token_backward')
    torch.cuda.synchronize()
    return dx, part, npart


def _colsum(part, npart, Q):
    lib, nat = _lib()
    out = torch.full((npart,), float('nan'), device=DEV)
    ws = torch.empty(256 * npart, device=DEV)
    nat.check(lib.tgmx_colsum(part.ptr, part.ld, Q, npart, out.data_ptr(), 0, ws.data_ptr(), nat.stream_ptr()), 'tgmx_colsum')
    torch.cuda.synchronize()
    return out


def _check_token(K, C, Q, p, constant=False):
    _, _, _, Ht, want = _token_case(K, C, Q, p, constant)
    (dx, part, npart), (dx2, part2, _) = [_launch_token(K, C, Q, p, constant=constant) for _ in range(2)]
    assert _same_bits(dx.flat, dx2.flat) and _same_bits(part.flat, part2.flat)
    assert dx.sentinels_intact() and part.sentinels_intact()
    tag = f'tpnet token bwd K={K} C={C} Q={Q} Ht={Ht} p={p}' + (' constant' if constant else '')
    worst = _report(tag + ' dx', dx.view, want['dx'].reshape(Q * K, C), br.gm.token_chain(K, Ht) * EPS * want['dx_m'].reshape(Q * K, C))
    worst = max(worst, _report(tag + ' part', part.view[:, :npart].contiguous(), want['part'], br.part_chain(K, Ht, C) * EPS * want['part_m']))
    assert not part.view[:, npart:].any()  # the pad columns are written as zeros
    nr, _, _ = _launch_token(K, C, Q, p, with_part=False, constant=constant)  # no parameter gradient wanted: the same dx
    assert _same_bits(nr.flat, dx.flat)
    # ONE colsum over the Q rows is the six gradients, in the partial row's column order
    six = lambda suffix: torch.cat([want[n + suffix].reshape(-1) for n in br.PART_NAMES])
    got = _colsum(part, npart, Q)
    worst = max(worst, _report(tag + ' colsum', got, six(''), br.part_colsum_chain(K, Ht, C, Q) * EPS * six('_m')))
    return worst


@pytest.mark.parametrize('C', [1, 64, 65, 172])
@pytest.mark.parametrize('K', [1, 2, 7, 32])
def test_token_backward_alone(K, C):
    assert max(_check_token(K, C, Q, p) for Q in (1, 5) for p in (0.0, 0.5)) <= 1.0


def test_token_backward_on_constant_columns():
    """var = 0 and x-hat = 0 exactly with the refined mean: rstd = 1 / sqrt(eps), finite and within the bound."""
    assert max(_check_token(7, 65, 5, 0.0, constant=True), _check_token(32, 172, 1, 0.5, constant=True)) <= 1.0
    lib, nat = _lib()
    dx, part, npart = _launch_token(7, 65, 5, 0.0, constant=True)
    Ht, K = 3, 7
    gxh = part.view[:, 2 * K * Ht + 2 * K : 2 * K * Ht + 3 * K]
    assert not gxh.any()  # sum dxn x-hat: x-hat is exactly 0


def test_token_backward_refuses_what_does_not_fit():
    lib, nat = _lib()
    from tgm_amd.nn._tpnet_train import train_supported

    z = torch.zeros(40 * 8 * 3, device=DEV)  # K = 40, Ht = 20: a partial row of 1740 floats, 24 a thread of a 64-channel pass hold 1536
    rc = lib.tgmx_tpnet_token_backward(z.data_ptr(), 8, z.data_ptr() + 4 * 320, 8, 1, 40, 8, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 20,
                                       z.data_ptr(), 1e-5, z.data_ptr() + 4 * 640, 8, None, 1740, None, None, nat.stream_ptr())  # fmt: skip
    assert rc == nat.E_UNSUPPORTED and not train_supported(40, 8, 20) and train_supported(32, 8, 16)
    assert not train_supported(32, 400, 16)  # the forward's tile


# ---- the time rows and the mean backward alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dT', [1, 8, 100])
@pytest.mark.parametrize('R', [1, 63, 64, 65, 257])
def test_time_backward_alone(R, dT):
    lib, nat = _lib()
    g = torch.Generator().manual_seed(R * 131 + dT)
    lg = torch.log(torch.randint(1, 10**6, (R,), generator=g).double())
    pad = torch.rand(R, generator=g) < 0.3
    if R > 2:
        pad[0], pad[1], lg[1] = True, False, 0.0  # a pad row and a zero gap
    lg_dev = torch.where(pad, torch.full_like(lg, -1.0), lg).to(DEV)
    tw, tb, d = torch.randn(dT, generator=g), torch.randn(dT, generator=g), torch.randn(R, dT, generator=g)
    want = br.time_rows(d, lg, pad, tw, tb)
    dtw, dtb = tw.to(DEV), tb.to(DEV)
    outs = []
    for _ in range(2):
        db, rows = Buf(R, dT, ld=up4(dT) + 4, data=d.to(DEV)), Buf(R, 2 * dT)
        nat.check(lib.tgmx_tpnet_time_backward(db.ptr, db.ld, lg_dev.data_ptr(), R, dtw.data_ptr(), dtb.data_ptr(), dT, rows.ptr, nat.stream_ptr()),
                  'tgmx_tpnet_time_backward')  # fmt: skip
        torch.cuda.synchronize()
        outs.append(rows)
    assert _same_bits(outs[0].flat, outs[1].flat) and outs[0].sentinels_intact()
    assert _report(f'tpnet time bwd R={R} dT={dT}', outs[0].view, want['rows'], br.time_chain() * EPS * want['rows_m']) <= 1.0
    if R > 2:
        assert not outs[0].view[0].any() and not outs[0].view[1, :dT].any()


@pytest.mark.parametrize('C', [5, 130])
@pytest.mark.parametrize('Q,k', [(1, 1), (1, 7), (3, 1), (3, 7)])
def test_mean_backward_alone(Q, k, C):
    lib, nat = _lib()
    g = torch.randn(Q, C, generator=torch.Generator().manual_seed(Q * 17 + k + C))
    want = br.mean_backward(g, k)
    outs = []
    for _ in range(2):
        gb, dz = Buf(Q, C, ld=C + 2, data=g.to(DEV)), Buf(Q * k, C, ld=up4(C) + 4)
        nat.check(lib.tgmx_tpnet_mean_backward(gb.ptr, gb.ld, Q, k, C, dz.ptr, dz.ld, nat.stream_ptr()), 'tgmx_tpnet_mean_backward')
        torch.cuda.synchronize()
        outs.append(dz)
    assert _same_bits(outs[0].flat, outs[1].flat) and outs[0].sentinels_intact()
    assert _report(f'tpnet mean bwd Q={Q} k={k} C={C}', outs[0].view, want, br.mean_chain() * EPS * want.abs()) <= 1.0


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stream():
    torch.manual_seed(4)
    return wiki_batches(E=1200, bs=100, k=7, D=12), torch.randn(400, 4, device=DEV)


def _model(variant='concat', L=2, dropout=0.0, upto=3, seed=0):
    """``TPNet(4, 12, 8, 10, 7)`` over tables ``enforce_dim=8`` that have seen the stream's first ``upto`` batches."""
    from tgm_amd.nn import RandomProjectionModule, TPNet

    batches, _ = _stream()
    torch.manual_seed(seed)
    rp = None if variant == 'none' else RandomProjectionModule(400, 2, 1e-5, 0, use_matrix=False, enforce_dim=8, concat_src_dst=variant == 'concat')
    m = TPNet(4, 12, 8, 10, 7, num_layers=L, dropout=dropout, random_projections=rp, device=DEV).to(DEV).train()
    with torch.no_grad():
        for p in m.parameters():
            if p.requires_grad:
                p.add_(0.1 * torch.randn_like(p))
    if rp is not None:
        for pb in batches[:upto]:
            rp.update(pb.edge_src, pb.edge_dst, pb.edge_time)
    return m


def _weight(n, E, seed=7):
    return torch.randn(n, E, generator=torch.Generator().manual_seed(seed))


def _call(m, b, node_x, how='forward'):
    sr, dr_ = pair_rows(b, True)
    if how == 'forward':
        nids, nt, nx = gathered(b, sr, dr_)
        return m(node_x, torch.stack([b.edge_src, b.neg]), b.edge_time, nids, nt, nx)
    return m.encode_pairs(node_x, b.edge_src, b.neg, b.edge_time, b.nbr_nids[0], b.nbr_edge_time[0], b.nbr_edge_x[0], sr, dr_)


def _trainable(m):
    return {n: p for n, p in m.named_parameters() if n.split('.')[-1] in ('weight', 'bias')}


def _device(m, b, node_x, w, how='forward'):
    """One forward and backward on the device: (out, name -> gradient or None)."""
    m.zero_grad(set_to_none=True)
    out = torch.cat(_call(m, b, node_x, how))
    (out * w.to(DEV)).sum().backward()
    return out.detach(), {n: (None if p.grad is None else p.grad.clone()) for n, p in _trainable(m).items()}


def _reference(m, b, node_x, w, masks=None):
    """(out, name -> gradient, name -> magnitude for the mixers'): float64 autograd through the restatement's forward."""
    c = lambda v: v.detach().cpu()
    sd = {n: (c(v).double() if v.is_floating_point() else c(v)) for n, v in m.state_dict().items()}
    leaf = {n: (v.clone().requires_grad_(True) if n in _trainable(m) else v) for n, v in sd.items()}
    rp = m.random_projections
    rpd = None if rp is None else dict(num_layer=rp.num_layer, concat=rp.concat_src_dst, scale=rp.scale)
    nids, nt, nx = gathered(b, *pair_rows(b, True))
    pos = (c(node_x), c(b.edge_src), c(b.neg), c(b.edge_time), c(nids), c(nt), c(nx))
    out = torch.cat(br.forward(leaf, m.num_layers, rpd, *pos, masks=masks))
    (out * w.double()).sum().backward()
    keep, mags = {}, {}
    br.forward(sd, m.num_layers, rpd, *pos, masks=masks, keep=keep)
    dims = dict(dN=m.node_feat_dim, dT=m.time_feat_dim, dE=m.edge_x_dim, od=0 if rp is None else rp.out_dim)
    restated = br.backward(sd, m.num_layers, dims, keep, w, masks, mags=mags)
    return out.detach(), {n: leaf[n].grad for n in _trainable(m)}, mags, restated


def _check_bar(label, got, ref, mags):
    """Every gradient within BAR of its largest entry.  A gradient that is all cancellation (the first batch: every sequence is K equal pad
    tokens, so every column the token LayerNorm sees is constant and d token_norm.weight is 0 but for float64's own rounding) has no such
    scale: where the reference's largest entry is below 1e-12 of the restated magnitude's, that magnitude is the scale; a reference of
    exactly 0 (the time encoder on pads) asks for exactly 0."""
    worst = 0.0
    for name, r in ref.items():
        g = got[name]
        assert g is not None and g.dtype == torch.float32 and torch.isfinite(g).all(), (label, name)
        r = torch.zeros(g.shape, dtype=F64) if r is None else r
        assert g.shape == r.shape, (label, name)
        if r.numel() == 0:
            continue
        scale = r.abs().max().item()
        if name in mags and scale <= 1e-12 * mags[name].max().item():
            scale = mags[name].max().item()
        dist = (g.cpu().double() - r).abs().max().item()
        if scale == 0.0:
            assert dist == 0.0, (label, name, dist)
            continue
        worst = max(worst, dist / scale)
        assert dist / scale <= BAR, (label, name, dist / scale)
    print(f'tpnet train {label}: worst ratio {worst:.3e}')
    return worst


@pytest.mark.parametrize('which', ['first', 'later'])
@pytest.mark.parametrize('variant,L,how', [('concat', 2, 'forward'), ('cross', 2, 'pairs'), ('none', 2, 'forward'), ('concat', 0, 'pairs'), ('cross', 3, 'forward')])
def test_gradients_match_float64_autograd(variant, L, how, which):
    batches, node_x = _stream()
    upto = 0 if which == 'first' else 3
    b = batches[upto]
    m = _model(variant, L, upto=upto)
    nids = gathered(b, *pair_rows(b, True))[0]
    pads = int((nids == -1).sum())
    assert (pads == nids.numel()) if which == 'first' else (0 < pads < nids.numel())
    w = _weight(2 * b.edge_src.numel(), m.output_dim)
    out, got = _device(m, b, node_x, w, how)
    assert type(_call(m, b, node_x, how)[0].grad_fn).__name__ == 'TPNetFunctionBackward'
    zr, ref, mags, restated = _reference(m, b, node_x, w)
    assert tr.rel_err(out, zr) < BAR and sorted(got) == sorted(ref) and len(ref) == 6 + (4 if variant != 'none' else 0) + 12 * L
    for n, r in ref.items():  # the restated chain is the autograd's
        assert (restated[n] - (torch.zeros_like(restated[n]) if r is None else r)).abs().max().item() <= 1e-9 * max(1.0, restated[n].abs().max().item()), n
    _check_bar(f'{variant} L={L} {how} {which}', got, ref, mags)


def _equal_grads(a, b, skip=()):
    for name in a:
        if skip and name.startswith(tuple(skip)):
            continue
        assert (a[name] is None) == (b[name] is None), name
        assert a[name] is None or _same_bits(a[name], b[name]), name


@pytest.mark.parametrize('variant,L', [('concat', 2), ('cross', 1), ('none', 0)])
def test_forward_bits_repeat_runs_and_py_mode(variant, L, monkeypatch):
    batches, node_x = _stream()
    for upto in (0, 3):
        b = batches[upto]
        m = _model(variant, L, upto=upto)
        w = _weight(2 * b.edge_src.numel(), m.output_dim)
        with torch.no_grad():
            plain = torch.cat(_call(m, b, node_x))
        out, ga = _device(m, b, node_x, w)
        assert _same_bits(out, plain)  # the grad-enabled forward is the inference call
        out_p, gp = _device(m, b, node_x, w, 'pairs')  # encode_pairs with row indices: the same computation
        assert _same_bits(out_p, plain)
        _equal_grads(ga, gp)
        _, ga2 = _device(m, b, node_x, w)
        _equal_grads(ga, ga2)
        monkeypatch.setenv('TGMX_TPNET_BWD', 'py')
        out_py, gpy = _device(m, b, node_x, w)
        monkeypatch.setenv('TGMX_TPNET_BWD', 'native')
        assert _same_bits(out_py, plain)
        _equal_grads(ga, gpy)
        m.eval()  # eval mode under gradients: the same
        out_eval, ge = _device(m, b, node_x, w)
        assert _same_bits(out_eval, plain)
        _equal_grads(ga, ge)


def _composed_spy(monkeypatch, m, took):
    orig = m._torch_forward
    monkeypatch.setattr(m, '_torch_forward', lambda a: took.append('composed') or orig(a))


def test_dispatch(monkeypatch):
    """Inside the envelope ``_torch_forward`` is not called and ``backward()`` is one ``tgmx_tpnet_backward``; every way out of the envelope
    composes, and returns gradients."""
    lib, _ = _lib()
    from tgm_amd.nn import _tpnet_train as tt

    monkeypatch.delenv('TGMX_TPNET_BWD')
    monkeypatch.setattr(tt, 'DEFAULT', 'native')
    calls, orig = [], lib.tgmx_tpnet_backward
    monkeypatch.setattr(lib, 'tgmx_tpnet_backward', lambda *a: calls.append(1) or orig(*a))
    batches, node_x = _stream()
    b = batches[3]
    m = _model('concat', 2)
    w = _weight(2 * b.edge_src.numel(), m.output_dim)
    took = []
    _composed_spy(monkeypatch, m, took)
    _, native = _device(m, b, node_x, w)
    assert took == [] and calls == [1]

    def composed(nx=node_x):
        took.clear()
        m.zero_grad(set_to_none=True)
        out = torch.cat(_call(m, b, nx))
        assert took == ['composed'] and out.requires_grad and type(out.grad_fn).__name__ != 'TPNetFunctionBackward'
        (out.float() * w.to(DEV)).sum().backward()
        assert m.projection_layer[0].weight.grad is not None and calls == [1]

    composed(node_x.clone().requires_grad_(True))
    monkeypatch.setenv('TGMX_TPNET_BWD', 'torch')
    composed()
    monkeypatch.delenv('TGMX_TPNET_BWD')
    took.clear()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        try:
            _call(m, b, node_x)
        except RuntimeError:  # (what the composed path makes of autocast is its own business, unchanged here)
            pass
    assert took == ['composed']
    _, again = _device(m, b, node_x, w)  # the module is intact after the composed calls
    assert calls == [1, 1]
    _equal_grads(native, again)


def test_needs_input_grad_is_honoured(monkeypatch):
    """Frozen time encoder, pair MLP and single layers: their ``.grad`` stays None, the others keep their bits, and the launches that feed
    only the frozen ones are not issued (counted in py mode, whose launch list is the native call's)."""
    lib, _ = _lib()
    batches, node_x = _stream()
    b = batches[3]
    m = _model('concat', 2)
    w = _weight(2 * b.edge_src.numel(), m.output_dim)
    _, full = _device(m, b, node_x, w)
    counts = {}
    for fn in ('tgmx_tpnet_time_backward', 'tgmx_tpnet_token_backward', 'tgmx_relu_mask', 'tgmx_sgemm_tn', 'tgmx_tpnet_mean_backward'):
        orig = getattr(lib, fn)
        monkeypatch.setattr(lib, fn, (lambda f, o: lambda *a: counts.__setitem__(f, counts.get(f, 0) + 1) or o(*a))(fn, orig))

    def run(frozen):
        for n, p in _trainable(m).items():
            p.requires_grad_(not n.startswith(frozen))
        counts.clear()
        monkeypatch.setenv('TGMX_TPNET_BWD', 'py')
        _, part = _device(m, b, node_x, w)
        monkeypatch.setenv('TGMX_TPNET_BWD', 'native')
        _, nat_part = _device(m, b, node_x, w)
        _equal_grads(part, nat_part)
        assert all((part[k] is None) == k.startswith(frozen) for k in part), frozen
        _equal_grads(full, part, skip=frozen)
        return dict(counts)

    everything = run(('no such prefix',))
    assert everything == {'tgmx_tpnet_mean_backward': 1, 'tgmx_tpnet_token_backward': 2, 'tgmx_relu_mask': 2, 'tgmx_tpnet_time_backward': 1,
                          'tgmx_sgemm_tn': 2 * 2 + 2 + 2}  # fmt: skip
    no_time = run(('time_encoder',))
    assert 'tgmx_tpnet_time_backward' not in no_time and no_time['tgmx_relu_mask'] == 2
    no_rp = run(('random_projections',))
    assert no_rp['tgmx_relu_mask'] == 1 and no_rp['tgmx_sgemm_tn'] == 2 * 2 + 2 and no_rp['tgmx_tpnet_time_backward'] == 1
    for frozen in ('mlp_mixers.1', 'mlp_mixers.0', 'projection_layer'):
        run((frozen,))
    # only the last layer's channel block trains: nothing below it runs
    for n, p in _trainable(m).items():
        p.requires_grad_(n.startswith('mlp_mixers.1.channel'))
    counts.clear()
    monkeypatch.setenv('TGMX_TPNET_BWD', 'py')
    _, top = _device(m, b, node_x, w)
    assert 'tgmx_tpnet_token_backward' not in counts and 'tgmx_relu_mask' not in counts and counts['tgmx_sgemm_tn'] == 2
    assert all((top[k] is None) != k.startswith('mlp_mixers.1.channel') for k in top)
    _equal_grads({k: v for k, v in full.items() if k.startswith('mlp_mixers.1.channel')}, {k: v for k, v in top.items() if k.startswith('mlp_mixers.1.channel')})


def test_call_sharing_across_an_optimizer_step():
    """Forward A, SGD step, forward B, backward B, backward A: A's gradients are those of the run without B in between -- and those of
    A's own weights (forward A, backward A), because the call keeps the weights it ran with."""
    batches, node_x = _stream()
    m0 = _model('concat', 2)
    bA, bB = batches[3], batches[5]
    wA, wB = _weight(2 * bA.edge_src.numel(), 10).to(DEV), _weight(2 * bB.edge_src.numel(), 10, seed=8).to(DEV)

    def run(with_b, step=True):
        m = copy.deepcopy(m0)
        params = list(_trainable(m).values())
        opt = torch.optim.SGD(params, lr=0.05)
        for p in params:
            p.grad = torch.full_like(p, 0.3)
        out_a = torch.cat(_call(m, bA, node_x))
        if step:
            opt.step()
        if with_b:
            out_b = torch.cat(_call(m, bB, node_x))
            torch.autograd.grad((out_b * wB).sum(), params)
        return torch.autograd.grad((out_a * wA).sum(), params)

    with_b, without_b, own = run(True), run(False), run(False, step=False)
    for x, y, z in zip(with_b, without_b, own):
        assert _same_bits(x, y) and _same_bits(x, z)


def test_inputs_overwritten_between_forward_and_backward():
    """The sampler's outputs are pooled and rewritten by the next batch: the backward reads none of the caller's tensors."""
    batches, node_x = _stream()
    b = batches[3]
    m = _model('concat', 2)
    w = _weight(2 * b.edge_src.numel(), m.output_dim)
    _, want = _device(m, b, node_x, w)
    m.zero_grad(set_to_none=True)
    nids, nt, nx = (t.clone() for t in gathered(b, *pair_rows(b, True)))
    ei, t, x = torch.stack([b.edge_src, b.neg]), b.edge_time.clone(), node_x.clone()
    out = torch.cat(m(x, ei, t, nids, nt, nx))
    nids.fill_(-1), nt.zero_(), nx.fill_(float('nan')), ei.zero_(), t.zero_(), x.fill_(float('nan'))
    (out * w.to(DEV)).sum().backward()
    _equal_grads(want, {n: p.grad for n, p in _trainable(m).items()})


# ---- dropout ----------------------------------------------------------------------------------------------------------------------------------------
def _masks_of(m, Q):
    """The masks of the forward call the module has just made."""
    first = m.__dict__['_tgmx_drop_calls'] * 64
    mx = m.mlp_mixers[0]
    return [br.layer_masks(m.dropout, torch.initial_seed(), first, l, Q, m.num_neighbors, m.output_dim, mx.token_feedforward.ffn[0].out_features,
                           mx.channel_feedforward.ffn[0].out_features) for l in range(m.num_layers)]  # fmt: skip


@pytest.mark.parametrize('variant', ['concat', 'cross'])
def test_dropout_matches_the_restatement_with_the_regenerated_masks(variant):
    batches, node_x = _stream()
    b = batches[3]
    m = _model(variant, 2, dropout=0.5)
    Q = 2 * b.edge_src.numel()
    w = _weight(Q, m.output_dim)
    out, got = _device(m, b, node_x, w)
    zr, ref, mags, _ = _reference(m, b, node_x, w, masks=_masks_of(m, Q))
    assert tr.rel_err(out, zr) < BAR
    _check_bar(f'dropout {variant}', got, ref, mags)
    out2, got2 = _device(m, b, node_x, w)  # another call, other masks
    assert not torch.equal(out, out2)
    zr2, ref2, mags2, _ = _reference(m, b, node_x, w, masks=_masks_of(m, Q))
    assert tr.rel_err(out2, zr2) < BAR
    _check_bar(f'dropout {variant} second call', got2, ref2, mags2)
    m.eval()  # eval mode is untouched: no masks, the inference call's bits
    with torch.no_grad():
        plain = torch.cat(_call(m, b, node_x))
    calls = m.__dict__['_tgmx_drop_calls']
    out_eval, _ = _device(m, b, node_x, w)
    assert _same_bits(out_eval, plain) and m.__dict__['_tgmx_drop_calls'] == calls


# ---- the reference's recorded float32 gradients ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['small', 'small_norp', 'small_cross', 'single', 'padheavy'])
def test_reference_gradient_fixtures(name):
    """``g32_tpnet_grad_*``: the reference's ``TPNet`` under float32 autograd on the g17 inputs.  The native gradients are held to the bar
    against the float64 restatement; their error over the reference's recorded float32 error is printed, not asserted."""
    import json
    import os

    from golden_util import GOLDEN_DIR, load
    from test_tpnet_cpu import build_model, encoder_inputs, fixture_state_dict, rp_dict

    meta, a = load(f'g17_tpnet_enc_{name}')
    gmeta, rec = load(f'g32_tpnet_grad_{name}')
    assert gmeta['inputs'] == f'g17_tpnet_enc_{name}'
    noise = json.load(open(os.path.join(GOLDEN_DIR, 'g32_tpnet_grad_noise.json')))[name]
    sd = fixture_state_dict(meta, a)
    m = build_model(meta)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    i = {k: v.to(DEV) for k, v in encoder_inputs(a).items()}
    dout = torch.from_numpy(rec['dout'])
    zs, zd = m(i['node_x'], torch.stack([i['src'], i['dst']]), i['edge_time'], i['nbr_nids'], i['nbr_time'], i['nbr_edge_x'])
    assert type(zs.grad_fn).__name__ == 'TPNetFunctionBackward'
    torch.cat([zs, zd]).backward(dout.to(DEV))
    train = lambda n: n.split('.')[-1] in ('weight', 'bias')
    leaf = {n: (v.double().requires_grad_(True) if train(n) else (v.double() if v.is_floating_point() else v)) for n, v in sd.items()}
    h = encoder_inputs(a)
    pos = (h['node_x'], h['src'], h['dst'], h['edge_time'], h['nbr_nids'], h['nbr_time'], h['nbr_edge_x'])
    L, rpd = meta['dims']['num_layers'], rp_dict(meta['cfg'])
    (torch.cat(br.forward(leaf, L, rpd, *pos)) * dout.double()).sum().backward()
    plain = {n: v.double() if v.is_floating_point() else v for n, v in sd.items()}
    keep, mags = {}, {}
    br.forward(plain, L, rpd, *pos, keep=keep)
    dims = dict(dN=meta['dims']['node_feat_dim'], dT=meta['dims']['time_feat_dim'], dE=meta['dims']['edge_x_dim'], od=0 if m.random_projections is None else m.random_projections.out_dim)
    br.backward(plain, L, dims, keep, dout, mags=mags)
    got = {n: p.grad for n, p in _trainable(m).items()}
    ref = {n: leaf[n].grad for n in got}
    assert sorted('g.' + n for n in got) == sorted(k for k in rec if k.startswith('g.'))
    _check_bar(f'fixture {name}', got, ref, mags)
    ratios = []
    for n, r in ref.items():
        scale = float(r.abs().max())
        if scale > 0 and noise[n] > 0:
            ratios.append(float((got[n].cpu().double() - r).abs().max()) / scale / noise[n])
    print(f'tpnet train fixture {name}: native error over the reference float32 error {min(ratios):.2f} .. {max(ratios):.2f} (reference worst {max(noise.values()):.3e})')
