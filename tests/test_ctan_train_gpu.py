"""CTAN's native training path on the device (``tgm_amd/nn/_ctan_train.py``, ``csrc/ctan_bwd.hip``).

The kernels alone, through ctypes, against the float64 restatement of ``tests/ctan_bwd_restate.py``: outputs pre-filled with NaN inside
``Buf`` allocations whose sentinel columns and tail must stay intact, every case launched twice and compared bit for bit, and the assertion
err / bound <= 1 with bound = chain * 2^-24 * magnitude (``pytest -rP`` prints the worst ratio).  Shapes: U = 40, every width class (one
column a lane, two with a tail, three, four with vector loads) and the segment lengths 0, 1, 16 | 17 (the one-wave limit), 64 | 65 (a wave's
block), a hub of 1 500 -- as in-degrees for the target pass and as out-degrees for the source pass.

End to end against float64 autograd through ``ctan_restate.ctan_forward`` at the project's bar for this model (each gradient within 2e-4 of
its largest entry; ``lin_key.bias``, whose exact gradient is 0, scaled by ``lin_query.bias``'s gradient, as tests/test_ctan_gpu.py does), then
bit equality with the no-grad forward, call sharing, repeat runs and the dispatch.
"""
import functools

import pytest
import torch

import ctan_bwd_restate as br
import ctan_restate as cr
from oracle.tgat_bwd_ref import EPS
from test_ctan_gpu import make_case
from test_tgat_bwd_blocks_gpu import Buf, _report, _same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BAR = 2e-4
NAN = float('nan')


def _lib():
    from tgm_amd import _native

    return _native.load(), _native


def dev(v):
    return v.to(DEV)


def _all_nan(t):
    return bool(torch.isnan(t).all())


# ---- the kernels alone ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _target_case(C):
    c = br.kernel_case(C)
    want = br.target_pass(c['q'], c['k'], c['v'], c['h4'], c['ep'], c['src'], c['tgt'], c['gx'], c['scale'], c['eps'])
    order, lo, hi = br.grouped(c['tgt'], c['U'])
    return c, want, (order, lo, hi)


def _launch_target(c, groups, accumulate):
    lib, nat = _lib()
    U, C, E = c['U'], c['C'], c['E']
    ins = {n: Buf(c[n].shape[0], C, data=dev(c[n]), fill=0.0) for n in ('q', 'k', 'v', 'h4', 'ep', 'gx')}
    order, lo, hi = (dev(t).contiguous() for t in groups)
    src = dev(c['src']).contiguous()
    d4, alpha, s = Buf(U, 4 * C), Buf(1, E), Buf(1, E)
    etgt = torch.full((E + 64,), -7, dtype=torch.int32, device=DEV)
    de = Buf(E, C, data=dev(c['de_old']) if accumulate else None)
    nat.check(lib.tgmx_ctan_attend_backward(ins['q'].ptr, ins['k'].ptr, ins['v'].ptr, ins['h4'].ptr, ins['ep'].ptr, order.data_ptr(), src.data_ptr(),
                                            lo.data_ptr(), hi.data_ptr(), U, C, c['scale'], c['eps'], ins['gx'].ptr, d4.ptr, alpha.ptr, s.ptr,
                                            etgt.data_ptr(), de.ptr, accumulate, nat.stream_ptr()), 'tgmx_ctan_attend_backward')  # fmt: skip
    torch.cuda.synchronize()
    return d4, alpha, s, etgt, de


@pytest.mark.parametrize('accumulate', [0, 1], ids=['store', 'add'])
@pytest.mark.parametrize('C', br.WIDTHS)
def test_target_pass_alone(C, accumulate):
    c, want, groups = _target_case(C)
    U, E = c['U'], c['E']
    d4, alpha, s, etgt, de = _launch_target(c, groups, accumulate)
    again = _launch_target(c, groups, accumulate)
    for a, b in zip((d4, alpha, s, de), (again[0], again[1], again[2], again[4])):
        assert _same_bits(a.flat, b.flat)
    assert torch.equal(etgt, again[3])
    for b in (d4, alpha, s, de):
        assert b.sentinels_intact()
    assert _all_nan(d4.view[:, C:3 * C])  # the source pass's columns are not this kernel's
    assert torch.equal(etgt[:E].cpu(), c['tgt'].to(torch.int32)) and bool((etgt[E:] == -7).all())
    chain = br.attend_chain(C, c['in_deg']).double()
    row, edge = (chain * EPS)[:, None], (chain[c['tgt']] * EPS)
    worst = [_report(f'target C={C} dz', d4.view[:, 3 * C:].contiguous(), want['dz'], row * want['dz_m']),
             _report(f'target C={C} dq', d4.view[:, :C].contiguous(), want['dq'], row * want['dq_m']),
             _report(f'target C={C} alpha', alpha.view[0], want['alpha'], edge * want['alpha_m']),
             _report(f'target C={C} s', s.view[0], want['s'], edge * want['s_m'])]  # fmt: skip
    if accumulate:
        old = c['de_old'].double()
        worst.append(_report(f'target C={C} d_eproj (add)', de.view, old + want['de'], (edge + EPS)[:, None] * (want['de_m'] + old.abs())))
    else:
        worst.append(_report(f'target C={C} d_eproj (store)', de.view, want['de'], edge[:, None] * want['de_m']))
    assert max(worst) <= 1.0, worst
    no_edges = (c['in_deg'] == 0).nonzero().flatten()
    assert no_edges.numel() and not d4.view[dev(no_edges), :C].any()  # dq = 0 exactly


def test_target_pass_without_a_d_eproj_and_without_edges():
    """d_eproj NULL: the other outputs keep their bits.  seg_lo NULL: no edges at all, dq = 0 and dz from z = h4."""
    lib, nat = _lib()
    c, want, groups = _target_case(100)
    full = _launch_target(c, groups, 0)
    U, C, E = c['U'], c['C'], c['E']
    ins = {n: dev(c[n]).contiguous() for n in ('q', 'k', 'v', 'h4', 'ep', 'gx')}
    order, lo, hi = (dev(t).contiguous() for t in groups)
    src = dev(c['src']).contiguous()
    d4, alpha, s = Buf(U, 4 * C), Buf(1, E), Buf(1, E)
    etgt = torch.zeros(E, dtype=torch.int32, device=DEV)
    nat.check(lib.tgmx_ctan_attend_backward(ins['q'].data_ptr(), ins['k'].data_ptr(), ins['v'].data_ptr(), ins['h4'].data_ptr(), ins['ep'].data_ptr(),
                                            order.data_ptr(), src.data_ptr(), lo.data_ptr(), hi.data_ptr(), U, C, c['scale'], c['eps'], ins['gx'].data_ptr(),
                                            d4.ptr, alpha.ptr, s.ptr, etgt.data_ptr(), None, 0, nat.stream_ptr()), 'tgmx_ctan_attend_backward')  # fmt: skip
    assert _same_bits(d4.flat, full[0].flat) and _same_bits(alpha.flat, full[1].flat) and _same_bits(s.flat, full[2].flat)
    d0 = Buf(U, 4 * C)
    nat.check(lib.tgmx_ctan_attend_backward(ins['q'].data_ptr(), None, None, ins['h4'].data_ptr(), None, None, None, None, None, U, C, c['scale'], c['eps'],
                                            ins['gx'].data_ptr(), d0.ptr, None, None, None, None, 0, nat.stream_ptr()), 'tgmx_ctan_attend_backward')  # fmt: skip
    assert d0.sentinels_intact() and not d0.view[:, :C].any() and _all_nan(d0.view[:, C:3 * C])
    tz = torch.tanh(c['h4'].double())
    dz, dz_m = c['eps'] * c['gx'].double() * (1 - tz * tz), c['eps'] * c['gx'].double().abs() * (1 + tz * tz)
    assert _report('target no edges dz', d0.view[:, 3 * C:].contiguous(), dz, br.attend_chain(C, 0) * EPS * dz_m) <= 1.0


@functools.lru_cache(maxsize=None)
def _source_case(C):
    c = br.kernel_case(C, seed=1)
    g = torch.Generator().manual_seed(C)
    c['dz'], c['alpha'], c['s'] = torch.randn(c['U'], C, generator=g), torch.rand(c['E'], generator=g), torch.randn(c['E'], generator=g)
    want = br.source_pass(c['q'], c['dz'], c['src'], c['tgt'], c['alpha'], c['s'])
    return c, want, br.grouped(c['src'], c['U'])


def _launch_source(c, groups):
    lib, nat = _lib()
    U, C, E = c['U'], c['C'], c['E']
    q = Buf(U, C, data=dev(c['q']), fill=0.0)
    d4 = Buf(U, 4 * C)
    d4.view[:, 3 * C:] = dev(c['dz'])
    order, lo, hi = (dev(t).contiguous() for t in groups)
    etgt, alpha, s = dev(c['tgt']).to(torch.int32).contiguous(), dev(c['alpha']).contiguous(), dev(c['s']).contiguous()
    nat.check(lib.tgmx_ctan_source_backward(q.ptr, d4.ptr, order.data_ptr(), etgt.data_ptr(), lo.data_ptr(), hi.data_ptr(), alpha.data_ptr(), s.data_ptr(),
                                            U, C, nat.stream_ptr()), 'tgmx_ctan_source_backward')  # fmt: skip
    torch.cuda.synchronize()
    return d4


@pytest.mark.parametrize('C', br.WIDTHS)
def test_source_pass_alone(C):
    c, want, groups = _source_case(C)
    d4, again = _launch_source(c, groups), _launch_source(c, groups)
    assert _same_bits(d4.flat, again.flat) and d4.sentinels_intact()
    assert _all_nan(d4.view[:, :C]) and torch.equal(d4.view[:, 3 * C:].cpu(), c['dz'])  # dq is the target pass's, dz is only read
    bound = (br.source_chain(c['out_deg']).double() * EPS)[:, None]
    worst = [_report(f'source C={C} dk', d4.view[:, C:2 * C].contiguous(), want['dk'], bound * want['dk_m']),
             _report(f'source C={C} dv', d4.view[:, 2 * C:3 * C].contiguous(), want['dv'], bound * want['dv_m'])]  # fmt: skip
    assert max(worst) <= 1.0, worst
    none = (c['out_deg'] == 0).nonzero().flatten()
    assert none.numel() and not d4.view[dev(none), C:3 * C].any()  # zero rows, written


def test_source_pass_without_edges():
    lib, nat = _lib()
    U, C = 7, 130
    d4 = Buf(U, 4 * C)
    nat.check(lib.tgmx_ctan_source_backward(None, d4.ptr, None, None, None, None, None, None, U, C, nat.stream_ptr()), 'tgmx_ctan_source_backward')
    assert d4.sentinels_intact() and not d4.view[:, C:3 * C].any() and _all_nan(d4.view[:, :C]) and _all_nan(d4.view[:, 3 * C:])


@pytest.mark.parametrize('E,T,U', [(1, 1, 1), (300, 5, 40), (777, 64, 13)])
def test_edge_attr_backward_alone(E, T, U):
    lib, nat = _lib()
    g = torch.Generator().manual_seed(E + T)
    base, mean, std = 1_700_000_000, 300.5, 450.25
    lu, t = base + torch.randint(0, 2000, (U,), generator=g), base + torch.randint(0, 2000, (E,), generator=g)
    src = torch.randint(0, U, (E,), generator=g)
    tw, tb, d_attr = torch.randn(T, generator=g), torch.randn(T, generator=g), torch.randn(E, T, generator=g)
    assert (lu[src] > t).any() or E == 1
    want, mag = br.edge_attr_backward(br.rel_time(lu, src, t, mean, std), tw, tb, d_attr)
    outs = []
    lu_d, src_d, t_d, tw_d, tb_d = (dev(v).contiguous() for v in (lu, src, t, tw, tb))
    for _ in range(2):
        d, part = Buf(E, T, ld=T + 3, lead=1, data=dev(d_attr), fill=0.0), Buf(E, 2 * T)
        nat.check(lib.tgmx_ctan_edge_attr_backward(lu_d.data_ptr(), src_d.data_ptr(), t_d.data_ptr(), tw_d.data_ptr(), tb_d.data_ptr(), d.ptr, d.ld, T, E,
                                                   mean, std, part.ptr, nat.stream_ptr()), 'tgmx_ctan_edge_attr_backward')  # fmt: skip
        torch.cuda.synchronize()
        outs.append(part)
    assert _same_bits(outs[0].flat, outs[1].flat) and outs[0].sentinels_intact()
    assert _report(f'edge_attr E={E} T={T}', outs[0].view, want, br.edge_attr_chain() * EPS * mag) <= 1.0


@pytest.mark.parametrize('M', [1, 5, 256])
def test_antisym_grad_alone(M):
    lib, nat = _lib()
    dA = torch.randn(M, M, generator=torch.Generator().manual_seed(M))
    want, mag = br.antisym_grad(dA)
    outs, dA_d = [], dev(dA).contiguous()
    for _ in range(2):
        out = Buf(M, M)
        nat.check(lib.tgmx_ctan_antisym_grad(dA_d.data_ptr(), M, out.ptr, nat.stream_ptr()), 'tgmx_ctan_antisym_grad')
        torch.cuda.synchronize()
        outs.append(out)
    assert _same_bits(outs[0].flat, outs[1].flat) and outs[0].sentinels_intact()
    assert _report(f'antisym M={M}', outs[0].view, want, br.antisym_chain() * EPS * mag) <= 1.0
    assert not torch.diagonal(outs[0].view).any()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
def _reference(enc, args, cfg, weight, dtype=torch.float64):
    p = {k: v.detach().cpu().to(dtype).requires_grad_(k in cr.PARAMS) for k, v in enc.state_dict().items()}
    x = args[0].detach().clone().to(dtype).requires_grad_(True)  # (a copy: the case's own tensor stays a plain leaf)
    (cr.ctan_forward(p, x, *args[1:], dtype=dtype, **cfg) * weight.to(dtype)).sum().backward()
    grads = {k: p[k].grad for k in cr.PARAMS}
    grads['node_x'] = x.grad
    return grads


def _device(enc, args, weight, x_grad=True, edge_index=None):
    """One forward and backward on the device: (out, name -> gradient)."""
    enc = enc.to(DEV).train()
    enc.zero_grad(set_to_none=True)
    x = dev(args[0]).requires_grad_(x_grad)
    out = enc(x, dev(args[1]), dev(args[2]) if edge_index is None else edge_index, dev(args[3]), dev(args[4]))
    (out * dev(weight)).sum().backward()
    enc.check()
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in enc.named_parameters()}
    grads['node_x'] = x.grad
    return out.detach(), grads


def _magnitudes(enc, args, cfg, weight):
    """(name -> the restated gradient's MAGNITUDE, the same sums over absolute values: the size of the terms that make the gradient up,
    whether or not they cancel;  the whole backward's chain for this case)."""
    p = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
    sv = br.forward_saved(p, *[a.detach() for a in args], **cfg)
    E = sv['src'].numel()
    longest = lambda ids: int(torch.bincount(ids).max()) if E else 0
    chain = br.backward_chain(args[0].shape[0], E, sv['out'].shape[1], args[0].shape[1], sv['edge_attr'].shape[1], cfg['num_iters'],
                              longest(sv['tgt']), longest(sv['src']))  # fmt: skip
    return {k: m for k, (_, m) in br.backward(sv, weight).items()}, chain


def _check_bar(label, got, ref, f32=None, mags=None):
    """Every gradient within BAR of its largest entry.  A gradient that is exactly 0 because its terms cancel has no such scale (float64
    autograd leaves 0 or ~1e-17 of it): ``lin_key.bias`` always (scaled by ``lin_query.bias``'s gradient, as tests/test_ctan_gpu.py does), and
    at degenerate graphs others too -- one edge (alpha = 1, so s = dalpha - delta = 0 and with it dq, dk) or every edge between the same
    two nodes (sum_e s_e = 0 in dk).  Where the reference's largest entry is below 1e-12 of the largest entry of the restated MAGNITUDE
    (``mags``: the size of the cancelling terms), that magnitude is the scale, and every entry must also lie within the restatement's own
    rounding bound of the reference, chain * 2^-24 * magnitude, entry by entry; where the magnitude is 0 too no path reaches the gradient
    (num_iters = 0, no edges) and it must be exactly 0."""
    worst, mag = 0.0, None
    for name, r in ref.items():
        g = got[name]
        assert g is not None and g.dtype == torch.float32 and torch.isfinite(g).all(), (label, name)
        r = torch.zeros(g.shape, dtype=torch.float64) if r is None else r
        scale = r.abs().max().item()
        if name == 'aconv.phi.lin_key.bias':
            q = ref['aconv.phi.lin_query.bias']
            scale = 0.0 if q is None else q.abs().max().item()
            r = torch.zeros_like(r)  # its exact gradient
        dist = (g.cpu().double() - r).abs().max().item()
        if mags is not None:
            mag = mags() if mag is None else mag
            m, chain = mag[0][name], mag[1]
            if scale <= 1e-12 * float(m.max()):
                scale = float(m.max())
                assert ((g.cpu().double() - r).abs() <= chain * EPS * m).all(), (label, name, 'outside chain * EPS * magnitude')
        if scale == 0.0:  # no path reaches it (num_iters = 0, no edges): exactly zero
            assert dist == 0.0, (label, name, dist)
            continue
        err = dist / scale
        line = f'ctan train {label} {name}: {err:.3e}'
        if f32 is not None and f32[name] is not None and name != 'aconv.phi.lin_key.bias':
            d32 = (f32[name].double() - r).abs().max().item() / scale
            line += f' (float32 autograd on the CPU {d32:.3e}, ratio {err / max(d32, 1e-30):.2f})'
        print(line)
        worst = max(worst, err)
        assert err <= BAR, (label, name, err)
    return worst


def _weight(U, M, seed=7):
    return torch.randn(U, M, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('num_iters', [0, 1, 3])
@pytest.mark.parametrize('M', [5, 256])
def test_gradients_match_float64_autograd(M, num_iters):
    enc, args, cfg = make_case(200 + M + num_iters, 40, M, 6, 9, 2, num_iters, E=300)
    w = _weight(40, M)
    ref, f32 = _reference(enc, args, cfg, w), _reference(enc, args, cfg, w, torch.float32)
    _, got = _device(enc, args, w)
    assert sorted(got) == sorted(ref)
    _check_bar(f'M={M} iters={num_iters}', got, ref, f32)


def test_gradients_with_a_hub():
    enc, args, cfg = make_case(231, 40, 256, 8, 12, 1, 2, seg_lens=br.SEG_LENS)
    w = _weight(40, 256)
    _, got = _device(enc, args, w)
    _check_bar('hub M=256', got, _reference(enc, args, cfg, w))


@pytest.mark.parametrize('U,E', [(1, 0), (1, 5), (7, 0), (33, 1)])
def test_gradients_with_no_edges_and_one_node(U, E):
    enc, args, cfg = make_case(250 + U, U, 12, 4, 3, 1, 2, E=E)
    w = _weight(U, 12)
    _, got = _device(enc, args, w)
    _check_bar(f'U={U} E={E}', got, _reference(enc, args, cfg, w), mags=lambda: _magnitudes(enc, args, cfg, w))


def _equal_grads(a, b, skip=()):
    for name in a:
        if name in skip:
            continue
        assert (a[name] is None) == (b[name] is None), name
        assert a[name] is None or _same_bits(a[name], b[name]), name


def test_needs_input_grad_is_honoured():
    """node_x without a gradient (the example's case: memory is a buffer) and a frozen time encoder: those gradients are None, the others
    keep their bits."""
    enc, args, cfg = make_case(260, 40, 100, 6, 9, 2, 2, E=300)
    w = _weight(40, 100)
    _, full = _device(enc, args, w)
    _, no_x = _device(enc, args, w, x_grad=False)
    assert no_x['node_x'] is None
    _equal_grads(full, no_x, skip=('node_x',))
    for p in enc.time_enc.parameters():
        p.requires_grad_(False)
    _, frozen = _device(enc, args, w)
    time = ('time_enc.lin.weight', 'time_enc.lin.bias')
    assert all(frozen[k] is None for k in time)
    _equal_grads(full, frozen, skip=time)


def test_edge_index_dtypes_and_out_of_range_entries():
    enc, args, cfg = make_case(270, 40, 64, 6, 9, 2, 2, E=300)
    w = _weight(40, 64)
    _, base = _device(enc, args, w)
    _, g32 = _device(enc, args, w, edge_index=dev(args[2]).to(torch.int32))
    wide = torch.zeros(2, 600, dtype=torch.int64, device=DEV)
    wide[:, ::2] = dev(args[2])
    assert not wide[:, ::2].is_contiguous()
    _, gnc = _device(enc, args, w, edge_index=wide[:, ::2])
    _equal_grads(base, g32)
    _equal_grads(base, gnc)
    # out of range: clamped and reported; the gradients are those of the clamped graph
    bad = args[2].clone()
    bad[0, 3], bad[1, 5] = 40, -2
    enc = enc.to(DEV).train()
    enc.zero_grad(set_to_none=True)
    out = enc(dev(args[0]), dev(args[1]), dev(bad), dev(args[3]), dev(args[4]))
    (out * dev(w)).sum().backward()
    with pytest.raises(ValueError, match='outside'):
        enc.check()
    got = {k: p.grad for k, p in enc.named_parameters()}
    clamped = (args[0], args[1], bad.clamp(0, 39), args[3], args[4])
    ref = _reference(enc, clamped, cfg, w)
    ref.pop('node_x')
    _check_bar('clamped', got, ref)


def test_forward_bits_call_sharing_and_repeat_runs():
    enc, args, cfg = make_case(280, 40, 256, 16, 20, 1, 3, E=700)
    w = _weight(40, 256)
    enc = enc.to(DEV).train()
    with torch.no_grad():
        plain = enc(*[dev(a) for a in args])
    out, ga = _device(enc, args, w)
    assert 'CtanFunction' in type(enc(*[dev(a) for a in args]).grad_fn).__name__
    assert _same_bits(out, plain)  # the grad-enabled forward is the inference call
    _, ga2 = _device(enc, args, w)
    _equal_grads(ga, ga2)  # two runs, the same bits
    # another input through the same module before ONE backward: nothing saved is shared
    enc_b, args_b, _ = make_case(281, 40, 256, 16, 20, 1, 3, E=500)
    _, gb = _device(enc, args_b, w)
    enc.zero_grad(set_to_none=True)
    xa, xb = dev(args[0]).requires_grad_(True), dev(args_b[0]).requires_grad_(True)
    oa = enc(xa, *[dev(a) for a in args[1:]])
    ob = enc(xb, *[dev(a) for a in args_b[1:]])
    ((oa * dev(w)).sum() + (ob * dev(w)).sum()).backward()
    assert _same_bits(xa.grad, ga['node_x']) and _same_bits(xb.grad, gb['node_x'])
    for name, p in enc.named_parameters():
        assert _same_bits(p.grad, ga[name] + gb[name]), name


PY_CASES = {
    'no iterations': dict(num_iters=0, E=300),
    'no edges': dict(num_iters=2, E=0),
    'node_x a buffer': dict(num_iters=2, E=300, x_grad=False),
    'time_enc frozen': dict(num_iters=2, E=300, frozen=('time_enc',)),
    'edge side frozen, node_x a buffer': dict(num_iters=3, E=300, x_grad=False, frozen=('time_enc', 'aconv.phi.lin_edge')),
    'enc_x frozen, node_x a buffer': dict(num_iters=2, E=300, x_grad=False, frozen=('enc_x',)),
}


@pytest.mark.parametrize('case', list(PY_CASES))
def test_py_mode_gives_the_one_calls_bits(case, monkeypatch):
    """``backward_per_launch`` is the readable specification: the same bits as the one call in the branches the full case does not reach
    -- the zeroed gradients of ``num_iters = 0`` and ``E = 0``, no ``d_eproj`` wanted, no ``d_node_x``, frozen parameters, and the
    projection skipped at the first iteration when nobody reads the gradient at ``enc_x``'s output."""
    c = PY_CASES[case]
    enc, args, cfg = make_case(300 + len(case), 40, 100, 6, 9, 2, c['num_iters'], E=c['E'])
    w = _weight(40, 100)
    for name, p in enc.named_parameters():
        if name.startswith(c.get('frozen', ())) and c.get('frozen'):
            p.requires_grad_(False)
    monkeypatch.delenv('TGMX_CTAN_BWD', raising=False)
    _, native = _device(enc, args, w, x_grad=c.get('x_grad', True))
    monkeypatch.setenv('TGMX_CTAN_BWD', 'py')
    _, py = _device(enc, args, w, x_grad=c.get('x_grad', True))
    frozen = [k for k, g in native.items() if g is None]
    assert sorted(frozen) == sorted(k for k in native if (k == 'node_x' and not c.get('x_grad', True)) or (c.get('frozen') and k.startswith(c['frozen'])))
    _equal_grads(native, py)
    ref = _reference(enc, args, cfg, w)
    _check_bar(f'py {case}', {k: g for k, g in py.items() if g is not None}, {k: r for k, r in ref.items() if py[k] is not None})


def test_dispatch(monkeypatch):
    """One ``tgmx_ctan_backward`` per ``backward()`` inside the envelope; none at M = 260, under autocast or with TGMX_CTAN_BWD=torch / py; the
    gradients within the bar on every path that returns, and py with the one call's bits.  Under autocast the call is outside the envelope
    and goes to ``forward_composed``, which does not run under autocast: its ``index_add_`` meets a reduced-precision accumulator and a
    float32 source and raises (as it did before the native training path existed: that path is unchanged).  The test runs the real call
    and asserts that, with no native backward counted."""
    lib, _ = _lib()
    calls, orig = [], lib.tgmx_ctan_backward
    monkeypatch.setattr(lib, 'tgmx_ctan_backward', lambda *a: calls.append(1) or orig(*a))
    monkeypatch.delenv('TGMX_CTAN_BWD', raising=False)
    enc, args, cfg = make_case(290, 30, 8, 4, 5, 2, 2, E=200)
    w = _weight(30, 8)
    ref = _reference(enc, args, cfg, w)
    _, native = _device(enc, args, w)
    assert calls == [1]
    _check_bar('native', native, ref)
    _device(enc, args, w)
    assert calls == [1, 1]
    monkeypatch.setenv('TGMX_CTAN_BWD', 'py')
    _, py = _device(enc, args, w)
    assert calls == [1, 1]
    _equal_grads(native, py)
    monkeypatch.setenv('TGMX_CTAN_BWD', 'torch')
    _, composed = _device(enc, args, w)
    assert calls == [1, 1]
    _check_bar('torch', composed, ref)
    monkeypatch.delenv('TGMX_CTAN_BWD')
    for dtype in (torch.bfloat16, torch.float16):
        with torch.autocast('cuda', dtype=dtype), pytest.raises(RuntimeError, match='same scalar type'):
            enc(*[dev(a) for a in args])
    assert calls == [1, 1]
    _, after = _device(enc, args, w)  # the module is intact after the refused calls
    assert calls == [1, 1, 1]
    _equal_grads(native, after)
    calls.clear()
    wide, wargs, wcfg = make_case(291, 20, 260, 4, 5, 2, 1, E=100)
    ww = _weight(20, 260)
    _, gw = _device(wide, wargs, ww)
    assert calls == []
    _check_bar('M=260', gw, _reference(wide, wargs, wcfg, ww))
