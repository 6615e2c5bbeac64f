"""GCLSTM / ChebConv training on the device against the float64 restatement (tests/gclstm_bwd_restate.py, tests/gclstm_restate.py): the gate
backward, the transposed Laplacian and the Clenshaw pass alone through ctypes, then ``loss.backward()`` through ``GCLSTM`` / ``ChebConv``
against float64 autograd, and the dispatch (``TGMX_GCLSTM_BWD``).

The kernel tests follow tests/test_decoder_train_gpu.py: outputs pre-filled with NaN inside allocations with sentinel columns and a
sentinel tail that must stay intact, every case launched twice and compared bit for bit.  Bars: the restatement's per-element bound
(err / bound <= 1, the worst ratio printed: ``pytest -rP``) for the kernels; the project's own for gradients end to end,
err <= 1e-4 max|ref| per tensor (tests/test_gclstm_gpu.py).  The end-to-end tests also print the parity ratio -- the device's distance
from float64 against float32 autograd's own on the CPU -- without asserting it.
"""
import functools

import pytest
import torch

import gclstm_bwd_restate as br
import gclstm_restate as gr
from oracle.tgat_bwd_ref import EPS
from test_tgat_bwd_blocks_gpu import Buf, _report, _same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F64 = torch.float64
NORM = {None: 0, 'sym': 1, 'rw': 2}
LONG_ROW, VERY_LONG, CHUNK = 64, 2048, 1024  # kSpmmLongRow, kSpmmVeryLong, kSpmmChunk (csrc/spmm.h)


def _lib():
    from tgm_amd import _native

    return _native.load(), _native


def dev(v):
    return None if v is None else v.to(DEV)


# ---- tgmx_gclstm_gate_backward alone ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gate_case(N, C, saturate_all):
    return br.gate_case(N, C, saturate_all=saturate_all)


def _gate_want(N, C, saturate_all, dH, dC):
    return br.gate_bounds(_gate_case(N, C, saturate_all), dH, dC)  # (used once each: not kept, the large case is 130 MB a tensor)


def _gate_bwd(c, dH=True, dC=True, want_dcp=True):
    lib, native = _lib()
    N, C = c['Cprev'].shape
    pre, cp = Buf(N, 4 * C, data=c['pre']), Buf(N, C, data=c['Cprev'])
    gh, gc = Buf(N, C, ld=C + 3, lead=1, fill=7.0, data=c['dH']), Buf(N, C, ld=C + 5, lead=2, fill=7.0, data=c['dC'])
    outs = []
    for _ in range(2):
        dpre, dcp = Buf(N, 4 * C), Buf(N, C)
        native.check(lib.tgmx_gclstm_gate_backward(pre.ptr, cp.ptr, N, C, gh.ptr if dH else None, gh.ld, gc.ptr if dC else None, gc.ld, dpre.ptr,
                                                   dcp.ptr if want_dcp else None, native.stream_ptr()), 'tgmx_gclstm_gate_backward')  # fmt: skip
        torch.cuda.synchronize()
        assert dpre.sentinels_intact() and dcp.sentinels_intact(), 'a write outside dpre or dCprev'
        outs.append((dpre.view.clone(), dcp.view.clone()))
    assert _same_bits(outs[0][0], outs[1][0]) and (not want_dcp or _same_bits(outs[0][1], outs[1][1])), 'two launches differ'
    return outs[0]


def _check_gate(N, C, saturate_all):
    c = _gate_case(N, C, saturate_all)
    tag = f'gate_backward N={N} C={C}{" saturated" if saturate_all else ""}'
    full = None
    for dH, dC in ((True, True), (False, True), (True, False)):
        (want_p, want_c), (bp, bc) = _gate_want(N, C, saturate_all, dH, dC)
        dpre, dcp = _gate_bwd(c, dH, dC)
        assert _report(f'{tag} dpre dH={dH} dC={dC}', dpre, want_p, bp) <= 1.0
        assert _report(f'{tag} dCprev dH={dH} dC={dC}', dcp, want_c, bc) <= 1.0
        if dH and dC:
            full = dpre
        if not dH:  # the output gate sees dH' alone
            assert not dpre[:, 3 * C:].any()
    dpre, dcp = _gate_bwd(c, want_dcp=False)
    assert torch.isnan(dcp).all() and _same_bits(dpre, full)
    if c['band']:  # saturated sigmoids give exact zeros, no NaN
        assert torch.isfinite(full[c['band']]).all()


@pytest.mark.parametrize('N,C', br.GATE_CASES)
def test_gate_backward_alone(N, C):
    """One element; a few rows with a band row in the middle; 700 elements (three blocks, the last partial) with the band of four rows."""
    _check_gate(N, C, False)
    if N < 3:
        _check_gate(N, C, True)  # the only row is the band


def test_gate_backward_alone_past_the_block_cap():
    N, C = br.GATE_BIG_CASE
    assert N * C == 16384 * 256 + 96  # the second grid-stride trip carries exactly the tail
    _check_gate(N, C, False)


# ---- tgmx_cheb_laplacian_t against tgmx_cheb_laplacian ------------------------------------------------------------------------------------------
def _laplacian(which, ei, w, N, norm, lam, count=True):
    """(indptr, cols, vals, diag) on the host and the skipped count; every buffer sits inside sentinels."""
    lib, native = _lib()
    fn = getattr(lib, which)
    E = ei.shape[1]
    src, dst = dev(ei[0].contiguous()), dev(ei[1].contiguous())
    wd = dev(w)
    nbytes = lib.tgmx_cheb_workspace_bytes(E, N)
    assert nbytes > 0
    indptr, cols, vals, diag, ws = Buf(1, N + 1), Buf(1, max(E, 1)), Buf(1, max(E, 1)), Buf(1, N), Buf(1, (nbytes + 3) // 4)
    skipped = torch.zeros(1, dtype=torch.int32, device=DEV)
    native.check(fn(src.data_ptr(), dst.data_ptr(), int(ei.dtype == torch.int64), native.ptr(wd), E, N, NORM[norm], float(lam), None, indptr.ptr, cols.ptr,
                    vals.ptr, diag.ptr, ws.ptr, nbytes, skipped.data_ptr() if count else None, native.stream_ptr()), which)  # fmt: skip
    torch.cuda.synchronize()
    for b in (indptr, cols, vals, diag, ws):
        assert b.sentinels_intact(), f'{which}: a write outside a buffer'
    ip = indptr.view.reshape(-1).view(torch.int32).cpu().long()
    nnz = int(ip[N])
    return ip, cols.view.reshape(-1).view(torch.int32).cpu().long()[:nnz], vals.view.reshape(-1).cpu()[:nnz], diag.view.reshape(-1).cpu(), int(skipped.item())


def _triples(ip, cols, vals, N, swap=False):
    rows = torch.repeat_interleave(torch.arange(N), ip[1:] - ip[:-1])
    r, c = (cols, rows) if swap else (rows, cols)
    bits = vals.contiguous().view(torch.int32).long() & 0xFFFFFFFF
    return torch.sort(((r * N + c) << 32) | bits)[0]


def _check_transpose(ei, w, N, norm, lam, expect_skipped=0):
    fwd = _laplacian('tgmx_cheb_laplacian', ei, w, N, norm, lam)
    outs = [_laplacian('tgmx_cheb_laplacian_t', ei, w, N, norm, lam) for _ in range(2)]
    tr = outs[0]
    for a, b in zip(outs[0][:4], outs[1][:4]):
        assert _same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b), 'two launches differ'
    assert fwd[4] == tr[4] == expect_skipped
    assert _laplacian('tgmx_cheb_laplacian_t', ei, w, N, norm, lam, count=False)[4] == 0  # NULL: not counted
    assert int(fwd[0][N]) == int(tr[0][N]) and _same_bits(fwd[3], tr[3]), 'nnz or diag differ'
    assert torch.equal(_triples(*fwd[:3], N), _triples(*tr[:3], N, swap=True)), 'the entries are not the transposed multiset, bit for bit'
    ip, cols = tr[0], tr[1]
    for i in range(N):  # the destinations ascend within a row
        row = cols[int(ip[i]):int(ip[i + 1])]
        assert bool((row[1:] >= row[:-1]).all())
    return fwd, tr


def _mixed_graph(N, E, seed):
    """directed, with self loops, duplicates (in both orders of appearance) and repeated sources"""
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[:, 5:15] = ei[:, 15:25]  # duplicates
    ei[1, 30:34] = ei[0, 30:34]  # self loops
    return ei, torch.rand(E, generator=g) + 0.5


@pytest.mark.parametrize('idx', [torch.int32, torch.int64])
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('norm,lam', [('sym', 2.0), ('rw', 2.3), (None, 9.0)])
def test_laplacian_t_is_the_transpose_bit_for_bit(norm, lam, weighted, idx):
    N, E = 37, 260
    ei, w = _mixed_graph(N, E, 5)
    _check_transpose(ei.to(idx), w if weighted else None, N, norm, lam)
    bad = torch.cat([ei[:, :100], torch.tensor([[3, N + 4, -1], [N, 2, 5]]), ei[:, 100:]], dim=1)  # endpoints outside [0, N)
    wb = torch.cat([w[:100], torch.tensor([5.0, 6.0, 7.0]), w[100:]])
    fwd_bad, tr_bad = _check_transpose(bad.to(idx), wb if weighted else None, N, norm, lam, expect_skipped=3)
    fwd, tr = _check_transpose(ei.to(idx), w if weighted else None, N, norm, lam)
    for a, b in zip(tr_bad[:4], tr[:4]):  # the skipped edges leave no trace
        assert torch.equal(a, b) if a.dtype != torch.float32 else _same_bits(a, b)


def test_laplacian_t_keeps_duplicates_in_edge_order():
    """No normalisation, lambda_max = 2: vals = -w exactly, so a row's run of one destination spells the weights in edge order."""
    ei = torch.tensor([[4, 1, 4, 4, 2, 4, 1], [0, 3, 0, 2, 2, 0, 3]])
    w = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0])
    _, tr = _check_transpose(ei, w, 6, None, 2.0)
    ip, cols, vals = tr[0], tr[1], tr[2]
    assert cols[int(ip[4]):int(ip[5])].tolist() == [0, 0, 0, 2] and vals[int(ip[4]):int(ip[5])].tolist() == [-1.0, -3.0, -6.0, -4.0]
    assert cols[int(ip[1]):int(ip[2])].tolist() == [3, 3] and vals[int(ip[1]):int(ip[2])].tolist() == [-2.0, -7.0]
    assert int(ip[3]) == int(ip[2])  # node 2 sends only a self loop: dropped


def test_laplacian_t_degenerate_and_hub():
    empty = torch.zeros((2, 0), dtype=torch.int64)
    for norm, lam in (('sym', 2.0), (None, 3.0)):
        _check_transpose(empty, None, 9, norm, lam)  # E = 0
        _check_transpose(empty, None, 1, norm, lam)  # N = 1
        _check_transpose(torch.zeros((2, 3), dtype=torch.int64), torch.tensor([1.0, 2.0, 3.0]), 1, norm, lam)  # N = 1, self loops only
    g = torch.Generator().manual_seed(8)
    N = 2300
    hub = torch.stack([torch.zeros(2200, dtype=torch.int64), torch.randperm(N - 1, generator=g)[:2200] + 1])  # node 0 sends 2 200 edges
    ei = torch.cat([hub, torch.randint(0, N, (2, 3000), generator=g)], dim=1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    _, tr = _check_transpose(ei, torch.rand(ei.shape[1], generator=g) + 0.5, N, 'sym', 2.0)
    assert int(tr[0][1] - tr[0][0]) >= 2200


# ---- the Clenshaw pass alone ----------------------------------------------------------------------------------------------------------------------
CLENSHAW_N = 300


@functools.lru_cache(maxsize=None)
def _clenshaw_graph():
    """Sources 0 and 1 send 2 200 edges each (rows 0 and 1 of the transpose: very long, and chunk 2 of the entry array holds the end of one
    and the start of the other), source 2 sends 500, source 3 sends 65, source 4 sends 64, source 5 none; the rest a sparse random graph.
    The destinations repeat (300 nodes).  No normalisation with lambda_max = twice the largest degree keeps L_hat of order one."""
    g = torch.Generator().manual_seed(12)
    N = CLENSHAW_N
    parts = [(0, 2200), (1, 2200), (2, 500), (3, 65), (4, 64)]
    src = torch.cat([torch.full((n,), s, dtype=torch.int64) for s, n in parts])
    dst = torch.randint(6, N, (src.numel(),), generator=g)
    rest = torch.randint(6, N, (2, 900), generator=g)
    ei = torch.cat([torch.stack([src, dst]), rest], dim=1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    w = torch.rand(ei.shape[1], generator=g) + 0.5
    assert (2200 // CHUNK) == (2200 + 10) // CHUNK == 2 and 2200 > VERY_LONG and 65 == LONG_ROW + 1
    ip, cols, vals, diag, _ = _laplacian('tgmx_cheb_laplacian_t', ei, w, N, None, 2.0 * 2200 * 1.5, count=False)
    deg = ip[1:] - ip[:-1]
    assert deg[:6].tolist() == [2200, 2200, 500, 65, 64, 0]
    rows = torch.repeat_interleave(torch.arange(N), deg)
    lap = (rows, cols, vals.double(), diag.double())  # propagate_t: out[row] += m t[col] -- the CSR's own rows
    csr = tuple(dev(t) for t in (ip.to(torch.int32), cols.to(torch.int32), vals, diag))
    return ei.shape[1], lap, csr, deg


def _clenshaw_device(C, K, aligned):
    lib, native = _lib()
    E, lap, csr, deg = _clenshaw_graph()
    N = CLENSHAW_N
    g = torch.Generator().manual_seed(100 * K + C)
    grad = torch.randn(N, K * C, generator=g)
    n = lib.tgmx_cheb_propagate_scratch_floats(E, C)
    assert n > 0
    ldg = (K * C + 3) // 4 * 4 + 4 if aligned else K * C + 3
    outs = []
    for _ in range(2):
        gb = Buf(N, K * C, ld=ldg, lead=0 if aligned else 1, fill=7.0, data=grad)
        out, ws = Buf(N, C, ld=(C + 3) // 4 * 4 + 4 if aligned else C + 2, lead=0 if aligned else 1), Buf(1, n)
        native.check(lib.tgmx_cheb_clenshaw(*(t.data_ptr() for t in csr), N, C, K, gb.ptr, gb.ld, out.ptr, out.ld, E, ws.ptr, n, native.stream_ptr()),
                     'tgmx_cheb_clenshaw')
        torch.cuda.synchronize()
        assert gb.sentinels_intact() and out.sentinels_intact() and ws.sentinels_intact(), 'a write outside the basis, dH or the scratch'
        outs.append(out.view.contiguous().clone())
    assert _same_bits(outs[0], outs[1]), 'two launches differ'
    want, mag = br.clenshaw(lap, grad, K)
    chain = br.clenshaw_chain(K, deg.double()[:, None], int(deg.max()))
    return outs[0], want, chain * EPS * mag, lap, grad


@pytest.mark.parametrize('K', [1, 2, 3, 4])
@pytest.mark.parametrize('C', [1, 5, 64, 260])
def test_clenshaw_alone(C, K):
    """Widths: scalar lanes with a tail (1, 5), one float4 a lane short of a pass (64), a second pass (260).  Rows of the transpose: 0, 64
    (one wave), 65 and 500 (four waves), 2 200 twice (the chunk launches, sharing a chunk)."""
    lib, native = _lib()
    if K == 1:  # dH = g_0: the one call writes the GEMM straight into dH and reads no graph
        x = torch.zeros(8, device=DEV).data_ptr()
        assert lib.tgmx_cheb_clenshaw(x, x, x, x, 4, C, 1, x, C, x, C, 0, None, 0, None) != 0 and b'K=1' in lib.tgmx_last_error()
        return
    got, want, bound, lap, grad = _clenshaw_device(C, K, aligned=C % 4 == 0)
    assert _report(f'clenshaw C={C} K={K}', got, want, bound) <= 1.0
    for mutation, (part, shows) in br.MUTATIONS.items():  # the bound tells the wrong variants apart
        if part == 'clenshaw' and shows(K=K):
            wrong, _ = br.clenshaw(lap, grad, K, mutate=mutation)
            assert float(((wrong - want).abs() / bound).max()) > 1.0, mutation


@pytest.mark.parametrize('K', [2, 4])
def test_clenshaw_alone_off_the_16_byte_grid(K):
    """64 channels in an operand whose leading dimension is odd and whose first column is off the grid: the scalar lanes."""
    got, want, bound, _, _ = _clenshaw_device(64, K, aligned=False)
    assert _report(f'clenshaw C=64 K={K} unaligned', got, want, bound) <= 1.0
    same, _, _, _, _ = _clenshaw_device(64, K, aligned=True)
    assert _report(f'clenshaw C=64 K={K} aligned', same, want, bound) <= 1.0


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
BAR = 1e-4  # err <= 1e-4 max|ref| per tensor (tests/test_gclstm_gpu.py, README)


def make_cell(cin, Co, K, norm, bias, seed=0):
    from tgm_amd.nn import GCLSTM

    torch.manual_seed(seed)
    cell = GCLSTM(cin, Co, K, normalization=norm, bias=bias)
    with torch.no_grad():
        for p in cell.parameters():
            p.uniform_(-0.5, 0.5)
    return cell


def make_snaps(seed, N, cin, sizes, weighted):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(N, cin, generator=g), torch.randint(0, N, (2, E), generator=g), torch.rand(E, generator=g) + 0.5 if weighted else None)
            for E in sizes]  # fmt: skip


def host_grads(sd, snaps, H0, C0, wH, wC, norm, lm, req, dtype, chain=True):
    """Autograd through the restatement on the CPU: name -> gradient (a tensor nothing reached counts as zeros).  ``chain``: the snapshots
    are a recurrence (BPTT); else every snapshot starts from (H0, C0) and the losses add up (two calls before one backward)."""
    leaf = lambda t, on: t.detach().to(dtype).clone().requires_grad_(on)  # (a copy: .to() of the same dtype is the caller's own tensor)
    p = {k: leaf(v, 'params' in req) for k, v in sd.items()}
    xs = [leaf(x, 'x' in req) for x, _, _ in snaps]
    H, C = (None if H0 is None else leaf(H0, 'H' in req)), (None if C0 is None else leaf(C0, 'C' in req))
    loss, Hs, Cs = 0.0, H, C
    for i, (x, (_, ei, ew)) in enumerate(zip(xs, snaps)):
        Hs, Cs = gr.gclstm_forward(p, x, ei, ew, Hs if chain else H, Cs if chain else C, lm, norm, dtype=dtype)
        if not chain or i == len(snaps) - 1:
            loss = loss + (0.0 if wH is None else (Hs * wH.to(dtype)).sum()) + (0.0 if wC is None else (Cs * wC.to(dtype)).sum())
    loss.backward()
    out = {}
    if 'params' in req:
        out.update(p)
    if 'x' in req:
        out.update({f'node_x{i}': x for i, x in enumerate(xs)})
    if 'H' in req and H is not None:
        out['H0'] = H
    if 'C' in req and C is not None:
        out['C0'] = C
    return {k: (torch.zeros_like(t) if t.grad is None else t.grad).detach() for k, t in out.items()}, Hs.detach(), Cs.detach()


def device_grads(cell, snaps, H0, C0, wH, wC, lm, req, chain=True):
    for p in cell.parameters():
        p.requires_grad_('params' in req)
        p.grad = None
    xs = [dev(x).requires_grad_('x' in req) for x, _, _ in snaps]
    H, C = (None if H0 is None else dev(H0).requires_grad_('H' in req)), (None if C0 is None else dev(C0).requires_grad_('C' in req))
    loss, Hs, Cs = 0.0, H, C
    for i, (x, (_, ei, ew)) in enumerate(zip(xs, snaps)):
        Hs, Cs = cell(x, dev(ei), dev(ew), Hs if chain else H, Cs if chain else C, lm)
        assert 'GclstmFunction' in type(Hs.grad_fn).__name__ and Hs.grad_fn is Cs.grad_fn
        if not chain or i == len(snaps) - 1:
            loss = loss + (0.0 if wH is None else (Hs * dev(wH)).sum()) + (0.0 if wC is None else (Cs * dev(wC)).sum())
    loss.backward()
    out = {}
    if 'params' in req:
        out.update(dict(cell.named_parameters()))
    if 'x' in req:
        out.update({f'node_x{i}': x for i, x in enumerate(xs)})
    if 'H' in req and H is not None:
        out['H0'] = H
    if 'C' in req and C is not None:
        out['C0'] = C
    return {k: t.grad for k, t in out.items()}, Hs.detach(), Cs.detach()


def check_grads(label, got, ref, f32):
    assert set(got) == set(ref), (label, set(got) ^ set(ref))
    worst = 0.0
    for k in ref:
        assert got[k] is not None, (label, k)
        g = got[k].detach().cpu().double()
        assert g.shape == ref[k].shape and torch.isfinite(g).all(), (label, k)
        err, scale = (g - ref[k]).abs().max().item() if g.numel() else 0.0, ref[k].abs().max().item() if g.numel() else 0.0
        own = (f32[k].double() - ref[k]).abs().max().item() if g.numel() else 0.0
        ratio = err / max(own, 1e-30)
        print(f'gclstm gradient {label} {k}: {err:.3e} of {scale:.3e}, float32 autograd {own:.3e}, parity ratio {ratio:.2f}')
        assert err <= BAR * scale, f'{label} {k}: {err:.3e} vs {scale:.3e}'
        worst = max(worst, ratio if own >= 1e-9 else 0.0)
    print(f'gclstm gradient {label}: worst parity ratio {worst:.2f}')


def run_case(label, cell, snaps, H0, C0, wH, wC, norm, lm, req, chain=True):
    sd = {k: v.detach().cpu().clone() for k, v in cell.state_dict().items()}
    ref, H64, C64 = host_grads(sd, snaps, H0, C0, wH, wC, norm, lm, req, F64, chain)
    f32, _, _ = host_grads(sd, snaps, H0, C0, wH, wC, norm, lm, req, torch.float32, chain)
    cell = cell.to(DEV).train()
    got, Hd, Cd = device_grads(cell, snaps, H0, C0, wH, wC, lm, req, chain)
    check_grads(label, got, ref, f32)
    gr.close(Hd.cpu(), H64.float(), f'{label} H')
    gr.close(Cd.cpu(), C64.float(), f'{label} C')
    cell.check()
    return got


N_E2E, CIN, CO = 40, 6, 8
# (normalisation, lambda_max, K, bias, weighted)
CONFIGS = [('sym', None, 1, True, True), ('sym', None, 2, True, False), ('sym', None, 3, True, True), ('sym', None, 3, False, True),
           ('rw', 2.3, 2, True, True), ('rw', 2.3, 3, False, False), (None, 12.0, 3, True, True), (None, 12.0, 1, False, True)]  # fmt: skip
SUBSETS = {'params': {'params'}, 'params+x': {'params', 'x'}, 'params+x+HC': {'params', 'x', 'H', 'C'}, 'H alone, frozen': {'H'}}


def _states(seed, N=N_E2E, Co=CO):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(N, Co, generator=g) * s for s in (0.5, 0.5, 1.0, 1.0))  # H0, C0, wH, wC


@pytest.mark.parametrize('subset', list(SUBSETS))
@pytest.mark.parametrize('cfg', CONFIGS, ids=lambda c: f'{c[0]}-K{c[2]}-{"bias" if c[3] else "nobias"}-{"w" if c[4] else "unw"}')
def test_gradients_against_float64_autograd(cfg, subset):
    norm, lm, K, bias, weighted = cfg
    H0, C0, wH, wC = _states(K)
    snaps = make_snaps(10 * K + int(weighted), N_E2E, CIN, (150,), weighted)
    run_case(f'{norm} K={K} bias={bias} weighted={weighted} [{subset}]', make_cell(CIN, CO, K, norm, bias, seed=K), snaps, H0, C0, wH, wC, norm, lm,
             SUBSETS[subset])  # fmt: skip


@pytest.mark.parametrize('only', ['H', 'C'])
def test_a_loss_on_one_output_alone(only):
    H0, C0, wH, wC = _states(3)
    snaps = make_snaps(77, N_E2E, CIN, (150,), True)
    cell = make_cell(CIN, CO, 3, 'sym', True, seed=7)
    got = run_case(f'loss on {only} alone', cell, snaps, H0, C0, wH if only == 'H' else None, wC if only == 'C' else None, 'sym', None,
                   {'params', 'x', 'H', 'C'})  # fmt: skip
    if only == 'C':  # the output gate takes no part in C': exact zeros
        assert not got['W_o'].any() and not got['conv_o.lins.1.weight'].any() and not got['b_o'].any() and not got['conv_o.bias'].any()


@pytest.mark.parametrize('K', [1, 3])
def test_two_snapshots_of_bptt(K):
    H0, C0, wH, wC = _states(5)
    snaps = make_snaps(41 + K, N_E2E, CIN, (150, 90), True)
    run_case(f'BPTT K={K}', make_cell(CIN, CO, K, 'sym', True, seed=41), snaps, H0, C0, wH, wC, 'sym', None, {'params', 'x', 'H', 'C'})
    run_case(f'BPTT from zero states K={K}', make_cell(CIN, CO, K, 'sym', True, seed=42), snaps, None, None, wH, wC, 'sym', None, {'params', 'x'})


def test_two_calls_on_one_module_before_one_backward():
    """The second call must not overwrite what the first saved: different graphs, different inputs, one module."""
    H0, C0, wH, wC = _states(6)
    snaps = make_snaps(61, N_E2E, CIN, (150, 400), True)
    run_case('two calls, one backward', make_cell(CIN, CO, 3, 'sym', True, seed=61), snaps, H0, C0, wH, wC, 'sym', None, {'params', 'x', 'H', 'C'},
             chain=False)  # fmt: skip


@pytest.mark.parametrize('name', gr.EXPECTED_FIXTURES)
def test_fixture_replay_with_a_backward_after_the_last_snapshot(name):
    from tgm_amd.nn import GCLSTM

    meta, params, fsnaps = gr.load_fixture(name)
    cell = GCLSTM(meta['in_channels'], meta['out_channels'], meta['K'], normalization=meta['normalization'], bias=meta['bias'])
    cell.load_state_dict(params, strict=True)
    snaps = [(s['x'], s['edge_index'], s['edge_weight']) for s in fsnaps]
    N, Co = snaps[0][0].shape[0], meta['out_channels']
    _, _, wH, wC = _states(len(name), N, Co)
    got = run_case(f'fixture {name}', cell, snaps, None, None, wH, wC, meta['normalization'], meta['lambda_max'], {'params', 'x'})
    assert len(got) == len(params) + len(snaps)


def test_chebconv_alone_under_gradients():
    from tgm_amd.nn import ChebConv

    for (norm, lm, K, bias, weighted), cin, cout in zip(CONFIGS[:7], (5, 6, 8, 3, 4, 7, 64), (7, 4, 8, 5, 12, 6, 10)):
        g = torch.Generator().manual_seed(K + cin)
        torch.manual_seed(K + cin)
        conv = ChebConv(cin, cout, K, normalization=norm, bias=bias)
        if bias:
            with torch.no_grad():
                conv.bias.uniform_(-0.5, 0.5, generator=g)
        N = 50
        x, ei = torch.randn(N, cin, generator=g), torch.randint(0, N, (2, 220), generator=g)
        ew = torch.rand(220, generator=g) + 0.5 if weighted else None
        w_out = torch.randn(N, cout, generator=g)
        host = {}
        for dtype in (F64, torch.float32):
            ws = [l.weight.detach().to(dtype).requires_grad_() for l in conv.lins]
            b = None if conv.bias is None else conv.bias.detach().to(dtype).requires_grad_()
            xh = x.to(dtype).clone().requires_grad_()
            out = gr.cheb_conv(ws, b, xh, ei, ew, norm, lm, dtype=dtype)
            (out * w_out.to(dtype)).sum().backward()
            host[dtype] = {**{f'lins.{k}.weight': w.grad for k, w in enumerate(ws)}, 'x': xh.grad, **({} if b is None else {'bias': b.grad})}
            out64 = out.detach() if dtype == F64 else out64
        conv = conv.to(DEV).train()
        xd = dev(x).requires_grad_()
        with torch.no_grad():
            plain = conv(xd, dev(ei), dev(ew), lm)
        out = conv(xd, dev(ei), dev(ew), lm)
        assert 'ChebConvFunction' in type(out.grad_fn).__name__ and _same_bits(out, plain)
        (out * dev(w_out)).sum().backward()
        got = {**{k: p.grad for k, p in conv.named_parameters()}, 'x': xd.grad}
        check_grads(f'ChebConv {norm} K={K} in={cin} out={cout}', got, host[F64], host[torch.float32])
        gr.close(out.detach().cpu(), out64.float(), 'ChebConv forward under gradients')
        # frozen parameters: x alone
        for p in conv.parameters():
            p.requires_grad_(False)
            p.grad = None
        x2 = dev(x).requires_grad_()
        (conv(x2, dev(ei), dev(ew), lm) * dev(w_out)).sum().backward()
        assert _same_bits(x2.grad, xd.grad) and all(p.grad is None for p in conv.parameters())
        conv.check()


def test_an_out_of_range_edge_under_gradients():
    """check() raises once -- the backward's Laplacian does not count the edge again -- and the gradients are those of the clean graph."""
    H0, C0, wH, wC = _states(9)
    (x, good, w_good), = make_snaps(91, N_E2E, CIN, (150,), True)
    bad = torch.cat([good[:, :70], torch.tensor([[3], [N_E2E + 2]]), good[:, 70:]], dim=1)
    w_bad = torch.cat([w_good[:70], torch.tensor([5.0]), w_good[70:]])
    cell = make_cell(CIN, CO, 3, 'sym', True, seed=91).to(DEV).train()
    req = {'params', 'x', 'H', 'C'}
    clean, _, _ = device_grads(cell, [(x, good, w_good)], H0, C0, wH, wC, None, req)
    clean = {k: v.clone() for k, v in clean.items()}
    cell.check()
    got, _, _ = device_grads(cell, [(x, bad, w_bad)], H0, C0, wH, wC, None, req)
    assert int(cell.__dict__['_tgmx_skipped'].item()) == 1  # one forward, one edge; the backward added nothing
    with pytest.raises(ValueError, match='outside'):
        cell.check()
    cell.check()  # reported once
    for k in clean:
        assert _same_bits(got[k], clean[k]), k


# ---- dispatch ---------------------------------------------------------------------------------------------------------------------------------------
def _dispatch_setup(K=3):
    H0, C0, wH, wC = _states(11)
    snaps = make_snaps(111, N_E2E, CIN, (150,), True)
    return make_cell(CIN, CO, K, 'sym', True, seed=111).to(DEV).train(), snaps, H0, C0, wH, wC


def test_the_grad_enabled_forward_is_the_no_grad_forward_bit_for_bit():
    cell, snaps, H0, C0, _, _ = _dispatch_setup()
    x, ei, ew = snaps[0]
    with torch.no_grad():
        Hn, Cn = cell(dev(x), dev(ei), dev(ew), dev(H0), dev(C0))
    Hg, Cg = cell(dev(x), dev(ei), dev(ew), dev(H0), dev(C0))
    assert Hn.grad_fn is None and Hg.requires_grad and Cg.requires_grad
    assert type(Hg.grad_fn).__name__.startswith('GclstmFunction') and Hg.grad_fn is Cg.grad_fn
    assert _same_bits(Hg, Hn) and _same_bits(Cg, Cn)
    for p in cell.parameters():  # frozen parameters, a state that wants a gradient: still the native path
        p.requires_grad_(False)
    Hs, _ = cell(dev(x), dev(ei), dev(ew), dev(H0).requires_grad_(), dev(C0))
    assert type(Hs.grad_fn).__name__.startswith('GclstmFunction') and _same_bits(Hs, Hn)
    H2, _ = cell(dev(x), dev(ei), dev(ew), dev(H0), dev(C0))  # nothing to track: the inference call
    assert H2.grad_fn is None and not H2.requires_grad and _same_bits(H2, Hn)


def test_modes_and_the_composed_path(monkeypatch):
    cell, snaps, H0, C0, wH, wC = _dispatch_setup()
    req = {'params', 'x', 'H', 'C'}
    monkeypatch.delenv('TGMX_GCLSTM_BWD', raising=False)
    one, H1, C1 = device_grads(cell, snaps, H0, C0, wH, wC, None, req)
    one = {k: v.clone() for k, v in one.items()}
    again, _, _ = device_grads(cell, snaps, H0, C0, wH, wC, None, req)
    for k in one:  # two backward runs give the same bits
        assert _same_bits(one[k], again[k]), k
    monkeypatch.setenv('TGMX_GCLSTM_BWD', 'py')
    per_launch, H2, C2 = device_grads(cell, snaps, H0, C0, wH, wC, None, req)
    assert _same_bits(H1, H2) and _same_bits(C1, C2)
    for k in one:
        assert _same_bits(one[k], per_launch[k]), f'{k}: the per-launch path and the one call differ'
    monkeypatch.setenv('TGMX_GCLSTM_BWD', 'torch')
    x, ei, ew = snaps[0]
    for p in cell.parameters():
        p.grad = None
    Ht, Ct = cell(dev(x), dev(ei), dev(ew), dev(H0), dev(C0))
    assert Ht.requires_grad and 'GclstmFunction' not in type(Ht.grad_fn).__name__
    ((Ht * dev(wH)).sum() + (Ct * dev(wC)).sum()).backward()
    for k, p in cell.named_parameters():  # the composed path's gradients and the native ones meet at the bar
        err, scale = (p.grad - one[k]).abs().max().item(), one[k].abs().max().item()
        assert err <= 2 * BAR * scale, (k, err, scale)
    monkeypatch.delenv('TGMX_GCLSTM_BWD')
    wt = dev(ew).requires_grad_()
    Hw, _ = cell(dev(x), dev(ei), wt, dev(H0), dev(C0))
    assert Hw.requires_grad and 'GclstmFunction' not in type(Hw.grad_fn).__name__  # a gradient for edge_weight: the composed path
    Hw.sum().backward()
    assert wt.grad is not None and torch.isfinite(wt.grad).all()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        Ha, _ = cell(dev(x), dev(ei), dev(ew), dev(H0), dev(C0))
    assert 'GclstmFunction' not in type(Ha.grad_fn).__name__
    cell.check()


def test_an_in_place_write_to_the_cell_state_before_backward_is_refused():
    """The backward reads the caller's C where it lies (H and node_x are copied into the operand): autograd's version check guards it."""
    cell, snaps, H0, C0, wH, _ = _dispatch_setup()
    x, ei, ew = snaps[0]
    Cd = dev(C0)
    H, _ = cell(dev(x), dev(ei), dev(ew), dev(H0), Cd)
    Cd.add_(1.0)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        (H * dev(wH)).sum().backward()


def test_example_step_builds_no_transpose_and_leaves_detached_states_alone():
    """examples/linkproppred/gclstm.py: h_0 / c_0 detached, node features without gradient -- parameters only, K = 1 and K = 2."""
    for K in (1, 2):
        cell, snaps, H0, C0, wH, wC = _dispatch_setup(K)
        lin = torch.nn.Linear(CO, CO).to(DEV)
        x, ei, ew = snaps[0]
        h, c = cell(dev(x), dev(ei), None, dev(H0), dev(C0))
        z = lin(torch.relu(h))
        z.square().mean().backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in cell.parameters())
        assert cell.W_o.grad.abs().max() > 0 and cell.W_i.grad.abs().max() > 0
        h, c = h.detach(), c.detach()
        h2, _ = cell(dev(x), dev(ei), None, h, c)
        assert type(h2.grad_fn).__name__.startswith('GclstmFunction')
