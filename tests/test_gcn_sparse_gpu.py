"""GCNConv / TGCN over the sparse adjacency on the device (``propagate='sparse'``, ``GCNGraph``), training included, against the float64
restatement over the edge list (tests/gcn_sparse_restate.py): the CSR transpose entry by entry, the forward on either side of the dense cap,
the saving forward against the inference one bit for bit, every gradient against float64 autograd, the one-call backward against its
launches one by one, determinism, routing, ``check()`` and what the autograd context keeps.

Shapes.  T1: 37 nodes, 300 edges with repeats, explicit self loops (one node has two) and two ids out of range.  T2: the degenerate
graphs.  T3: 3 000 nodes, 6 000 edges, 2 500 INTO node 5 (a forward row above 2 048 entries) and 2 500 OUT OF node 3 (a transposed row above
2 048: the chunked route of the propagate), 100 into node 7 and out of node 9 (rows split over a workgroup's waves).  T4: 20 000 nodes,
above the dense cap.  Widths: C = 5 (scalar lanes; 3C = 15 is unaligned) with Fin = 3, C = 32 (float4 lanes) with Fin = 16."""
import functools

import pytest
import torch

import gcn_sparse_restate as gr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64
WIDTHS = [(3, 5), (16, 32)]  # (Fin, C)
U = 2.0**-24


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edges(name):
    """(edge_index int64 [2, E], edge_weight [E], N) on the host; never modified."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if name in ('T1', 'T1_inside'):
        N, E = 37, 300
        ei = torch.randint(0, N, (2, E), generator=g)
        ei[:, :8] = ei[0, :8]  # explicit self loops
        ei[:, 8] = ei[:, 0]  # a second loop on one node: the later one's weight counts
        ei[:, 20:30] = ei[:, 40:50]  # repeated edges
        if name == 'T1':
            ei[0, 60], ei[1, 61] = -1, N
    elif name == 'T3':
        N, E = 3000, 6000
        ei = torch.randint(0, N, (2, E), generator=g)
        ei[1, :2500] = 5
        ei[0, 2500:5000] = 3
        ei[1, 5000:5100] = 7
        ei[0, 5100:5200] = 9
        ei[:, 5200:5204] = ei[0, 5200:5204]
    elif name == 'T4':
        N, E = 20000, 3000
        ei = torch.randint(0, N, (2, E), generator=g)
        ei[:, :20] = ei[:, 100:120]
        ei[:, 50:54] = ei[0, 50:54]
    elif name == 'one_node':
        N, ei = 1, torch.zeros((2, 0), dtype=torch.int64)
    elif name == 'no_edges':
        N, ei = 5, torch.zeros((2, 0), dtype=torch.int64)
    elif name == 'all_outside':
        N, ei = 5, torch.tensor([[-1, 5, 7, 2, -3], [0, 1, 9, 5, -1]])
    elif name == 'all_loops':
        N, ei = 5, torch.tensor([[0, 1, 1, 3, 4, 4], [0, 1, 1, 3, 4, 4]])
    else:
        raise KeyError(name)
    return ei, torch.rand(ei.shape[1], generator=g) + 0.2, N


DEGENERATE = ['one_node', 'no_edges', 'all_outside', 'all_loops']
# (case, weighted, improved, add_self_loops, ids)
VARIANTS = [('T1', False, False, True, torch.int64), ('T1', True, True, True, torch.int32), ('T1', True, False, False, torch.int64),
            ('T1', False, True, False, torch.int32), ('T3', True, False, True, torch.int64), ('T4', True, True, True, torch.int32)]  # fmt: skip
VARIANTS += [(name, True, False, asl, torch.int64) for name in DEGENERATE for asl in (True, False)]
ids_of = lambda v: f'{v[0]}-{"w" if v[1] else "u"}-{"imp" if v[2] else "std"}-{"loops" if v[3] else "noloops"}-{str(v[4])[-5:]}'


def on_device(name, weighted, ids=torch.int64):
    ei, ew, N = edges(name)
    return ei.to(ids).to(DEV), (ew.to(DEV) if weighted else None), N


def restated(name, weighted, improved, asl, dtype=F64):
    ei, ew, N = edges(name)
    return gr.gcn_norm(ei, ew if weighted else None, N, improved, asl, dtype=dtype)


def tensors(seed, *shapes, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [scale * torch.randn(*s, generator=g) for s in shapes]


def make(cls, Fin, C, seed=0, **kw):
    torch.manual_seed(seed)
    m = cls(Fin, C, **kw)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn_like(p))  # (the biases start at zero)
    return m.to(DEV)


def params64(m):
    return {k: v.detach().cpu().to(F64).requires_grad_(True) for k, v in m.named_parameters()}


def close(got, ref, label):
    """The project's bar for aggregated embeddings: every element within 1e-5 relative to max(1, |element|)."""
    got, ref = got.detach().cpu().to(F64), ref.detach().to(F64)
    assert got.shape == ref.shape and torch.isfinite(got).all(), label
    worst = ((got - ref).abs() / ref.abs().clamp(min=1.0)).max().item() if got.numel() else 0.0
    print(f'gcn sparse forward {label}: {worst:.3e}')
    assert worst <= 1e-5, (label, worst)


def gclose(got, ref, label):
    """The project's bar for gradients: within 1e-4 of the gradient's largest entry."""
    assert got is not None, label
    scale, err = ref.abs().max().item(), (got.detach().cpu().to(F64) - ref).abs().max().item()
    print(f'gcn sparse gradient {label}: {err:.3e} of {scale:.3e}')
    assert err <= 1e-4 * max(scale, 1e-30), f'{label}: max |d| {err:.3e} vs gradient max {scale:.3e}'


def bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


# ---- 1. the transpose ---------------------------------------------------------------------------------------------------------------------
def host_csr(csr):
    indptr, cols, vals, diag = (t.cpu() for t in csr)
    nnz = int(indptr[-1])
    rows = torch.repeat_interleave(torch.arange(indptr.numel() - 1), (indptr[1:] - indptr[:-1]).long())
    return indptr, rows, cols[:nnz].long(), vals[:nnz], diag, nnz


@pytest.mark.parametrize('variant', [v for v in VARIANTS if v[0] != 'T4'], ids=ids_of)
def test_transpose_entry_by_entry(variant):
    from tgm_amd.nn import gcn_graph
    from tgm_amd.nn._snapshot import csr_transpose

    name, weighted, improved, asl, ids = variant
    ei, ew, N = on_device(name, weighted, ids)
    graph = gcn_graph(ei, ew, num_nodes=N, improved=improved, add_self_loops=asl)
    indptr, rows, cols, vals, diag, nnz = host_csr(graph.csr)
    want = restated(name, weighted, improved, asl)
    assert nnz == want.src.numel() and (indptr[1:] >= indptr[:-1]).all()
    t1, t2 = graph.transposed(), csr_transpose(graph.csr, N)
    assert graph.transposed() is t1  # built once
    indptr_t, rows_t, cols_t, vals_t, diag_t, nnz_t = host_csr(t1)
    assert nnz_t == nnz == int(indptr_t[N]) and indptr_t.numel() == N + 1 and int(indptr_t[0]) == 0
    assert torch.equal(diag_t, diag)
    # the forward's entries in a stable order by (col, row) ARE the transposed CSR: columns ascend within a row, equal (row, col) entries
    # keep the forward's order, every value is the forward's bit for bit
    order = torch.sort(cols * N + rows, stable=True).indices
    assert torch.equal(rows_t, cols[order]) and torch.equal(cols_t, rows[order])
    assert torch.equal(vals_t.view(torch.int32), vals[order].view(torch.int32))
    same_row = rows_t[1:] == rows_t[:-1]
    assert (cols_t[1:][same_row] >= cols_t[:-1][same_row]).all()
    # as sorted lists of (row, col, value bits)
    key = lambda r, c, v: torch.sort((r * N + c) * (1 << 32) + (v.view(torch.int32).long() & 0xFFFFFFFF)).values
    assert torch.equal(key(rows_t, cols_t, vals_t), key(cols, rows, vals))
    assert torch.equal(t1[0], t2[0]) and torch.equal(t1[1][:nnz], t2[1][:nnz]) and bits(t1[2][:nnz], t2[2][:nnz])  # two runs: the same arrays


def test_transpose_copies_the_diagonal_when_asked():
    from tgm_amd import _native
    from tgm_amd.nn import gcn_graph

    ei, ew, N = on_device('T1', True)
    graph = gcn_graph(ei, ew, num_nodes=N)
    indptr, cols, vals, diag = graph.csr
    lib, E = _native.load(), graph.E
    nbytes = lib.tgmx_csr_transpose_workspace_bytes(E, N)
    it, ct = torch.empty(N + 1, dtype=torch.int32, device=DEV), torch.empty(E, dtype=torch.int32, device=DEV)
    vt, dt, ws = torch.empty(E, device=DEV), torch.full((N,), -1.0, device=DEV), torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _native.check(lib.tgmx_csr_transpose(indptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), diag.data_ptr(), N, E, it.data_ptr(), ct.data_ptr(),
                                         vt.data_ptr(), dt.data_ptr(), ws.data_ptr(), nbytes, _native.stream_ptr()), 'tgmx_csr_transpose')  # fmt: skip
    assert bits(dt, diag) and torch.equal(it.cpu(), graph.transposed()[0].cpu())


@pytest.mark.parametrize('C', [5, 32])
@pytest.mark.parametrize('variant', [v for v in VARIANTS if v[0] in ('T1', 'T3', 'all_loops', 'no_edges')], ids=ids_of)
def test_transposed_propagate_against_its_bound(variant, C):
    from tgm_amd.nn import gcn_graph
    from tgm_amd.nn._snapshot import gcn_propagate, propagate_scratch

    name, weighted, improved, asl, ids = variant
    ei, ew, N = on_device(name, weighted, ids)
    graph = gcn_graph(ei, ew, num_nodes=N, improved=improved, add_self_loops=asl)
    want = restated(name, weighted, improved, asl)
    (y,) = tensors(7, (N, C))
    ref = gr.adj_matmul(want, y.to(F64), transpose=True)
    bound = (gr.row_lengths(want, transpose=True).to(F64).unsqueeze(1) + 2) * U * gr.adj_abs_matmul(want, y.to(F64), transpose=True)
    csr_t, yd = graph.transposed(), y.to(DEV)
    outs = []
    for scratch in (None, propagate_scratch(csr_t, C)):
        out = gcn_propagate(csr_t, yd, torch.empty_like(yd), scratch=scratch, E=graph.E)
        assert ((out.cpu().to(F64) - ref).abs() <= bound).all(), (name, C, scratch is not None)
        outs.append(out)
    if name == 'T3':
        assert propagate_scratch(csr_t, C) is not None and int(gr.row_lengths(want, transpose=True).max()) > 2048
        assert int(gr.row_lengths(want).max()) > 2048 and ((gr.row_lengths(want) > 64) & (gr.row_lengths(want) <= 2048)).any()


# ---- 2. forward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Fin,C', WIDTHS)
@pytest.mark.parametrize('variant', VARIANTS, ids=ids_of)
def test_forward_against_the_restatement(variant, Fin, C):
    from tgm_amd.nn import TGCN, GCNConv, gcn_graph

    name, weighted, improved, asl, ids = variant
    ei, ew, N = on_device(name, weighted, ids)
    want = restated(name, weighted, improved, asl)
    x, H = tensors(1, (N, Fin), (N, C))
    conv = make(GCNConv, Fin, C, improved=improved, add_self_loops=asl, propagate='sparse')
    cell = make(TGCN, Fin, C, improved=improved, add_self_loops=asl, propagate='sparse')
    pc, pt = params64(conv), params64(cell)
    with torch.no_grad():
        out_c, out_t, out_t0 = conv(x.to(DEV), ei, ew), cell(x.to(DEV), ei, ew, H.to(DEV)), cell(x.to(DEV), ei, ew)
        close(out_c, gr.gcn_conv(want, x.to(F64), pc['lin.weight'], pc['bias']), f'GCNConv {ids_of(variant)}')
        close(out_t, gr.tgcn_cell(pt, want, x.to(F64), H.to(F64)), f'TGCN {ids_of(variant)}')
        close(out_t0, gr.tgcn_cell(pt, want, x.to(F64)), f'TGCN H=None {ids_of(variant)}')
        # a GCNGraph in place of edge_index: the same bits, whatever the module's propagate=
        graph = gcn_graph(ei, ew, num_nodes=N, improved=improved, add_self_loops=asl)
        assert bits(conv(x.to(DEV), graph), out_c) and bits(cell(x.to(DEV), graph, None, H.to(DEV)), out_t)
        conv.propagate = cell.propagate = 'auto'
        assert bits(conv(x.to(DEV), graph), out_c) and bits(cell(x.to(DEV), graph, H=H.to(DEV)), out_t)


@pytest.mark.parametrize('Fin,C', WIDTHS)
@pytest.mark.parametrize('weighted', [False, True])
def test_sparse_against_the_dense_route(weighted, Fin, C):
    from tgm_amd.nn import TGCN, GCNConv

    ei, ew, N = on_device('T1_inside', weighted)  # (the dense builder does not take ids out of range)
    x, H = tensors(2, (N, Fin), (N, C))
    for cls, args in ((GCNConv, (x.to(DEV), ei, ew)), (TGCN, (x.to(DEV), ei, ew, H.to(DEV)))):
        m = make(cls, Fin, C, propagate='sparse')
        with torch.no_grad():
            sparse = m(*args)
            m.propagate = 'dense'
            dense = m(*args)
        close(sparse, dense.cpu(), f'{cls.__name__} sparse vs dense')


# ---- 3. saving and non-saving -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Fin,C', WIDTHS)
@pytest.mark.parametrize('name', ['T1', 'T3', 'no_edges'])
def test_forward_under_gradients_gives_the_inference_bits(name, Fin, C):
    from tgm_amd.nn import TGCN, GCNConv, gcn_graph

    ei, ew, N = on_device(name, True)
    x, H = tensors(3, (N, Fin), (N, C))
    graph = gcn_graph(ei, ew, num_nodes=N)
    for cls, extra in ((GCNConv, ()), (TGCN, (H.to(DEV),))):
        m = make(cls, Fin, C, propagate='sparse')
        for e, w in ((ei, ew), (graph, None)):
            with torch.no_grad():
                quiet = m(x.to(DEV), e, w, *extra)
            saving = m(x.to(DEV), e, w, *extra)
            assert saving.requires_grad and 'Sparse' in type(saving.grad_fn).__name__
            assert bits(saving, quiet), (cls.__name__, name)


# ---- 4. gradients -------------------------------------------------------------------------------------------------------------------------
def conv_gradients(name, Fin, C, weighted=True, improved=False, use_graph=False, seed=4):
    from tgm_amd.nn import GCNConv, gcn_graph

    ei, ew, N = on_device(name, weighted)
    want = restated(name, weighted, improved, True)
    x, w = tensors(seed, (N, Fin), (N, C))
    conv = make(GCNConv, Fin, C, improved=improved, propagate='sparse')
    p, xr = params64(conv), x.to(F64).requires_grad_(True)
    (gr.gcn_conv(want, xr, p['lin.weight'], p['bias']) * w.to(F64)).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    out = conv(xd, gcn_graph(ei, ew, num_nodes=N, improved=improved), None) if use_graph else conv(xd, ei, ew)
    (out * w.to(DEV)).sum().backward()
    return conv, xd, p, xr


@pytest.mark.parametrize('Fin,C', WIDTHS)
@pytest.mark.parametrize('name,use_graph', [('T1', False), ('T1', True), ('T3', False), ('T3', True), ('T4', False), ('all_outside', False)])
def test_conv_gradients(name, use_graph, Fin, C):
    conv, xd, p, xr = conv_gradients(name, Fin, C, use_graph=use_graph)
    for k, v in conv.named_parameters():
        gclose(v.grad, p[k].grad, f'GCNConv {name} {k}')
    gclose(xd.grad, xr.grad, f'GCNConv {name} x')


def cell_gradients(name, Fin, C, weighted, improved, use_graph=False):
    """Two snapshots with the state carried: the second snapshot's loss reaches the first through H."""
    from tgm_amd.nn import TGCN, gcn_graph

    ei, ew, N = on_device(name, weighted)
    want = restated(name, weighted, improved, True)
    cell = make(TGCN, Fin, C, improved=improved, propagate='sparse')
    p = params64(cell)
    x0, x1, H0, w = tensors(5, (N, Fin), (N, Fin), (N, C), (N, C))
    H0 = 0.3 * H0
    refs = [t.to(F64).requires_grad_(True) for t in (x0, x1, H0)]
    Hr = gr.tgcn_cell(p, want, refs[1], gr.tgcn_cell(p, want, refs[0], refs[2]))
    (Hr * w.to(F64)).sum().backward()
    devs = [t.to(DEV).requires_grad_(True) for t in (x0, x1, H0)]
    e = (gcn_graph(ei, ew, num_nodes=N, improved=improved), None) if use_graph else (ei, ew)
    Hd = cell(devs[1], *e, cell(devs[0], *e, devs[2]))
    close(Hd, Hr, f'TGCN two snapshots {name}')
    (Hd * w.to(DEV)).sum().backward()
    return cell, p, devs, refs


@pytest.mark.parametrize('Fin,C', WIDTHS)
@pytest.mark.parametrize('name,weighted,improved,use_graph', [('T1', True, True, False), ('T1', False, False, True), ('T4', True, True, False),
                                                              ('T4', True, False, True), ('T3', True, False, False)])  # fmt: skip
def test_cell_gradients_over_two_snapshots(name, weighted, improved, use_graph, Fin, C):
    cell, p, devs, refs = cell_gradients(name, Fin, C, weighted, improved, use_graph)
    for k, v in cell.named_parameters():
        gclose(v.grad, p[k].grad, f'TGCN {name} {k}')
    for tag, d, r in zip(('x0', 'x1', 'H0'), devs, refs):
        gclose(d.grad, r.grad, f'TGCN {name} {tag}')


@pytest.mark.parametrize('Fin,C', WIDTHS)
def test_two_layer_stack_sharing_one_graph(Fin, C):
    from tgm_amd.nn import GCNConv, gcn_graph

    ei, ew, N = on_device('T1', True)
    want = restated('T1', True, False, True)
    l1, l2 = make(GCNConv, Fin, C, seed=1), make(GCNConv, C, C, seed=2)  # propagate='auto': the graph selects the sparse route
    p1, p2 = params64(l1), params64(l2)
    x, w = tensors(6, (N, Fin), (N, C))
    xr = x.to(F64).requires_grad_(True)
    ref = gr.gcn_conv(want, torch.relu(gr.gcn_conv(want, xr, p1['lin.weight'], p1['bias'])), p2['lin.weight'], p2['bias'])
    (ref * w.to(F64)).sum().backward()
    graph = gcn_graph(ei, ew, num_nodes=N)
    xd = x.to(DEV).requires_grad_(True)
    out = l2(torch.relu(l1(xd, graph)), graph)
    close(out, ref, 'two layers')
    assert graph._t is None
    (out * w.to(DEV)).sum().backward()
    assert graph._t is not None  # one transpose for both layers
    for layer, p in ((l1, p1), (l2, p2)):
        for k, v in layer.named_parameters():
            gclose(v.grad, p[k].grad, f'stack {k}')
    gclose(xd.grad, xr.grad, 'stack x')


def test_composed_torch_backward(monkeypatch):
    monkeypatch.setenv('TGMX_TGCN_BWD', 'torch')
    conv, xd, p, xr = conv_gradients('T1', 3, 5)
    gclose(conv.lin.weight.grad, p['lin.weight'].grad, 'torch mode lin.weight')
    gclose(xd.grad, xr.grad, 'torch mode x')
    cell, p, devs, refs = cell_gradients('T1', 3, 5, True, False)
    for k, v in cell.named_parameters():
        gclose(v.grad, p[k].grad, f'torch mode {k}')
    gclose(devs[2].grad, refs[2].grad, 'torch mode H0')


# ---- 5. one call = per launch, 6. determinism ---------------------------------------------------------------------------------------------
def all_gradients(name, Fin, C, use_graph):
    conv, xd, _, _ = conv_gradients(name, Fin, C, use_graph=use_graph)
    cell, _, devs, _ = cell_gradients(name, Fin, C, True, False, use_graph)
    return [v.grad for v in conv.parameters()] + [xd.grad] + [v.grad for v in cell.parameters()] + [d.grad for d in devs]


@pytest.mark.parametrize('Fin,C', WIDTHS)
@pytest.mark.parametrize('name,use_graph', [('T1', False), ('T1', True), ('T3', False), ('T3', True)])
def test_one_call_backward_equals_its_launches(monkeypatch, name, use_graph, Fin, C):
    monkeypatch.delenv('TGMX_TGCN_BWD', raising=False)
    native = all_gradients(name, Fin, C, use_graph)
    monkeypatch.setenv('TGMX_TGCN_BWD', 'py')
    per_launch = all_gradients(name, Fin, C, use_graph)
    assert len(native) == len(per_launch) == 3 + 12 + 3
    for i, (a, b) in enumerate(zip(native, per_launch)):
        assert bits(a, b), i


@pytest.mark.parametrize('Fin,C', WIDTHS)
def test_backward_is_deterministic(monkeypatch, Fin, C):
    monkeypatch.delenv('TGMX_TGCN_BWD', raising=False)
    first, second = all_gradients('T3', Fin, C, False), all_gradients('T3', Fin, C, False)
    for i, (a, b) in enumerate(zip(first, second)):
        assert bits(a, b), i


# ---- 7. routing ---------------------------------------------------------------------------------------------------------------------------
def test_routing_above_the_cap(monkeypatch):
    from tgm_amd.nn import TGCN, GCNConv

    monkeypatch.delenv('TGMX_GCN_ROUTE', raising=False)
    ei, ew, N = on_device('T4', True)
    x, H = tensors(8, (N, 3), (N, 5))
    conv = make(GCNConv, 3, 5)
    with pytest.raises(NotImplementedError, match="propagate='sparse'"):
        conv(x.to(DEV), ei, ew)  # default arguments, gradients: as before
    for cls in (GCNConv, TGCN):
        with pytest.raises(NotImplementedError):
            with torch.no_grad():
                make(cls, 3, 5, propagate='dense')(x.to(DEV), ei, ew)
    with pytest.raises(NotImplementedError):
        make(TGCN, 3, 5)(x.to(DEV), ei, ew)  # default arguments, gradients
    cell = make(TGCN, 3, 5)
    with torch.no_grad():
        out = cell(x.to(DEV), ei, ew, H.to(DEV))  # default arguments, no gradients: now the sparse route
        cell.propagate = 'sparse'
        assert bits(out, cell(x.to(DEV), ei, ew, H.to(DEV)))
    conv.propagate = 'sparse'  # (test_conv_gradients checks what it computes there)
    assert conv(x.to(DEV), ei, ew).grad_fn is not None


def test_route_variable_overrides_auto_only(monkeypatch):
    from tgm_amd.nn import TGCN, GCNConv

    ei, ew, N = on_device('T1_inside', True)  # (the dense route at the end does not take ids out of range)
    x, H = tensors(9, (N, 3), (N, 5))
    for cls, extra in ((GCNConv, ()), (TGCN, (H.to(DEV),))):
        m = make(cls, 3, 5, propagate='sparse')
        monkeypatch.delenv('TGMX_GCN_ROUTE', raising=False)
        with torch.no_grad():
            want = m(x.to(DEV), ei, ew, *extra)
            m.propagate = 'auto'
            monkeypatch.setenv('TGMX_GCN_ROUTE', 'sparse')
            assert bits(m(x.to(DEV), ei, ew, *extra), want)
        assert 'Sparse' in type(m(x.to(DEV), ei, ew, *extra).grad_fn).__name__
        m.propagate = 'dense'  # the variable does not override an explicit choice
        assert 'Sparse' not in type(m(x.to(DEV), ei, ew, *extra).grad_fn).__name__


# ---- 8. check() ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grad', [False, True])
def test_check_reports_skipped_edges_once(grad):
    from tgm_amd.nn import TGCN, GCNConv, gcn_graph

    ei, ew, N = on_device('T1', True)
    x, H = tensors(10, (N, 3), (N, 5))
    with torch.set_grad_enabled(grad):
        for cls, extra in ((GCNConv, ()), (TGCN, (H.to(DEV),))):
            m = make(cls, 3, 5, propagate='sparse')
            m.check()  # nothing seen yet
            m(x.to(DEV), ei, ew, *extra)
            with pytest.raises(ValueError, match='skipped'):
                m.check()
            m.check()  # reported once
            graph = gcn_graph(ei, ew, num_nodes=N)
            m(x.to(DEV), graph, None, *extra)
            m.check()  # the graph's edges are the graph's to report
            with pytest.raises(ValueError, match='skipped'):
                graph.check()
            graph.check()
            ei_ok, ew_ok, _ = on_device('T1_inside', True)
            m(x.to(DEV), ei_ok, ew_ok, *extra)
            m.check()


# ---- 9. memory ----------------------------------------------------------------------------------------------------------------------------
def test_nothing_saved_is_n_by_n():
    from tgm_amd.nn import TGCN, GCNConv, gcn_graph

    ei, ew, N = on_device('T3', True)
    x, H = tensors(11, (N, 16), (N, 32))
    graph = gcn_graph(ei, ew, num_nodes=N)
    for cls, extra in ((GCNConv, ()), (TGCN, (H.to(DEV).requires_grad_(True),))):
        for e, w in ((ei, ew), (graph, None)):
            out = make(cls, 16, 32, propagate='sparse')(x.to(DEV).requires_grad_(True), e, w, *extra)
            fn = out.grad_fn
            assert 'Sparse' in type(fn).__name__
            held = list(fn.saved_tensors) + [t for t in fn.graph.csr]
            assert held and all(t.numel() < N * N for t in held)
            assert sum(t.numel() for t in held) < N * N // 4
