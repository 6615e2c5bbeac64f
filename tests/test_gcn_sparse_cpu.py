"""The sparse GCNConv / TGCN route, what can be checked without a device: the float64 restatement against the oracle, the ABI additions,
the argument checks of the new entry points (they fail before anything is launched), and the host-side validation of the Python surface."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gcn_sparse_restate as gr  # noqa: E402

F32 = torch.float32


def _graph(seed, N=23, E=140, weighted=True):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[:, :6] = ei[0, :6]  # explicit self loops
    ei[:, 6] = ei[:, 0]  # one node with two explicit loops: the later one's weight counts
    ei[:, 20:24] = ei[:, 30:34]  # repeated edges
    return ei, (torch.rand(E, generator=g) + 0.2 if weighted else None), g


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('improved', [False, True])
@pytest.mark.parametrize('add_self_loops', [False, True])
def test_restatement_agrees_with_the_oracle(weighted, improved, add_self_loops):
    from oracle.tgcn_ref import gcn_conv_ref, tgcn_cell_ref

    N, Fin, C = 23, 4, 5
    ei, ew, g = _graph(3, N, weighted=weighted)
    if add_self_loops and weighted:
        ew[6] = ew[0]  # the oracle assigns duplicate loop weights in an unspecified order: make the two agree
    x, W, b = torch.randn(N, Fin, generator=g), torch.randn(C, Fin, generator=g), torch.randn(C, generator=g)
    graph = gr.gcn_norm(ei, ew, N, improved, add_self_loops, dtype=F32)
    got, want = gr.gcn_conv(graph, x, W, b), gcn_conv_ref(x, ei, ew, W, b, improved, add_self_loops)
    assert (got - want).abs().max() <= 1e-6 * want.abs().max()
    p = {}
    for k in 'urc':
        p[f'conv_{k}.lin.weight'], p[f'conv_{k}.bias'] = torch.randn(C, Fin, generator=g), torch.randn(C, generator=g)
        p[f'linear_{k}.weight'], p[f'linear_{k}.bias'] = 0.3 * torch.randn(C, 2 * C, generator=g), torch.randn(C, generator=g)
    H = torch.randn(N, C, generator=g)
    got, want = gr.tgcn_cell(p, graph, x, H), tgcn_cell_ref(p, x, ei, ew, H, improved, add_self_loops)
    assert (got - want).abs().max() <= 1e-6 * want.abs().max()


def test_restatement_drops_out_of_range_edges_and_transposes():
    N = 9
    ei, ew, g = _graph(5, N, E=60)
    bad = torch.cat([ei, torch.tensor([[-1, 2], [3, N]])], dim=1)
    a = gr.gcn_norm(ei, ew, N)
    b = gr.gcn_norm(bad, torch.cat([ew, torch.ones(2)]), N)
    assert torch.equal(a.vals, b.vals) and torch.equal(a.diag, b.diag) and a.vals.dtype == torch.float64
    y, z = torch.randn(N, 3, generator=g, dtype=gr.F64), torch.randn(N, 3, generator=g, dtype=gr.F64)
    lhs, rhs = (z * gr.adj_matmul(a, y)).sum(), (gr.adj_matmul(a, z, transpose=True) * y).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * float(gr.adj_abs_matmul(a, y).abs().sum())
    assert int(gr.row_lengths(a).sum()) == int(gr.row_lengths(a, transpose=True).sum()) == a.src.numel()
    last = gr.gcn_norm(torch.tensor([[0, 0, 1], [0, 0, 0]]), torch.tensor([5.0, 7.0, 1.0]), 2)  # two loops on node 0: the later one counts
    assert torch.allclose(last.diag, torch.tensor([7.0 / 8.0, 1.0], dtype=gr.F64))


NEW = ('tgmx_csr_transpose', 'tgmx_csr_transpose_workspace_bytes', 'tgmx_gcn_conv_backward_csr', 'tgmx_gcn_conv_backward_csr_workspace_bytes',
       'tgmx_tgcn_forward_csr', 'tgmx_tgcn_gather_left', 'tgmx_tgcn_backward_csr', 'tgmx_tgcn_backward_csr_workspace_bytes')  # fmt: skip


def test_abi_additions():
    from tgm_amd import _native

    lib = _native.load()
    for name in NEW:
        assert name in _native.SIGNATURES and hasattr(lib, name)
    assert lib.tgmx_abi_sizeof(39) == ctypes.sizeof(_native.GcnConvBwd) > 0
    assert lib.tgmx_abi_sizeof(40) == ctypes.sizeof(_native.TgcnCsrFwd) > 0
    assert lib.tgmx_abi_sizeof(41) == ctypes.sizeof(_native.TgcnCsrBwd) > 0
    assert lib.tgmx_abi_sizeof(42) == 0


def test_transpose_rejects_bad_arguments():
    from tgm_amd import _native

    lib = _native.load()
    x = 0x1000  # (never dereferenced: the calls return before any launch)
    big = 1 << 20
    E_INVALID = lib.tgmx_csr_transpose(None, x, x, x, 4, 5, x, x, x, None, x, big, None)
    assert E_INVALID != 0 and b'csr_transpose' in lib.tgmx_last_error()
    assert lib.tgmx_csr_transpose(x, None, x, x, 4, 5, x, x, x, None, x, big, None) == E_INVALID  # cols with nnz > 0
    assert lib.tgmx_csr_transpose(x, x, x, x, 0, 5, x, x, x, None, x, big, None) == E_INVALID  # N = 0
    assert lib.tgmx_csr_transpose(x, x, x, x, 4, 1 << 31, x, x, x, None, x, big, None) == E_INVALID  # nnz >= 2^31
    assert lib.tgmx_csr_transpose(x, x, x, x, 1 << 31, 5, x, x, x, None, x, big, None) == E_INVALID  # N >= 2^31
    assert lib.tgmx_csr_transpose(x, x, x, None, 4, 5, x, x, x, x, x, big, None) == E_INVALID  # a diagonal to copy from nowhere
    assert lib.tgmx_csr_transpose(x, x, x, x, 4, 5, x, x, x, None, x, 16, None) == E_INVALID and b'workspace too small' in lib.tgmx_last_error()
    assert lib.tgmx_csr_transpose_workspace_bytes(5, 0) == 0 and lib.tgmx_csr_transpose_workspace_bytes(1 << 31, 4) == 0
    assert lib.tgmx_csr_transpose_workspace_bytes(5, 4) > 0 and lib.tgmx_csr_transpose_workspace_bytes(0, 4) > 0
    assert lib.tgmx_tgcn_gather_left(None, x, x, 3, 4, x, None) == E_INVALID
    assert lib.tgmx_tgcn_gather_left(x, x, x, 0, 4, x, None) == E_INVALID
    assert lib.tgmx_tgcn_gather_left(x, x, x, 3, 0, x, None) == 0  # N = 0: nothing to do


def test_conv_backward_rejects_bad_arguments():
    from tgm_amd import _native

    lib = _native.load()
    x = 0x1000
    E_INVALID = lib.tgmx_gcn_conv_backward_csr(None, None)
    assert E_INVALID != 0 and lib.tgmx_gcn_conv_backward_csr_workspace_bytes(None) == 0
    t = _native.GcnConvBwd()
    assert lib.tgmx_gcn_conv_backward_csr(ctypes.byref(t), None) == E_INVALID and b'bad sizes' in lib.tgmx_last_error()  # N = 0
    t.N, t.in_ch, t.C, t.nnz, t.lddo = 10, 4, 3, 7, 2
    assert lib.tgmx_gcn_conv_backward_csr(ctypes.byref(t), None) == E_INVALID and b'leading dimension' in lib.tgmx_last_error()
    t.lddo = 3
    t.d_x = x
    assert lib.tgmx_gcn_conv_backward_csr(ctypes.byref(t), None) == E_INVALID and b'transposed weight' in lib.tgmx_last_error()
    t.WT, t.ldwt = x, 2
    assert lib.tgmx_gcn_conv_backward_csr(ctypes.byref(t), None) == E_INVALID and b'transposed weight' in lib.tgmx_last_error()  # ldwt < C
    t.ldwt = 3
    assert lib.tgmx_gcn_conv_backward_csr(ctypes.byref(t), None) == E_INVALID and b'null pointer' in lib.tgmx_last_error()  # dout, diag
    t.dout = t.diag = x
    assert lib.tgmx_gcn_conv_backward_csr(ctypes.byref(t), None) == E_INVALID and b'CSR is missing' in lib.tgmx_last_error()
    t.indptr = t.cols = t.vals = x
    need = lib.tgmx_gcn_conv_backward_csr_workspace_bytes(ctypes.byref(t))
    assert need > 0
    assert lib.tgmx_gcn_conv_backward_csr(ctypes.byref(t), None) == E_INVALID and b'workspace too small' in lib.tgmx_last_error()
    t.workspace, t.workspace_bytes = x, need - 1
    assert lib.tgmx_gcn_conv_backward_csr(ctypes.byref(t), None) == E_INVALID and b'workspace too small' in lib.tgmx_last_error()
    t.indptr_t = x  # a transposed CSR handed in without its entries
    assert lib.tgmx_gcn_conv_backward_csr(ctypes.byref(t), None) == E_INVALID and b'incomplete' in lib.tgmx_last_error()
    t.cols_t = t.vals_t = x
    assert 0 < lib.tgmx_gcn_conv_backward_csr_workspace_bytes(ctypes.byref(t)) < need  # nothing to transpose then


def test_cell_forward_rejects_bad_arguments():
    from tgm_amd import _native

    lib = _native.load()
    x = 0x1000
    E_INVALID = lib.tgmx_tgcn_forward_csr(None, None)
    assert E_INVALID != 0
    a = _native.TgcnCsrFwd()
    assert lib.tgmx_tgcn_forward_csr(ctypes.byref(a), None) == E_INVALID and b'bad sizes' in lib.tgmx_last_error()  # N = 0
    a.N, a.in_ch, a.C, a.E, a.ldx, a.ldw3 = 10, 4, 3, 7, 3, 4
    assert lib.tgmx_tgcn_forward_csr(ctypes.byref(a), None) == E_INVALID and b'leading dimension' in lib.tgmx_last_error()  # ldx < in_ch
    a.ldx = 4
    assert lib.tgmx_tgcn_forward_csr(ctypes.byref(a), None) == E_INVALID and b'null pointer' in lib.tgmx_last_error()
    a.x = a.W3 = a.b3 = a.H = a.indptr = a.cols = a.vals = a.diag = a.xw = a.G = a.out = x
    assert lib.tgmx_tgcn_forward_csr(ctypes.byref(a), None) == E_INVALID and b'edge list' in lib.tgmx_last_error()  # not built, no edges
    a.csr_built = 1
    assert lib.tgmx_tgcn_forward_csr(ctypes.byref(a), None) == E_INVALID and b'gate 0' in lib.tgmx_last_error()
    for g in range(3):
        a.lin_w[g] = a.lin_b[g] = a.pre[g] = x
    a.cat[0] = x
    a.save = 1  # the saving form needs all three cat buffers
    assert lib.tgmx_tgcn_forward_csr(ctypes.byref(a), None) == E_INVALID and b'gate 1' in lib.tgmx_last_error()


def test_cell_backward_rejects_bad_arguments():
    from tgm_amd import _native

    lib = _native.load()
    x = 0x1000
    E_INVALID = lib.tgmx_tgcn_backward_csr(None, None)
    assert E_INVALID != 0 and lib.tgmx_tgcn_backward_csr_workspace_bytes(None) == 0
    t = _native.TgcnCsrBwd()
    assert lib.tgmx_tgcn_backward_csr(ctypes.byref(t), None) == E_INVALID and b'bad sizes' in lib.tgmx_last_error()  # N = 0
    t.N, t.in_ch, t.C, t.nnz, t.ldx = 10, 4, 3, 7, 3
    assert lib.tgmx_tgcn_backward_csr(ctypes.byref(t), None) == E_INVALID and b'below in_ch' in lib.tgmx_last_error()
    t.ldx = 4
    t.d_x = x
    t.W3T, t.ldw3t = x, 8
    assert lib.tgmx_tgcn_backward_csr(ctypes.byref(t), None) == E_INVALID and b'transposed stacked' in lib.tgmx_last_error()  # ldw3t < 3C
    t.ldw3t = 9
    small = lib.tgmx_tgcn_backward_csr_workspace_bytes(ctypes.byref(t))
    assert small > 0
    assert lib.tgmx_tgcn_backward_csr(ctypes.byref(t), None) == E_INVALID and b'null pointer' in lib.tgmx_last_error()
    t.dout = t.H = t.diag = x
    assert lib.tgmx_tgcn_backward_csr(ctypes.byref(t), None) == E_INVALID and b'saved buffers' in lib.tgmx_last_error()
    for g in range(3):
        t.cat[g] = t.pre[g] = t.lin_wT[g] = x
    t.d_W3 = x
    assert lib.tgmx_tgcn_backward_csr(ctypes.byref(t), None) == E_INVALID and b'needs x' in lib.tgmx_last_error()
    t.x = x
    assert lib.tgmx_tgcn_backward_csr(ctypes.byref(t), None) == E_INVALID and b'CSR is missing' in lib.tgmx_last_error()
    t.indptr = t.cols = t.vals = x
    assert lib.tgmx_tgcn_backward_csr(ctypes.byref(t), None) == E_INVALID and b'workspace too small' in lib.tgmx_last_error()
    t.indptr_t = t.cols_t = t.vals_t = x
    assert 0 < lib.tgmx_tgcn_backward_csr_workspace_bytes(ctypes.byref(t)) < small  # the transpose is handed in: nothing to sort


def test_propagate_keyword_and_route(monkeypatch):
    from tgm_amd.nn import TGCN, GCNConv, _gcn_sparse_train as st

    for cls in (GCNConv, TGCN):
        assert cls(3, 4).propagate == 'auto' and cls(3, 4, propagate='sparse').propagate == 'sparse' and cls(3, 4, cached=True).cached
        for bad in ('csr', 'Sparse', None, 1):
            with pytest.raises(ValueError, match='propagate'):
                cls(3, 4, propagate=bad)
    monkeypatch.delenv('TGMX_GCN_ROUTE', raising=False)
    assert [st.route(r) for r in st.ROUTES] == ['auto', 'dense', 'sparse']
    monkeypatch.setenv('TGMX_GCN_ROUTE', 'sparse')
    assert [st.route(r) for r in st.ROUTES] == ['sparse', 'dense', 'sparse']  # the variable overrides 'auto' only
    monkeypatch.setenv('TGMX_GCN_ROUTE', 'dense')
    assert [st.route(r) for r in st.ROUTES] == ['dense', 'dense', 'sparse']
    monkeypatch.setenv('TGMX_GCN_ROUTE', 'SPARSE')
    assert st.route('auto') == 'auto'
    monkeypatch.delenv('TGMX_TGCN_BWD', raising=False)
    assert st.mode() == 'native'
    for value, want in (('py', 'py'), ('torch', 'torch'), ('', 'native'), ('PY', 'native')):
        monkeypatch.setenv('TGMX_TGCN_BWD', value)
        assert st.mode() == want


def test_gcn_graph_validates_on_the_host():
    from tgm_amd.nn import TGCN, GCNConv, GCNGraph, gcn_graph

    ei = torch.tensor([[0, 1], [1, 2]])
    for bad in (None, 0, -3, 2.0, True):
        with pytest.raises(ValueError, match='num_nodes'):
            gcn_graph(ei, num_nodes=bad)
    g = GCNGraph(None, 3, 2, improved=False, add_self_loops=True, device=torch.device('cpu'))
    x = torch.randn(3, 4)
    for module in (GCNConv(4, 5, improved=True), TGCN(4, 5, add_self_loops=False)):
        with pytest.raises(ValueError, match='GCNGraph built'):
            module(x, g)
    with pytest.raises(ValueError, match='edge_weight must be None'):
        GCNConv(4, 5)(x, g, torch.ones(2))
    with pytest.raises(ValueError, match='3 nodes'):
        TGCN(4, 5)(torch.randn(6, 4), g)


def test_sparse_route_has_no_cpu_fallback():
    from tgm_amd.exceptions import NativeLibraryError
    from tgm_amd.nn import TGCN, GCNConv, gcn_graph

    ei, x = torch.tensor([[0, 1], [1, 2]]), torch.randn(3, 4)
    with pytest.raises(NativeLibraryError):
        GCNConv(4, 5, propagate='sparse')(x, ei)
    with pytest.raises(NativeLibraryError):
        TGCN(4, 5, propagate='sparse')(x, ei)
    with pytest.raises(NativeLibraryError):
        gcn_graph(ei, num_nodes=3)
