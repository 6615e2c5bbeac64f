"""ChebConv / GCLSTM on the device against the float64 restatement (tests/gclstm_restate.py): the reference's recorded recurrences (g23
fixtures), the gather SpMM at the widths and row lengths that reach each of its branches, determinism, the one-call forward against the
cell composed from its parts, the training path's gradients and the example's loop."""
import copy

import pytest
import torch

import gclstm_restate as gr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# The parity bar of tests/test_ctan_gpu.py.  Ratio: the device's distance from the float64 restatement against the float32 restatement's
# own, 2.0 wherever the latter is measurable (>= 1e-7).  Absolute: close()'s 1e-5 of max(1, |ref|).
RATIO_BAR, NOISE_FLOOR, ABS_BAR = 2.0, 1e-7, 1e-5
LONG_ROW = 64  # kChebLongRow (csrc/cheb.hip): longer rows are split over the four waves of a workgroup


def dev(v):
    return None if v is None else v.to(DEV)


def bar(got, ref, f32, label):
    got = got.detach().cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32 and torch.isfinite(got).all(), label
    d_hip, d_f32 = gr.rel_err(got, ref), gr.rel_err(f32, ref)
    print(f'gclstm parity {label}: hip {d_hip:.3e} float32 {d_f32:.3e} ratio {d_hip / max(d_f32, 1e-30):.2f}')
    assert d_hip <= ABS_BAR, (label, d_hip)
    if d_f32 >= NOISE_FLOOR:
        assert d_hip <= RATIO_BAR * d_f32, (label, d_hip, d_f32)


def make_cell(meta, params):
    from tgm_amd.nn import GCLSTM

    cell = GCLSTM(meta['in_channels'], meta['out_channels'], meta['K'], normalization=meta['normalization'], bias=meta['bias'])
    cell.load_state_dict(params, strict=True)
    return cell.to(DEV).eval()


# ---- the reference's recorded recurrences ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', gr.EXPECTED_FIXTURES)
def test_fixture_recurrence(name):
    meta, params, snaps = gr.load_fixture(name)
    cell = make_cell(meta, params)
    norm = meta['normalization']
    runs = {}
    for idx in (torch.int64, torch.int32):
        step = lambda x, ei, ew, H, C, lm: cell(dev(x), dev(ei.to(idx)), dev(ew), H, C, lm)
        with torch.no_grad():
            runs[idx] = [(H.cpu(), C.cpu()) for _, H, C in gr.replay(meta, snaps, step)]
    cell.check()
    ref = list(gr.replay(meta, snaps, lambda x, ei, ew, H, C, lm: gr.gclstm_forward(params, x, ei, ew, H, C, lm, norm)))
    f32 = list(gr.replay(meta, snaps, lambda x, ei, ew, H, C, lm: gr.gclstm_forward(params, x, ei, ew, H, C, lm, norm, dtype=torch.float32)))
    for s, snap in enumerate(snaps):
        for j, tag in enumerate('HC'):
            assert torch.equal(runs[torch.int64][s][j], runs[torch.int32][s][j]), (name, s, tag)  # int32 ids are read as they are
            gr.close(runs[torch.int64][s][j], snap[tag], f'{name} {tag}{s} against the record')
            bar(runs[torch.int64][s][j], ref[s][1 + j], f32[s][1 + j], f'{name} {tag}{s}')


# ---- ChebConv alone ----------------------------------------------------------------------------------------------------------------------------
def conv_case(seed, N, cin, cout, K, ei, ew=None, normalization='sym', lambda_max=None, bias=True):
    from tgm_amd.nn import ChebConv

    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    conv = ChebConv(cin, cout, K, normalization=normalization, bias=bias)
    if bias:
        with torch.no_grad():
            conv.bias.uniform_(-0.5, 0.5, generator=g)
    x = torch.randn(N, cin, generator=g)
    return conv, x, ei, ew, normalization, lambda_max


def conv_parity(case, label, edge_index=None):
    conv, x, ei, ew, norm, lm = case
    ws, b = [l.weight.detach().clone() for l in conv.lins], None if conv.bias is None else conv.bias.detach().clone()
    ref = gr.cheb_conv(ws, b, x, ei, ew, norm, lm)
    f32 = gr.cheb_conv(ws, b, x, ei, ew, norm, lm, dtype=torch.float32)
    conv = conv.to(DEV).eval()
    with torch.no_grad():
        got = conv(dev(x), dev(ei) if edge_index is None else edge_index, dev(ew), lm)
    conv.check()
    bar(got, ref, f32, label)
    return got


def rand_graph(seed, N, E, weighted=True):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N, (2, E), generator=g)  # directed, with repeats and self loops
    return ei, (torch.rand(E, generator=g) + 0.5 if weighted else None)


@pytest.mark.parametrize('C', [1, 5, 64, 256, 260])
@pytest.mark.parametrize('K', [1, 2, 3, 4])
def test_chebconv_widths(C, K):
    """Scalar lanes with a tail (1, 5), one float4 a lane short of a pass (64), exactly one pass (256), a second pass (260); in != out."""
    ei, ew = rand_graph(C, 150, 700)
    conv_parity(conv_case(100 * K + C, 150, C, 7 if C != 7 else 9, K, ei, ew), f'C={C} K={K}')


@pytest.mark.parametrize('cin,K', [(5, 3), (6, 3), (3, 2)])
def test_chebconv_operand_width_not_a_multiple_of_four(cin, K):
    """K in = 15, 18, 6: the basis slices start off the 16-byte grid, so the propagate takes its scalar lanes and the GEMM its padded rows."""
    ei, ew = rand_graph(cin, 90, 400, weighted=False)
    conv_parity(conv_case(7 + cin, 90, cin, 12, K, ei, ew), f'in={cin} K={K}')


def hub_graph(N, hub_in, weighted):
    """node 0: hub_in distinct sources; node 1: one incoming edge; node 2: none (it only sends); the rest a sparse random graph"""
    assert N >= hub_in + 3
    g = torch.Generator().manual_seed(hub_in)
    src = torch.arange(3, 3 + hub_in)
    # (the hub sends one edge too: with 'sym' a node without outgoing edges has degree 0 and every entry of its row would be 0)
    ei = torch.stack([torch.cat([src, torch.tensor([2, 2, 1, 0])]), torch.cat([torch.zeros(hub_in, dtype=torch.int64), torch.tensor([1, 5, 7, 9])])])
    extra = torch.randint(3, N, (2, 2 * N), generator=g)
    ei = torch.cat([ei, extra], dim=1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    indeg = torch.bincount(ei[1][ei[0] != ei[1]], minlength=N)
    assert indeg[0] == hub_in and indeg[1] == 1 and indeg[2] == 0
    return ei, (torch.rand(ei.shape[1], generator=g) + 0.5 if weighted else None)


@pytest.mark.parametrize('C', [5, 64, 260])
@pytest.mark.parametrize('normalization,lambda_max', [('sym', None), ('rw', 2.3)])
def test_chebconv_row_lengths(C, normalization, lambda_max):
    """In-degree 0, 1 and 70 = the long-row threshold + 6: the hub's row is split over four waves (pieces of 18, 18, 18, 16)."""
    assert LONG_ROW + 6 == 70
    ei, ew = hub_graph(100, 70, weighted=normalization == 'rw')
    conv_parity(conv_case(C, 100, C, C, 3, ei, ew, normalization, lambda_max), f'hub C={C} {normalization}')


def test_chebconv_row_at_the_threshold_and_a_long_hub():
    for hub_in in (LONG_ROW, LONG_ROW + 1, 1000):
        ei, ew = hub_graph(1100, hub_in, weighted=True)
        conv_parity(conv_case(hub_in, 1100, 8, 8, 3, ei, ew, None, 40.0), f'hub of {hub_in}')


VERY_LONG, CHUNK = 2048, 1024  # kChebVeryLong, kChebChunk: longer rows are summed chunk by chunk of the entry array, a workgroup a chunk


@pytest.mark.parametrize('C', [5, 8, 260])
def test_chebconv_very_long_rows(C):
    """A hub at the very-long threshold, one past it, and one of 5 000 entries (five chunks, the first and the last partial).  No
    normalisation with lambda_max = the hub's length keeps L_hat of order one: under 'sym' / 'rw' a row of thousands of order-one entries
    puts values of order 100 beside values of order one, and the float32 restatement itself then misses the absolute bar."""
    for hub_in in (VERY_LONG, VERY_LONG + 1, 5000):
        ei, ew = hub_graph(hub_in + 40, hub_in, weighted=True)
        conv_parity(conv_case(hub_in + C, hub_in + 40, C, 6, 3, ei, ew, None, float(hub_in)), f'very long hub of {hub_in} C={C}')


@pytest.mark.parametrize('weighted', [False, True])
def test_chebconv_two_very_long_rows_share_a_chunk(weighted):
    """Rows 0 and 1 of 3 000 entries each (sources repeat): chunk 2 of the entry array holds the end of one and the start of the other;
    rows 6 and 7 of 2 500 follow after a short row, and node 9 has a row of 100.  (No normalisation, lambda_max = the longest row: see
    test_chebconv_very_long_rows.)"""
    g = torch.Generator().manual_seed(77)
    N = 400
    parts = [(0, 3000), (1, 3000), (5, 7), (6, 2500), (7, 2500), (9, 100)]
    dst = torch.cat([torch.full((n,), d, dtype=torch.int64) for d, n in parts])
    src = torch.randint(10, N, (dst.numel(),), generator=g)
    back = torch.stack([torch.tensor([0, 1, 5, 6, 7, 9]), torch.tensor([20, 21, 22, 23, 24, 25])])  # the hubs send too ('sym' needs their degree)
    ei = torch.cat([torch.stack([src, dst]), back, torch.randint(10, N, (2, 600), generator=g)], dim=1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    ew = torch.rand(ei.shape[1], generator=g) + 0.5 if weighted else None
    assert (3000 // CHUNK) == (3000 + 10) // CHUNK == 2
    for C in (8, 7, 260):
        conv_parity(conv_case(C, N, C, 5, 4, ei, ew, None, 3000.0), f'two hubs in a chunk C={C}')


def test_chebconv_degenerate_graphs():
    empty = torch.zeros((2, 0), dtype=torch.int64)
    conv_parity(conv_case(1, 1, 4, 3, 3, empty), 'N=1 E=0')
    conv_parity(conv_case(2, 1, 4, 3, 3, torch.zeros((2, 3), dtype=torch.int64), torch.tensor([1.0, 2.0, 3.0])), 'N=1 self loops')
    conv_parity(conv_case(3, 9, 4, 3, 4, empty), 'E=0')
    conv_parity(conv_case(4, 9, 4, 3, 4, empty, None, None, 3.0), 'E=0 no normalisation')
    loops = torch.arange(9).repeat(2, 2)
    conv_parity(conv_case(5, 9, 4, 3, 3, loops, torch.rand(18) + 0.5), 'self loops only')
    conv_parity(conv_case(6, 9, 4, 3, 2, loops, None, 'rw', 1.5, bias=False), 'self loops only, rw, no bias')


def test_chebconv_transposed_edge_index_view():
    ei, ew = rand_graph(11, 60, 300)
    pairs = dev(ei.t().contiguous())  # [E, 2]: its transpose is a non-contiguous [2, E] view
    view = pairs.t()
    assert not view.is_contiguous() and not view[0].is_contiguous()
    a = conv_parity(conv_case(12, 60, 8, 8, 3, ei, ew), 'transposed view', edge_index=view)
    b = conv_parity(conv_case(12, 60, 8, 8, 3, ei, ew), 'contiguous')
    c = conv_parity(conv_case(12, 60, 8, 8, 3, ei, ew), 'int32 view', edge_index=pairs.to(torch.int32).t())
    assert torch.equal(a, b) and torch.equal(a, c)


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    from tgm_amd.nn import GCLSTM

    N, E, C, K = 300, 4000, 64, 3
    g = torch.Generator().manual_seed(9)
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[1, :500] = 0  # a hub (the four-wave split)
    ei[1, 1200:3400] = 7  # and a very long row (the chunk launches)
    ei[:, 600:900] = ei[:, 900:1200]  # duplicates
    ew = torch.rand(E, generator=g) + 0.1
    torch.manual_seed(9)
    cell = GCLSTM(32, C, K).to(DEV).eval()
    x, H0, C0 = (torch.randn(N, d, generator=g).to(DEV) for d in (32, C, C))
    with torch.no_grad():
        a = cell(x, dev(ei), dev(ew), H0, C0)
        b = cell(x, dev(ei), dev(ew), H0, C0)
        c = copy.deepcopy(cell)(x, dev(ei), dev(ew), H0, C0)  # its own scratch and sort workspace
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    assert torch.isfinite(a[0]).all() and a[0].abs().max() > 0


# ---- one call against the composition --------------------------------------------------------------------------------------------------------------
def composed_from_parts(cell, x, ei, ew, H, C, lm):
    """The cell from four ChebConv calls (native), matmul and torch pointwise ops."""
    pre = [torch.matmul(x, W) + conv(H, ei, ew, lm) + b for W, b, conv in cell._gates()]
    I, F, T, O = torch.sigmoid(pre[0]), torch.sigmoid(pre[1]), torch.tanh(pre[2]), torch.sigmoid(pre[3])
    C = F * C + I * T
    return O * torch.tanh(C), C


def run_snapshots(cell, seed, N, sizes, norm, lm, label):
    g = torch.Generator().manual_seed(seed)
    sd = {k: v.detach().cpu().clone() for k, v in cell.state_dict().items()}
    cin, Co = cell.in_channels, cell.out_channels
    H = C = Hp = Cp = H64 = C64 = H32 = C32 = None
    for s, E in enumerate(sizes):
        x = torch.randn(N, cin, generator=g)
        ei = torch.randint(0, N, (2, E), generator=g)
        ew = torch.rand(E, generator=g) + 0.5 if s % 2 == 0 else None
        with torch.no_grad():
            H, C = cell(dev(x), dev(ei), dev(ew), H, C, lm)
            zeros = torch.zeros(N, Co, device=DEV)
            Hp, Cp = composed_from_parts(cell, dev(x), dev(ei), dev(ew), zeros if Hp is None else Hp, zeros if Cp is None else Cp, lm)
        H64, C64 = gr.gclstm_forward(sd, x, ei, ew, H64, C64, lm, norm)
        H32, C32 = gr.gclstm_forward(sd, x, ei, ew, H32, C32, lm, norm, dtype=torch.float32)
        for got, parts, ref, f32, tag in ((H, Hp, H64, H32, 'H'), (C, Cp, C64, C32, 'C')):
            bar(got, ref, f32, f'{label} one call {tag}{s} E={E}')
            bar(parts, ref, f32, f'{label} from parts {tag}{s} E={E}')
            gr.close(got.cpu(), parts.cpu(), f'{label} one call against the parts {tag}{s}')
    cell.check()


@pytest.mark.parametrize('norm,lm', [('sym', None), (None, 60.0)])  # (60: about twice the largest weighted degree, so L_hat stays of order one)
def test_one_call_against_the_composition(norm, lm):
    from tgm_amd.nn import GCLSTM

    torch.manual_seed(21)
    cell = GCLSTM(6, 5, 3, normalization=norm).to(DEV).eval()  # operand width 6 + 3 * 5 = 21: padded to 24
    with torch.no_grad():
        for g in 'ifco':
            getattr(cell, f'conv_{g}').bias.uniform_(-0.3, 0.3)
            getattr(cell, f'b_{g}').uniform_(-0.3, 0.3)
    sizes = [40, 0, 200, 90, 1500]  # an empty snapshot, and one larger than any before: the scratch regrows
    run_snapshots(cell, 1, 120, sizes, norm, lm, 'fresh')
    with torch.no_grad():  # the cached stacked weight must follow an in-place update
        cell.W_i.add_(0.25)
        cell.conv_f.lins[2].weight.mul_(-1.5)
        cell.conv_o.bias.add_(0.4)
        cell.b_c.sub_(0.2)
    run_snapshots(cell, 2, 120, sizes[::-1], norm, lm, 'updated')
    twin = copy.deepcopy(cell)
    with torch.no_grad():
        twin.W_c.mul_(0.5)
    run_snapshots(twin, 3, 120, [60, 300], norm, lm, 'deepcopy')
    run_snapshots(cell, 3, 77, [60, 300], norm, lm, 'original after the copy, another N')


# ---- lambda_max ----------------------------------------------------------------------------------------------------------------------------------
def test_lambda_max_as_a_float_and_as_a_device_tensor():
    from tgm_amd.nn import GCLSTM, ChebConv

    ei, ew = rand_graph(31, 50, 300)
    torch.manual_seed(31)
    x = torch.randn(50, 8).to(DEV)
    for norm in ('rw', None, 'sym'):
        conv, cell = ChebConv(8, 8, 3, normalization=norm).to(DEV).eval(), GCLSTM(8, 6, 3, normalization=norm).to(DEV).eval()
        lam_t, ei_d, ew_d = torch.tensor(2.75, device=DEV), dev(ei), dev(ew)
        lam_1 = lam_t.reshape(1)
        with torch.no_grad():
            a, (ha, ca) = conv(x, ei_d, ew_d, 2.75), cell(x, ei_d, ew_d, lambda_max=2.75)
            torch.cuda.synchronize()
            mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode('error')  # a read back of the tensor would raise here
            try:
                b, (hb, cb) = conv(x, ei_d, ew_d, lam_t), cell(x, ei_d, ew_d, lambda_max=lam_1)
            finally:
                torch.cuda.set_sync_debug_mode(mode)
            c = conv(x, ei_d, ew_d, torch.tensor(2.75))  # a host tensor is a number
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(ha, hb) and torch.equal(ca, cb)
        ref = gr.cheb_conv([l.weight.detach().cpu() for l in conv.lins], conv.bias.detach().cpu(), x.cpu(), ei, ew, norm, 2.75)
        f32 = gr.cheb_conv([l.weight.detach().cpu() for l in conv.lins], conv.bias.detach().cpu(), x.cpu(), ei, ew, norm, 2.75, dtype=torch.float32)
        bar(a, ref, f32, f'lambda_max 2.75 {norm}')
    with pytest.raises(ValueError, match='lambda_max'):
        GCLSTM(8, 6, 2, normalization='rw').to(DEV).eval()(x, dev(ei))
    with pytest.raises(NotImplementedError):
        ChebConv(8, 8, 2).to(DEV).eval()(x, dev(ei), None, torch.tensor([2.0, 2.0], device=DEV))


# ---- training ------------------------------------------------------------------------------------------------------------------------------------
def test_training_path_gradients_against_float64_autograd():
    from tgm_amd.nn import GCLSTM

    N, cin, Co, K = 40, 6, 8, 3
    g = torch.Generator().manual_seed(41)
    torch.manual_seed(41)
    cell = GCLSTM(cin, Co, K).to(DEV).train()
    with torch.no_grad():
        for p in cell.parameters():
            p.uniform_(-0.5, 0.5)
    snaps = [(torch.randn(N, cin, generator=g), torch.randint(0, N, (2, E), generator=g), torch.rand(E, generator=g) + 0.5) for E in (150, 90)]
    H0, C0 = torch.randn(N, Co, generator=g) * 0.5, torch.randn(N, Co, generator=g) * 0.5
    wH, wC = torch.randn(N, Co, generator=g), torch.randn(N, Co, generator=g)

    # float64 autograd through the restatement
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in cell.state_dict().items()}
    xs64 = [x.double().requires_grad_(True) for x, _, _ in snaps]
    H64, C64 = H0.double().requires_grad_(True), C0.double().requires_grad_(True)
    H, C = H64, C64
    for x64, (_, ei, ew) in zip(xs64, snaps):
        H, C = gr.gclstm_forward(sd, x64, ei, ew, H, C)
    ((H * wH.double()).sum() + (C * wC.double()).sum()).backward()
    H_ref, C_ref = H.detach(), C.detach()

    xs = [dev(x).requires_grad_(True) for x, _, _ in snaps]
    Hd, Cd = dev(H0).requires_grad_(True), dev(C0).requires_grad_(True)
    H, C = Hd, Cd
    for xd, (_, ei, ew) in zip(xs, snaps):
        H, C = cell(xd, dev(ei), dev(ew), H, C)
    assert H.requires_grad and C.requires_grad
    ((H * dev(wH)).sum() + (C * dev(wC)).sum()).backward()
    pairs = [(p.grad, sd[k].grad, k) for k, p in cell.named_parameters()]
    pairs += [(xs[0].grad, xs64[0].grad, 'node_x (snapshot 0)'), (xs[1].grad, xs64[1].grad, 'node_x (snapshot 1)'), (Hd.grad, H64.grad, 'H0'), (Cd.grad, C64.grad, 'C0')]
    assert len(pairs) == 4 * (2 + K + 1) + 4
    for got, ref, tag in pairs:
        assert got is not None and ref is not None, tag
        err, scale = (got.cpu().double() - ref).abs().max().item(), ref.abs().max().item()
        print(f'gclstm gradient {tag}: {err:.3e} of {scale:.3e}')
        assert scale > 0 and err <= 1e-4 * scale, f'{tag}: {err:.3e} vs {scale:.3e}'

    # the grad-enabled forward and the no-grad one hold the same bar
    with torch.no_grad():
        Hn, Cn = dev(H0), dev(C0)
        for x, ei, ew in snaps:
            Hn, Cn = cell(dev(x), dev(ei), dev(ew), Hn, Cn)
    H32, C32 = H0, C0
    sd32 = {k: v.detach().cpu() for k, v in cell.state_dict().items()}
    for x, ei, ew in snaps:
        H32, C32 = gr.gclstm_forward(sd32, x, ei, ew, H32, C32, dtype=torch.float32)
    for got, ref, f32, tag in ((H, H_ref, H32, 'H grad'), (C, C_ref, C32, 'C grad'), (Hn, H_ref, H32, 'H no-grad'), (Cn, C_ref, C32, 'C no-grad')):
        bar(got, ref, f32, f'training {tag}')


# ---- an edge outside the node table ----------------------------------------------------------------------------------------------------------------
def test_out_of_range_edge_is_skipped_and_reported_once():
    from tgm_amd.nn import GCLSTM, ChebConv

    torch.manual_seed(51)
    x = torch.randn(6, 4).to(DEV)
    good = torch.tensor([[0, 1, 2, 3, 4, 1], [1, 2, 3, 4, 5, 0]])
    for bad_edge in ([2, 9], [9, 2], [-1, 3]):  # node 9 of 6
        bad = torch.cat([good[:, :3], torch.tensor([bad_edge]).t(), good[:, 3:]], dim=1)
        w_good = torch.rand(6) + 0.5
        w_bad = torch.cat([w_good[:3], torch.tensor([5.0]), w_good[3:]])
        for mod in (GCLSTM(4, 3, 2).to(DEV).eval(), ChebConv(4, 3, 3).to(DEV).eval()):
            for idx in (torch.int64, torch.int32):
                with torch.no_grad():
                    want = mod(x, dev(good.to(idx)), dev(w_good))
                    mod.check()
                    got = mod(x, dev(bad.to(idx)), dev(w_bad))  # the call returns
                for a, b in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
                    assert torch.equal(a, b)
                with pytest.raises(ValueError, match='outside'):
                    mod.check()
                mod.check()  # reported once


# ---- the example's loop ----------------------------------------------------------------------------------------------------------------------------
class RecurrentGCN(torch.nn.Module):
    """examples/linkproppred/gclstm.py:47-70 over tgm_amd."""

    def __init__(self, node_dim, embed_dim, K=1):
        from tgm_amd.nn import GCLSTM

        super().__init__()
        self.recurrent = GCLSTM(in_channels=node_dim, out_channels=embed_dim, K=K)
        self.linear = torch.nn.Linear(embed_dim, embed_dim)

    def forward(self, batch, node_feat, h=None, c=None):
        edge_index = torch.stack([batch.edge_src, batch.edge_dst], dim=0)
        edge_weight = batch.edge_weight if hasattr(batch, 'edge_weight') else None
        h_0, c_0 = self.recurrent(node_feat, edge_index, edge_weight, h, c)
        return self.linear(torch.nn.functional.relu(h_0)), h_0, c_0


@pytest.mark.parametrize('K', [1, 2])
def test_example_loop_over_discretized_snapshots(K):
    from tgm_amd import DGData, DGDataLoader, DGraph
    from tgm_amd.synth import make_stream

    s = make_stream('wiki', seed=23, num_edges=900, n_src=40, n_dst=20, edge_dim=0, node_dim=8, t_hi=3 * 3600 - 1)
    data = DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1), None, static_node_x=s.node_x, time_delta='s').discretize('h', device=DEV)
    dg = DGraph(data, device=DEV)
    torch.manual_seed(23)
    model = RecurrentGCN(8, 16, K=K).to(DEV).eval()
    sd = {k[len('recurrent.') :]: v.detach().cpu() for k, v in model.state_dict().items() if k.startswith('recurrent.')}
    lin_w, lin_b = model.linear.weight.detach().cpu().double(), model.linear.bias.detach().cpu().double()
    h = c = h64 = c64 = h32 = c32 = None
    n = 0
    with torch.no_grad():
        for batch in DGDataLoader(dg, batch_unit='h'):
            z, h, c = model(batch, dg.static_node_x, h, c)
            ei = torch.stack([batch.edge_src, batch.edge_dst]).cpu()
            assert ei.shape[1] > 0
            h64, c64 = gr.gclstm_forward(sd, s.node_x, ei, None, h64, c64)
            h32, c32 = gr.gclstm_forward(sd, s.node_x, ei, None, h32, c32, dtype=torch.float32)
            bar(h, h64, h32, f'example K={K} h{n}')
            bar(c, c64, c32, f'example K={K} c{n}')
            z64 = torch.relu(h64) @ lin_w.t() + lin_b
            assert torch.isfinite(z).all() and gr.rel_err(z.cpu(), z64) <= ABS_BAR
            n += 1
    assert n == 3
    model.recurrent.check()
