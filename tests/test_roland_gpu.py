"""ROLAND / sparse GCNConv on the device against the float64 restatement (tests/roland_restate.py): the reference's recorded recurrences
(g24 fixtures), the CSR normalisation against the dense one, the gather SpMM with each epilogue at the widths and row lengths that reach
each of its branches, ROLAND at the example's width, determinism, the module's state handling, the one-call forward against the same
launches composed from Python, and GCNConv on either side of the dense cap."""
import pytest
import torch

import roland_restate as rr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# The parity bar of tests/test_gclstm_gpu.py / test_ctan_gpu.py.  Ratio: the device's distance from the float64 restatement against the
# float32 restatement's own, 2.0 wherever the latter is measurable (>= 1e-7).  Absolute: close()'s 1e-5 of max(1, |ref|).
RATIO_BAR, NOISE_FLOOR, ABS_BAR = 2.0, 1e-7, 1e-5
LONG_ROW, VERY_LONG = 64, 2048  # kSpmmLongRow, kSpmmVeryLong (csrc/spmm.h)
UPDATES = ['moving', 'learnable', 'gru', 'mlp', None]


def dev(v):
    return None if v is None else v.to(DEV)


def bar(got, ref, f32, label):
    got = got.detach().cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32 and torch.isfinite(got).all(), label
    d_hip, d_f32 = rr.rel_err(got, ref), rr.rel_err(f32, ref)
    print(f'roland parity {label}: hip {d_hip:.3e} float32 {d_f32:.3e} ratio {d_hip / max(d_f32, 1e-30):.2f}')
    assert d_hip <= ABS_BAR, (label, d_hip)
    if d_f32 >= NOISE_FLOOR:
        assert d_hip <= RATIO_BAR * d_f32, (label, d_hip, d_f32)


def make_model(meta, params):
    from tgm_amd.nn import ROLAND

    model = ROLAND(meta['input_channel'], meta['out_channel'], meta['num_nodes'], update=meta['update'], tau=meta['tau'] if meta['update'] is None else 0.5)
    model.load_state_dict(params, strict=True)
    return model.to(DEV).eval()


def device_replay(meta, params, snaps, idx=torch.int64):
    model = make_model(meta, params)
    step = lambda s, x, ei, prev, cur, prv: model(dev(x), dev(ei.to(idx)), prev, cur, prv)
    with torch.no_grad():
        runs = [[h.cpu() for h in out] for _, out in rr.replay(meta, snaps, step)]
    model.check()
    return runs


# ---- the reference's recorded recurrences ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', rr.EXPECTED_FIXTURES)
def test_fixture_recurrence(name):
    meta, params, snaps = rr.load_fixture(name)
    r64, r32 = device_replay(meta, params, snaps, torch.int64), device_replay(meta, params, snaps, torch.int32)
    ref, f32 = rr.restated_replay(meta, params, snaps), rr.restated_replay(meta, params, snaps, torch.float32)
    for s, snap in enumerate(snaps):
        for l in range(2):
            assert torch.equal(r64[s][l], r32[s][l]), (name, s, l)  # int32 ids are read as they are
            assert not r64[s][l].requires_grad
            rr.close(r64[s][l], snap[f'H{l}'], f'{name} H{l} {s} against the record')
            bar(r64[s][l], ref[s][1][l], f32[s][1][l], f'{name} H{l} {s}')


# ---- tgmx_gcn_norm_csr alone -------------------------------------------------------------------------------------------------------------------
def Holder():
    """Something with the skipped-edge counter and check() of the modules."""
    from tgm_amd.nn.gclstm import _Skipped

    return type('Holder', (_Skipped,), {})()


def densify(csr, N):
    indptr, cols, vals, diag = (t.cpu() for t in csr)
    A = torch.diag(diag.double())
    assert indptr[0] == 0 and (indptr[1:] >= indptr[:-1]).all()
    for i in range(N):
        for j in range(int(indptr[i]), int(indptr[i + 1])):
            A[i, cols[j]] += vals[j].double()
    return A


def loops_and_repeats_graph(N, E, seed):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N, (2, E), generator=g)
    loops = torch.tensor([[3, 3, 3, 5], [3, 3, 3, 5]])  # three loops on node 3: the last one's weight is the loop weight
    ei = torch.cat([ei, loops, ei[:, :10]], dim=1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    return ei, torch.rand(ei.shape[1], generator=g) + 0.5


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('fill,add_self_loops', [(1.0, True), (2.0, True), (1.0, False)])
def test_norm_csr_against_the_dense_normalisation(weighted, fill, add_self_loops):
    from tgm_amd.nn.tgcn import gcn_norm_csr, normalized_adjacency

    N = 41
    ei, w = loops_and_repeats_graph(N, 160, 5)
    w = w if weighted else None
    for idx in (torch.int64, torch.int32):
        csr = gcn_norm_csr(dev(ei.to(idx)), dev(w), N, fill, add_self_loops)
        A = densify(csr, N)
        dense = normalized_adjacency(dev(ei), dev(w), N, fill, add_self_loops).cpu().double()
        assert (A - dense).abs().max() <= 1e-6
        ref = rr.dense_adjacency(rr.gcn_norm(ei, w, N, fill, add_self_loops), N)
        assert (A - ref).abs().max() <= 1e-6
        if not add_self_loops:
            assert not csr[3].any()


def test_norm_csr_two_runs_give_the_same_bits_and_the_last_loop_wins():
    from tgm_amd.nn.tgcn import gcn_norm_csr

    N = 60
    ei, w = loops_and_repeats_graph(N, 900, 8)
    a, b = gcn_norm_csr(dev(ei), dev(w), N, 1.0, True), gcn_norm_csr(dev(ei), dev(w), N, 1.0, True)
    nnz = int(a[0][-1])
    assert nnz == int((ei[0] != ei[1]).sum())
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3]) and torch.equal(a[1][:nnz], b[1][:nnz]) and torch.equal(a[2][:nnz], b[2][:nnz])
    last = max(e for e in range(ei.shape[1]) if ei[0, e] == 3 and ei[1, e] == 3)
    deg = w[(ei[1] == 3) & (ei[0] != 3)].double().sum() + w[last].double()
    assert a[3][3].item() == pytest.approx((w[last].double() / deg).item(), rel=1e-6)


def test_norm_csr_skips_out_of_range_endpoints_and_check_raises_once():
    from tgm_amd.nn.tgcn import gcn_norm_csr

    N = 30
    ei, w = loops_and_repeats_graph(N, 100, 6)
    bad = torch.tensor([[2, -1, N, 4], [N, 3, 5, -7]])
    ei_bad, w_bad = torch.cat([ei[:, :50], bad, ei[:, 50:]], dim=1), torch.cat([w[:50], torch.ones(4), w[50:]])
    holder = Holder()
    good = densify(gcn_norm_csr(dev(ei), dev(w), N, 1.0, True, holder._skipped(torch.device(DEV))), N)
    holder.check()  # nothing skipped
    got = densify(gcn_norm_csr(dev(ei_bad), dev(w_bad), N, 1.0, True, holder._skipped(torch.device(DEV))), N)
    assert torch.equal(got, good)
    with pytest.raises(ValueError, match='skipped'):
        holder.check()
    holder.check()  # reported once


def test_norm_csr_without_edges():
    from tgm_amd.nn.tgcn import gcn_norm_csr

    empty = torch.zeros((2, 0), dtype=torch.int64, device=DEV)
    for fill, loops, want in ((1.0, True, 1.0), (2.0, True, 1.0), (1.0, False, 0.0)):
        indptr, cols, vals, diag = gcn_norm_csr(empty, None, 9, fill, loops)
        assert not indptr.any() and indptr.numel() == 10 and torch.allclose(diag.cpu(), torch.full((9,), want), atol=1e-6)  # fill / fill = 1


# ---- tgmx_gcn_propagate alone ------------------------------------------------------------------------------------------------------------------
def rand_graph(seed, N, E):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, N, (2, E), generator=g)  # directed, with repeats and self loops


def hub_graph(N, hub_in):
    """node 0: hub_in distinct sources; node 1: one incoming edge; node 2: none (it only sends); the rest a sparse random graph"""
    assert N >= hub_in + 3
    g = torch.Generator().manual_seed(hub_in)
    ei = torch.stack([torch.cat([torch.arange(3, 3 + hub_in), torch.tensor([2, 2])]), torch.cat([torch.zeros(hub_in, dtype=torch.int64), torch.tensor([1, 5])])])
    ei = torch.cat([ei, torch.randint(3, N, (2, 2 * N), generator=g)], dim=1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    indeg = torch.bincount(ei[1][ei[0] != ei[1]], minlength=N)
    assert indeg[0] == hub_in and indeg[1] == 1 and indeg[2] == 0
    return ei


def propagate_case(ei, N, C, mode, label, tau=0.3, tau_tensor=False, off_grid=False, scratch=False, bias=True, seed=0):
    """tgmx_gcn_propagate over tgmx_gcn_norm_csr's CSR against the restatement's propagate + epilogue."""
    from tgm_amd import _native
    from tgm_amd.nn.tgcn import gcn_norm_csr, gcn_propagate

    g = torch.Generator().manual_seed(seed + C)
    t, prev = torch.randn(N, C, generator=g), torch.randn(N, C, generator=g)
    b = torch.empty(C).uniform_(-0.5, 0.5, generator=g) if bias else None
    outs = {}
    for dtype in (torch.float64, torch.float32):
        s = rr.propagate(rr.gcn_norm(ei, None, N, 1.0, True, dtype), t.to(dtype))
        outs[dtype] = rr.epilogue(s if b is None else s + b.to(dtype), mode, prev.to(dtype), tau)
    csr = gcn_norm_csr(dev(ei), None, N, 1.0, True)
    if off_grid:  # the operand a column slice that starts one float off the 16-byte grid; the output's leading dimension wider than C
        wide = torch.zeros(N, C + 5, device=DEV)
        wide[:, 1 : C + 1] = dev(t)
        wide_out = torch.full((N, C + 3), -7.0, device=DEV)
        t_d, out = wide[:, 1 : C + 1], wide_out[:, :C]
        assert t_d.data_ptr() % 16 == 4 and out.stride(0) != C
    else:
        t_d, out = dev(t), torch.empty(N, C, device=DEV)
    ws = None
    if scratch:
        n = _native.load().tgmx_cheb_propagate_scratch_floats(ei.shape[1], C)
        assert n > 0
        ws = torch.empty(n, device=DEV)
    copy = torch.empty(N, C, device=DEV) if mode == 'tau' else None
    got = gcn_propagate(csr, t_d, out, bias=dev(b), epilogue=mode, prev=dev(prev) if mode == 'tau' else None,
                        tau=torch.tensor([tau], device=DEV) if tau_tensor else tau, prev_copy=copy, scratch=ws, E=ei.shape[1])  # fmt: skip
    bar(got, outs[torch.float64], outs[torch.float32], label)
    if copy is not None:
        assert torch.equal(copy.cpu(), prev)  # the caller's state copied on the way
    if off_grid:
        assert (wide_out[:, C:] == -7.0).all()  # nothing written past the row's C floats
    return got


@pytest.mark.parametrize('C', [1, 5, 64, 256, 260])
@pytest.mark.parametrize('mode', ['none', 'relu', 'tau'])
def test_propagate_widths_and_epilogues(C, mode):
    """Scalar lanes with a tail (1, 5), one float4 a lane short of a pass (64), exactly one pass (256), a second pass (260)."""
    ei = rand_graph(C, 150, 700)
    a = propagate_case(ei, 150, C, mode, f'C={C} {mode}')
    if mode == 'tau':
        b = propagate_case(ei, 150, C, mode, f'C={C} tau on the device', tau_tensor=True)
        assert torch.equal(a, b)  # tau as a float and as a device tensor: the same bits


@pytest.mark.parametrize('C', [5, 8, 260])
@pytest.mark.parametrize('mode', ['none', 'relu', 'tau'])
def test_propagate_off_the_16_byte_grid(C, mode):
    ei = rand_graph(3 + C, 90, 400)
    a = propagate_case(ei, 90, C, mode, f'off grid C={C} {mode}', off_grid=True, bias=mode != 'none')
    b = propagate_case(ei, 90, C, mode, f'on grid C={C} {mode}', bias=mode != 'none')
    assert torch.equal(a, b)  # scalar and float4 lanes sum in the same order


@pytest.mark.parametrize('mode', ['none', 'relu', 'tau'])
def test_propagate_row_lengths(mode):
    """In-degree 0, 1, the long-row threshold 64, 65 and 70 (split over four waves: the epilogue runs in wave 0)."""
    for hub_in in (LONG_ROW, LONG_ROW + 1, LONG_ROW + 6):
        for C in (8, 260):
            propagate_case(hub_graph(100, hub_in), 100, C, mode, f'hub of {hub_in} C={C} {mode}', tau_tensor=C == 8)


@pytest.mark.parametrize('mode', ['none', 'relu', 'tau'])
def test_propagate_very_long_row(mode):
    """In-degree 2 049 = one past the very-long threshold: with scratch the row goes through the chunk launch and the epilogue runs in the
    join kernel; without scratch it stays with its workgroup."""
    assert VERY_LONG + 1 == 2049
    ei = hub_graph(2100, VERY_LONG + 1)
    propagate_case(ei, 2100, 8, mode, f'very long {mode} with scratch', scratch=True)
    propagate_case(ei, 2100, 8, mode, f'very long {mode} without scratch')
    propagate_case(ei, 2100, 5, mode, f'very long {mode} scalar lanes', scratch=True, tau_tensor=True)


# ---- ROLAND at the example's width ---------------------------------------------------------------------------------------------------------------
def wide_model(C, update, seed):
    """The constructor's own (Glorot-scaled) initialisation: with uniform(-0.6, 0.6) at this width the float32 restatement itself drifts past
    1e-5 over four snapshots.  The zero biases and the zero tau are replaced by small draws."""
    from tgm_amd.nn import ROLAND

    torch.manual_seed(seed)
    model = ROLAND(C, C, 150, update=update, tau=0.6)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for conv in (model.conv1, model.conv2):
            conv.bias.uniform_(-0.1, 0.1, generator=g)
        if update == 'learnable':
            model.tau.fill_(0.3)
    return model


@pytest.mark.parametrize('C', [256, 260])
@pytest.mark.parametrize('update', UPDATES)
def test_roland_at_width(C, update):
    N = 150
    model = wide_model(C, update, C)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(C + 1)
    snaps = [dict(x=torch.randn(N, C, generator=g), edge_index=rand_graph(10 * C + s, N, 500 + 50 * s), counts=(None, None) if s == 0 else (500 + 50 * s, 450 + 50 * s))
             for s in range(4)]  # fmt: skip
    meta = dict(input_channel=C, out_channel=C, num_nodes=N, update=update, tau=0.6, snapshots=4)
    got = device_replay(meta, params, snaps)
    ref, f32 = rr.restated_replay(meta, params, snaps), rr.restated_replay(meta, params, snaps, torch.float32)
    for s in range(4):
        for l in range(2):
            bar(got[s][l], ref[s][1][l], f32[s][1][l], f'C={C} {update} H{l} {s}')


# ---- semantics -------------------------------------------------------------------------------------------------------------------------------------
def small_setup(update, seed=4, N=300, E=4000, cin=20, C=64, dropout=0.0):
    from tgm_amd.nn import ROLAND

    torch.manual_seed(seed)
    model = ROLAND(cin, C, N, dropout=dropout, update=update, tau=0.4).to(DEV)
    if update == 'learnable':
        with torch.no_grad():
            model.tau.fill_(0.35)
    g = torch.Generator().manual_seed(seed)
    x, ei = torch.randn(N, cin, generator=g), torch.randint(0, N, (2, E), generator=g)
    prev = [torch.randn(N, C, generator=g), torch.randn(N, C, generator=g)]
    return model, dev(x), dev(ei), [dev(p) for p in prev]


@pytest.mark.parametrize('update', UPDATES)
def test_two_calls_give_the_same_bits(update):
    model, x, ei, prev = small_setup(update)
    model.eval()
    with torch.no_grad():
        a = model(x, ei, prev, 10, 30)
        b = model(x, ei, prev, 10, 30)
        c = model(x, ei)  # the stored copy of prev
    assert all(torch.equal(a[l], b[l]) and torch.equal(a[l], c[l]) for l in range(2))


@pytest.mark.parametrize('update', UPDATES)
def test_train_mode_with_grad_equals_no_grad(update):
    model, x, ei, prev = small_setup(update)
    model.train()
    assert torch.is_grad_enabled() and any(p.requires_grad for p in model.parameters())
    a = model(x.requires_grad_(), ei, prev)
    with torch.no_grad():
        b = model(x, ei, prev)
    model.eval()
    with torch.no_grad():
        c = model(x, ei, prev)
    for l in range(2):
        assert not a[l].requires_grad and a[l].grad_fn is None
        assert torch.equal(a[l], b[l]) and torch.equal(a[l], c[l])


@pytest.mark.parametrize('update', ['learnable', 'gru'])
def test_dropout_in_training_takes_the_composed_path(update):
    model, x, ei, prev = small_setup(update, dropout=0.5)
    model.train()
    torch.manual_seed(11)
    a = model(x, ei, prev)
    torch.manual_seed(11)
    b = model(x, ei, prev)
    c = model(x, ei, prev)
    for l in range(2):
        assert tuple(a[l].shape) == (300, 64) and torch.isfinite(a[l]).all() and not a[l].requires_grad
        assert torch.equal(a[l], b[l])
    assert not torch.equal(a[1], c[1])  # another mask
    model.eval()
    with torch.no_grad():
        d = model(x, ei, prev)
    ref = rr.roland_forward({k: v.cpu() for k, v in model.state_dict().items()}, update, x.cpu(), ei.cpu(), [p.cpu() for p in prev])
    assert rr.rel_err(d[1].cpu(), ref[1]) <= ABS_BAR  # eval: the native path, no dropout


@pytest.mark.parametrize('update', UPDATES)
def test_passed_embeddings_are_copied_into_the_module(update):
    model, x, ei, prev = small_setup(update)
    model.eval()
    with torch.no_grad():
        zeros = model(x, ei)  # no embeddings ever passed: zeros of [num_nodes, out_channel]
        ref0 = rr.roland_forward({k: v.cpu() for k, v in model.state_dict().items()}, update, x.cpu(), ei.cpu(), [torch.zeros(300, 64)] * 2, 0.0 if update == 'moving' else 0.4)
        assert rr.rel_err(zeros[1].cpu(), ref0[1]) <= ABS_BAR
        mine = [p.clone() for p in prev]
        a = model(x, ei, mine, 10, 30)
        mine[0].zero_(), mine[1].fill_(3.0)  # the caller overwrites its tensors
        b = model(x, ei)
        assert all(torch.equal(a[l], b[l]) for l in range(2)) and not torch.equal(a[1], zeros[1])
        assert all(torch.equal(model.previous_embeddings[l], prev[l]) for l in range(2))  # the copy; not the forward's own outputs
        with pytest.raises(ValueError):
            model(x[:-1], ei.clamp(max=298))
    model.check()


def test_moving_tau_follows_the_edge_counts():
    model, x, ei, prev = small_setup('moving')
    model.eval()
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        for counts, tau in (((None, None), 0.0), ((10, 30), 0.75), ((None, 5), 0.75), ((7, 3), float(torch.tensor(3 / 10, dtype=torch.float32)))):
            got = model(x, ei, prev, *counts)
            assert model.tau.item() == pytest.approx(tau)
            ref = rr.roland_forward(sd, 'moving', x.cpu(), ei.cpu(), [p.cpu() for p in prev], tau)
            assert rr.rel_err(got[1].cpu(), ref[1]) <= ABS_BAR


@pytest.mark.parametrize('update', ['learnable', None, 'mlp'])
def test_one_call_forward_equals_the_launches_composed_in_python(update):
    """tgmx_roland_forward against gcn_norm_csr, sgemm_nt and gcn_propagate called one by one: equal bits."""
    from tgm_amd.nn import _ops
    from tgm_amd.nn.tgcn import gcn_norm_csr, gcn_propagate

    model, x, ei, prev = small_setup(update, N=300, E=5000)
    model.eval()
    N, C = 300, 64
    with torch.no_grad():
        got = model(x, ei, prev)
        csr = gcn_norm_csr(ei, None, N, 1.0, True)
        h, out = x, []
        for l, conv in enumerate((model.conv1, model.conv2)):
            xw = _ops.sgemm_nt(h, conv.lin.weight.detach(), torch.empty(N, C, device=DEV))
            if update == 'mlp':
                op = torch.empty(N, 2 * C, device=DEV)
                op[:, C:] = prev[l]
                gcn_propagate(csr, xw, op[:, :C], bias=conv.bias.detach(), epilogue='relu', E=ei.shape[1])
                lin = getattr(model, f'mlp{l + 1}')
                h = _ops.sgemm_nt(op, lin.weight.detach(), torch.empty(N, C, device=DEV), bias=lin.bias.detach())
            else:
                tau = model.tau.detach() if update == 'learnable' else float(model.tau)
                h = gcn_propagate(csr, xw, torch.empty(N, C, device=DEV), bias=conv.bias.detach(), epilogue='tau', prev=prev[l], tau=tau, E=ei.shape[1])
            out.append(h)
    assert torch.equal(got[0], out[0]) and torch.equal(got[1], out[1])


def test_out_of_range_edges_are_skipped_and_reported():
    model, x, ei, prev = small_setup('learnable')
    model.eval()
    bad = torch.cat([ei[:, :100], torch.tensor([[0, 300], [-1, 4]], device=DEV), ei[:, 100:]], dim=1)
    with torch.no_grad():
        a, b = model(x, ei, prev), model(x, bad, prev)
    assert torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match='skipped'):
        model.check()
    model.check()


# ---- GCNConv on either side of the dense cap ---------------------------------------------------------------------------------------------------
def test_gcnconv_above_the_dense_cap():
    from tgm_amd.nn import GCNConv

    N, C = 16385, 5
    g = torch.Generator().manual_seed(2)
    ei = torch.cat([torch.randint(0, N, (2, 3000), generator=g), torch.tensor([[N - 1, 7, 7], [0, 7, N - 1]])], dim=1)
    w = torch.rand(ei.shape[1], generator=g) + 0.5
    x = torch.randn(N, 6, generator=g)
    torch.manual_seed(2)
    conv = GCNConv(6, C, improved=True)
    with torch.no_grad():
        conv.bias.uniform_(-0.5, 0.5, generator=g)
    W, b = conv.lin.weight.detach().clone(), conv.bias.detach().clone()
    conv = conv.to(DEV)
    with torch.no_grad():
        got = conv(dev(x), dev(ei), dev(w))
    conv.check()
    bar(got, rr.gcn_conv(W, b, x, ei, w, 2.0), rr.gcn_conv(W, b, x, ei, w, 2.0, dtype=torch.float32), 'GCNConv N=16385')
    with pytest.raises(NotImplementedError):  # with gradients the dense path is the only one
        conv(dev(x), dev(ei), dev(w))


def test_gcnconv_at_the_dense_cap_is_the_dense_path():
    """N = 16 384 stays on the dense adjacency: the same bits as the two GEMMs over normalized_adjacency."""
    from tgm_amd.nn import GCNConv, _ops
    from tgm_amd.nn.tgcn import normalized_adjacency

    N, C = 16384, 5
    g = torch.Generator().manual_seed(3)
    ei, x = dev(torch.randint(0, N, (2, 3000), generator=g)), dev(torch.randn(N, 6, generator=g))
    torch.manual_seed(3)
    conv = GCNConv(6, C).to(DEV)
    with torch.no_grad():
        got = conv(x, ei)
        A = normalized_adjacency(ei, None, N, 1.0, True)
        xwt = _ops.sgemm_nt(conv.lin.weight.detach(), x, torch.empty(C, N, device=DEV))
        want = _ops.sgemm_nt(A, xwt, torch.empty(N, C, device=DEV), bias=conv.bias.detach(), K=N)
    assert torch.equal(got, want)
