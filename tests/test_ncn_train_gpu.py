"""NCNPredictor training on the device: ``tgmx_ncn_dx`` alone against the float64 restatement's bound at the kernel's edges (tests/ncn_train_cases.py),
then the whole training path -- ``NcnFunction``: forward = the no-grad call's bits, backward = ONE ``tgmx_ncn_backward`` -- against the
restatement's bound, against float64 autograd under the project's bar (1e-4 of each gradient's max) and next to the float32 gradients
recorded from the reference.  The measured figures are in DESIGN.md 3.7.
"""
import ctypes

import pytest
import torch

import ncn_bwd_restate as br
import ncn_restate as nr
import ncn_train_cases as tc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-4  # of each gradient's max
NAMES = ('x', *br.PARAMS)


def build(c, **kw):
    from tgm_amd.nn import NCNPredictor

    m = NCNPredictor(c.C, c.H, c.out, k=c.k, cn_time_decay=c.decay, duplicate_targets=c.dup, **kw)
    m.load_state_dict(c.sd, strict=True)
    return m.to(DEV).train()


def run(c, m, x_grad=True, prepared=False, tar64=True):
    """(out, name -> gradient) of one call and its backward with the case's upstream gradient"""
    from tgm_amd.nn.ncn import adjacency

    x, ei, tar, lu, et = tc.tensors(c, DEV, tar64)
    x = x.requires_grad_(x_grad)
    m.zero_grad(set_to_none=True)
    out = m(x, adjacency(c.N, ei) if prepared else ei, tar, lu, et)
    if out.requires_grad and out.numel():
        out.backward(c.dout.to(DEV).reshape(out.shape))
    g = {n: p.grad for n, p in m.named_parameters()}
    g['x'] = x.grad
    return out, g


def check(tag, c, got, want=None):
    """every gradient three ways: the restatement's bound, the project's bar against float64 autograd, and the printed parity ratio"""
    want = br.grads(c.sd, c.x, c.ei, c.tar, c.k, c.dout, c.lu, c.et, c.dup) if want is None else want
    auto = br.autograd_grads(c.sd, c.x, c.ei, c.tar, c.k, c.dout, c.lu, c.et, c.dup)
    f32 = getattr(c, 'ref', None)  # the reference's recorded float32 gradients, or float32 autograd of the restatement
    src = 'recorded' if f32 is not None else 'float32 autograd'
    if f32 is None:
        f32 = br.autograd_grads(c.sd, c.x, c.ei, c.tar, c.k, c.dout, c.lu, c.et, c.dup, dtype=torch.float32)
    worst = 0.0
    for n in NAMES:
        assert got[n] is not None, (tag, n)
        val, bound = want[n]
        ratio = br.worst_ratio(got[n], val, bound)
        d_hip, d_f32 = nr.rel_err(got[n], val), nr.rel_err(f32[n], val)
        print(f'ncn grad {tag} {n}: err/bound {ratio:.3f}; hip {d_hip:.3e} {src} {d_f32:.3e} ratio {d_hip / max(d_f32, 1e-30):.2f}')
        worst = max(worst, ratio)
        assert float((got[n].detach().cpu().double() - auto[n]).abs().max()) <= BAR * float(auto[n].abs().max()), (tag, n)
    assert got['xslin.weight'] is None and got['xslin.bias'] is None
    assert worst <= 1.0, (tag, worst)


# ---- tgmx_ncn_dx alone ----------------------------------------------------------------------------------------------------------------------
def dx_on_device(c):
    from tgm_amd import _native
    from tgm_amd.nn.ncn import adjacency

    lib, st = _native.load(), _native.stream_ptr()
    x, ei, tar, lu, et = tc.tensors(c, DEV, c.tar64)
    N, B, C, k, E = c.N, c.B, c.C, c.k, c.ei.shape[1]
    adj = adjacency(N, ei)
    tar = tar.contiguous()
    is64 = int(tar.dtype == torch.int64)
    last = torch.empty(2 * N, dtype=torch.int32, device=DEV)
    lastp = 0 if c.dup == 'all' else last.data_ptr()
    xs = torch.empty((max(B, 1), k * C), device=DEV)
    _native.check(lib.tgmx_ncn_cn_emb(x.data_ptr(), N, C, k, adj.indptr.data_ptr(), adj.cols.data_ptr(), tar.data_ptr(), is64, max(B, 1), B,
                                      _native.ptr(lu), _native.ptr(et), lastp, xs.data_ptr(), k * C, st), 'tgmx_ncn_cn_emb')  # fmt: skip
    dxs = c.dxs.to(DEV)
    need = int(lib.tgmx_ncn_dx_workspace_bytes(N, E, B, C))
    assert need > 0
    outs = []
    for _ in range(2):
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        dx = torch.full((N, C), float('nan'), device=DEV)
        _native.check(lib.tgmx_ncn_dx(x.data_ptr(), N, C, k, adj.indptr.data_ptr(), adj.cols.data_ptr(), E, tar.data_ptr(), is64, max(B, 1), B,
                                      _native.ptr(lu), _native.ptr(et), lastp, dxs.data_ptr(), k * C, dx.data_ptr(), ws.data_ptr(), need, st),
                      'tgmx_ncn_dx')  # fmt: skip
        outs.append(dx)
    return outs


@pytest.mark.parametrize('name', sorted(tc.DX_CASES))
def test_dx_alone_within_the_restatement_s_bound(name):
    c = tc.DX_CASES[name]()
    a, b = dx_on_device(c)
    assert torch.equal(a, b) and not torch.isnan(a).any()  # every row written; two runs, the same bits
    val, bound = br.grads(None, c.x, c.ei, c.tar, c.k, None, c.lu, c.et, c.dup, dxs=c.dxs)['x']
    ratio = br.worst_ratio(a, val, bound)
    print(f'ncn dx {name}: err/bound {ratio:.3f}, hip vs float64 {nr.rel_err(a, val):.3e}')
    assert ratio <= 1.0
    if c.B and 'no_edge' not in name and 'one_node' not in name:
        assert bool(val.any())  # the case is not vacuous


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(tc.GPU_CASES))
def test_gradients_end_to_end(name):
    c = tc.GPU_CASES[name]()
    m = build(c)
    out, got = run(c, m)
    assert 'NcnFunction' in type(out.grad_fn).__name__
    if not name.startswith('rand_outside'):
        assert nr.rel_err(out, nr.forward(c.sd, c.x, c.ei, c.tar, c.k, c.lu, c.et, c.dup)) < 1e-4
    check(name, c, got)


def test_the_output_is_the_no_grad_call_s_and_the_function_is_native():
    c = tc.GPU_CASES['g31_k4_decay']()
    m = build(c)
    x, ei, tar, lu, et = tc.tensors(c, DEV)
    out = m(x.requires_grad_(), ei, tar, lu, et)
    with torch.no_grad():
        plain = m(x, ei, tar, lu, et)
    assert torch.equal(out, plain) and out.requires_grad
    assert 'NcnFunction' in type(out.grad_fn).__name__


def test_two_calls_then_one_backward():
    """the positives' and the negatives' call keep their own activations: one backward gives the sum of the two restated gradients"""
    cp, cn = tc.GPU_CASES['pos'](), tc.GPU_CASES['neg']()
    m = build(cp)
    x, ei, tp, lu, et = tc.tensors(cp, DEV)
    tn = cn.tar.to(DEV)
    x.requires_grad_()
    pos, neg = m(x, ei, tp, lu, et), m(x, ei, tn, lu, et)
    ((pos * cp.dout.to(DEV)).sum() + (neg * cn.dout.to(DEV)).sum()).backward()
    got = {n: p.grad for n, p in m.named_parameters()}
    got['x'] = x.grad
    a, b = (br.grads(c.sd, c.x, c.ei, c.tar, c.k, c.dout, c.lu, c.et, c.dup) for c in (cp, cn))
    for n in NAMES:
        # (autograd adds the two calls' gradients: one more rounding of their sum)
        val, bound = a[n][0] + b[n][0], a[n][1] + b[n][1] + br.U * (a[n][0] + b[n][0]).abs()
        assert br.worst_ratio(got[n], val, bound) <= 1.0, n
    assert not torch.equal(tp, tn)


def test_prepared_adjacency_and_a_second_run_give_the_same_bits():
    c = tc.GPU_CASES['hub_k4']()
    m = build(c)
    _, a = run(c, m)
    _, b = run(c, m)
    _, p = run(c, m, prepared=True)
    _, i32 = run(c, m, tar64=False)
    for n in NAMES:
        assert torch.equal(a[n], b[n]) and torch.equal(a[n], p[n]) and torch.equal(a[n], i32[n]), n


@pytest.mark.parametrize('subset', ['x_only', 'weights_only', 'first_frozen', 'last_frozen'])
def test_requires_grad_subsets(subset):
    c = tc.GPU_CASES['rand_k4_decay']()
    _, full = run(c, build(c))
    m = build(c)
    frozen = {'x_only': list(br.PARAMS), 'weights_only': [], 'first_frozen': ['xsmlp.0.weight', 'xsmlp.0.bias'],
              'last_frozen': ['xsmlp.2.weight', 'xsmlp.2.bias']}[subset]  # fmt: skip
    for n, p in m.named_parameters():
        p.requires_grad_(n not in frozen and not n.startswith('xslin'))
    out, got = run(c, m, x_grad=subset != 'weights_only')
    assert 'NcnFunction' in type(out.grad_fn).__name__
    for n in NAMES:
        if n in frozen or (n == 'x' and subset == 'weights_only'):
            assert got[n] is None, n
        else:
            assert torch.equal(got[n], full[n]), n  # skipping a gradient changes no other


@pytest.mark.parametrize('name', ['rand_k4_decay', 'rand_out17', 'hub_k4'])
def test_backward_modes(name, monkeypatch):
    c = tc.GPU_CASES[name]()
    m = build(c)
    _, native = run(c, m)
    monkeypatch.setenv('TGMX_NCN_BWD', 'py')
    out, py = run(c, m)
    assert 'NcnFunction' in type(out.grad_fn).__name__
    monkeypatch.setenv('TGMX_NCN_BWD', 'torch')
    out, composed = run(c, m)
    assert 'NcnFunction' not in type(out.grad_fn).__name__
    for n in NAMES:
        assert torch.equal(native[n], py[n]), n  # the launches one by one: the same bits
        assert float((composed[n] - native[n]).abs().max()) <= BAR * float(native[n].abs().max()), n


def test_autocast_takes_the_composed_path():
    c = tc.GPU_CASES['rand_k4_decay']()
    m = build(c)
    x, ei, tar, lu, et = tc.tensors(c, DEV)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = m(x.requires_grad_(), ei, tar, lu, et)
    assert out.requires_grad and 'NcnFunction' not in type(out.grad_fn).__name__
    g = m.get_cn_emb(x, ei, tar, (lu, et))  # under gradients: composed, as before
    assert g.requires_grad and 'NcnFunction' not in type(g.grad_fn).__name__


def test_no_pair_gives_zero_gradients():
    c = tc.make(nr.hashed_x(12, 5, 50), tc.small_graph(50)[1], torch.zeros((2, 0), dtype=torch.long), 4, 50)
    m = build(c)
    out, got = run(c, m)
    assert out.shape == (0,)
    out.sum().backward()
    assert all(got[n] is None for n in NAMES)  # (run() did not call backward on an empty result)
    assert all(p.grad is None or not bool(p.grad.any()) for n, p in m.named_parameters())


def test_workspace_bytes_at_large_sizes():
    from tgm_amd import _native
    from test_ncn_train_cpu import _block

    lib = _native.load()
    need = lambda *a: int(lib.tgmx_ncn_backward_workspace_bytes(ctypes.byref(_block(*a))))
    sizes = [need(1250, 2300, B) for B in (200, 4096, 100_000, 10**6)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert need(1250, 2300, 2**30) == 0 and need(1250, 2**30, 200) == 0


def test_one_adam_step_changes_the_weights_and_the_next_call_sees_them():
    c = tc.GPU_CASES['pos']()
    m = build(c)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    x, ei, tar, lu, et = tc.tensors(c, DEV)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    pos, neg = m(x, ei, tar, lu, et), m(x, ei, tar.flip(0), lu, et)
    assert 'NcnFunction' in type(pos.grad_fn).__name__
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    loss = bce(pos, torch.ones_like(pos)) + bce(neg, torch.zeros_like(neg))
    opt.zero_grad()
    loss.backward()
    opt.step()
    assert all(not torch.equal(before[n], p) for n, p in m.named_parameters() if n.startswith('xsmlp')) and m.xslin.weight.grad is None
    sd = {n: v.detach().cpu() for n, v in m.state_dict().items()}
    with torch.no_grad():
        assert nr.rel_err(m(x, ei, tar, lu, et), nr.forward(sd, c.x, c.ei, c.tar, c.k, c.lu, c.et)) < 1e-4
    again = m(x, ei, tar, lu, et)  # and the training path reads the updated weights too
    assert nr.rel_err(again, nr.forward(sd, c.x, c.ei, c.tar, c.k, c.lu, c.et)) < 1e-4


@pytest.mark.parametrize('k', [2, 4])
def test_one_training_step_at_the_example_s_dims(k):
    """Sampler -> TGNMemory -> GraphAttentionEmbedding -> NCNPredictor (positives, negatives) -> BCE -> backward, C = H = 100, B = 200 on a
    600-edge wiki-shaped prefix: z.grad reaches the encoder, and the decoder's gradients are held to the restatement on the device's own z."""
    from tgm_amd import DGData, DGDataLoader, DGraph
    from tgm_amd.hooks import DeduplicationHook, HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook
    from tgm_amd.nn import GraphAttentionEmbedding, IdentityMessage, LastAggregator, NCNPredictor, TGNMemory, sampled_edge_list
    from tgm_amd.synth import make_stream

    torch.manual_seed(3)
    D, M, T_ = 172, 100, 100
    s = make_stream('wiki', seed=5, num_edges=600, edge_dim=D, n_src=300, n_dst=100, t_hi=600 * 20)
    N = s.num_nodes
    dg = DGraph(DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1).int(), s.edge_x), device=DEV)
    hm = HookManager(keys=['k'])
    hm.register('k', RandomNegativeEdgeSamplerHook(low=300, high=N, seed=4))
    hm.register('k', RecencyNeighborHook(N, [10], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
    hm.register('k', DeduplicationHook(seed_nodes_keys=['neg', 'nbr_nids']))
    mem = TGNMemory(N, D, M, T_, IdentityMessage(D, M, T_), LastAggregator()).to(DEV).train()
    enc = GraphAttentionEmbedding(M, 100, D, mem.time_enc).to(DEV).train()
    decoder = NCNPredictor(100, 100, 1, k=k, cn_time_decay=True).to(DEV).train()
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    with hm.activate('k'):
        for b, batch in enumerate(DGDataLoader(dg, batch_size=200, hook_manager=hm)):
            if b < 2:  # two batches of history, then the step under test
                with torch.no_grad():
                    mem(batch.unique_nids)
                    mem.update_state(batch.edge_src, batch.edge_dst, batch.edge_time, batch.edge_x)
                continue
            ei, et, ex = sampled_edge_list(batch)
            z, lu = mem(batch.unique_nids)
            z = enc(z, lu, ei, et, ex)
            z.retain_grad()
            loc = lambda ids: batch.global_to_local(ids).long()
            pos_t, neg_t = torch.stack([loc(batch.edge_src), loc(batch.edge_dst)]), torch.stack([loc(batch.edge_src), loc(batch.neg)])
            pos, neg = decoder(z, ei, pos_t, lu, batch.edge_time), decoder(z, ei, neg_t, lu, batch.edge_time)
            assert 'NcnFunction' in type(pos.grad_fn).__name__ and pos.shape == (200,)
            loss = bce(pos, torch.ones_like(pos)) + bce(neg, torch.zeros_like(neg))
            loss.backward()
            break
    assert z.grad is not None and bool(z.grad.any()) and any(p.grad is not None and bool(p.grad.any()) for p in enc.parameters())
    # the upstream gradients of the two calls, by hand: d BCE / d logit = (sigmoid(logit) - label) / B.  Torch forms them in float32 on the
    # device and this test in float32 on the host: a sigmoid within 2 ulp of a value below 1, one subtraction, one scaling -- each within
    # 4 u / B of the exact value, so within 8 u / B of each other
    sd = {n: v.detach().cpu() for n, v in decoder.state_dict().items()}
    zc, eic, luc, etc = z.detach().cpu(), ei.cpu(), lu.cpu(), batch.edge_time.cpu()
    parts = []
    for logits, label, tar in ((pos, 1.0, pos_t), (neg, 0.0, neg_t)):
        dout = ((torch.sigmoid(logits.detach()) - label) / logits.numel()).cpu()
        g = br.grads(sd, zc, eic, tar.cpu(), k, dout, luc, etc, dout_abs_err=8 * br.U / logits.numel())
        assert br.ambiguous_relu_fraction(g) <= 0.01
        parts.append(g)
    got = {n: p.grad for n, p in decoder.named_parameters()}
    got['x'] = z.grad
    for n in NAMES:
        val = parts[0][n][0] + parts[1][n][0]
        bound = parts[0][n][1] + parts[1][n][1] + br.U * val.abs()  # (autograd adds the two calls' gradients: one more rounding)
        ratio = br.worst_ratio(got[n], val, bound)
        print(f'ncn step k={k} {n}: err/bound {ratio:.3f}, hip vs float64 {nr.rel_err(got[n], val):.3e}')
        assert ratio <= 1.0, n
        assert float((got[n].detach().cpu().double() - val).abs().max()) <= BAR * float(val.abs().max()), n
