"""CTAN on the device: CTANMemory against the reference's recorded states (g22 fixtures, bit for bit), the native encoder forward against
the float64 restatement (tests/ctan_restate.py) at the shapes that reach every branch of the wide-head attention walk, the training path's
gradients, and the example's loop end to end."""
import math

import numpy as np
import pytest
import torch

import ctan_restate as cr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# The parity bar.  Ratio: the device's distance from the float64 restatement against the float32 restatement's own, the project's standing
# 2.0 wherever the latter is measurable (>= 1e-7).  Absolute: outputs are tanh values in (-1, 1) built from float32 dot products of at
# most 428 terms of order one; 1e-5 is the bar smoke() holds the TGAT forward to.
RATIO_BAR, NOISE_FLOOR, ABS_BAR = 2.0, 1e-7, 1e-5
FIXTURES = ['basic', 'dup_in_batch', 'f32_tie', 'init_time_reset', 'ooo', 'rows_mismatch', 'wiki_small']


def dev(v):
    return v.to(DEV)


# ---- memory ---------------------------------------------------------------------------------------------------------------------------
def _device_replay(name, id_dtype=torch.int64):
    from tgm_amd.nn.encoder import CTANMemory, LastAggregator

    z, meta = cr.load_fixture(name)
    made = []

    def make(N, M, init_time):
        made.append(CTANMemory(N, M, aggr_module=LastAggregator(), init_time=init_time).to(DEV))
        return made[0]

    def update(mem, s, d, t, se, de):
        mem.update_state(dev(torch.tensor(s).to(id_dtype)), dev(torch.tensor(d).to(id_dtype)), dev(torch.tensor(t)), dev(torch.tensor(se)), dev(torch.tensor(de)))

    cr.replay(z, meta, make, update, lambda m: m.reset_state(), lambda m: (m.memory.cpu().numpy(), m.last_update.cpu().numpy()))
    made[0].check()
    return made[0].memory.clone(), made[0].last_update.clone()


@pytest.mark.parametrize('name', FIXTURES)
def test_memory_replays_the_reference_fixture(name):
    a = _device_replay(name)
    b = _device_replay(name, torch.int32 if name != 'f32_tie' else torch.int64)  # a second run, ids as the loader hands them (int32)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_memory_argument_checks_and_mean_aggregator():
    from tgm_amd.nn.encoder import CTANMemory, LastAggregator, MeanAggregator

    mem = CTANMemory(6, 3, aggr_module=LastAggregator()).to(DEV)
    s, d, t = dev(torch.tensor([0, 1])), dev(torch.tensor([2, 3])), dev(torch.tensor([5, 6]))
    with pytest.raises(ValueError):
        mem.update_state(s, d, t, torch.rand(2, 3, device=DEV), torch.rand(1, 3, device=DEV))  # fewer than 2B rows in total
    mem.update_state(s, dev(torch.tensor([2, 9])), t, torch.rand(2, 3, device=DEV), torch.rand(2, 3, device=DEV))  # node 9 of 6
    with pytest.raises(ValueError, match='outside'):
        mem.check()
    mem.check()  # reported once
    assert mem.last_update.tolist() == [5, 6, 5, 0, 0, 0]
    z, lu = mem(dev(torch.tensor([1, 2])))
    assert z.shape == (2, 3) and lu.tolist() == [6, 5]
    # MeanAggregator: composed from torch ops; the mean of a node's rows, the maximal time
    mean = CTANMemory(6, 3, aggr_module=MeanAggregator(), init_time=4).to(DEV)
    se, de = torch.rand(3, 3, device=DEV), torch.rand(3, 3, device=DEV)
    mean.update_state(dev(torch.tensor([0, 1, 0])), dev(torch.tensor([1, 1, 5])), dev(torch.tensor([7, 9, 8])), se, de)
    assert mean.last_update.tolist() == [8, 9, 4, 4, 4, 8]
    torch.testing.assert_close(mean.memory[0], (se[0] + se[2]) / 2)
    torch.testing.assert_close(mean.memory[1], (se[1] + de[0] + de[1]) / 3)
    assert torch.equal(mean.memory[5], de[2]) and not mean.memory[2:5].any()


# ---- encoder parity -------------------------------------------------------------------------------------------------------------------
def make_case(seed, U, M, T, D, S, num_iters, E=None, seg_lens=None, int_msg=False, defaults=False, base=1_700_000_000):
    """A model and inputs on the CPU.  seg_lens: incoming-edge counts of targets 0, 1, ... (the rest get none); else E random edges."""
    from tgm_amd.nn.encoder import CTAN

    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    kw = {} if defaults else dict(mean_delta_t=300.5, std_delta_t=450.25, epsilon=0.5, gamma=0.3)
    enc = CTAN(edge_dim=D, memory_dim=M, time_dim=T, node_dim=S, num_iters=num_iters, **kw)
    with torch.no_grad():
        enc.aconv.bias.uniform_(-0.5, 0.5, generator=g)
    if seg_lens is not None:
        tgt = torch.repeat_interleave(torch.arange(len(seg_lens)), torch.tensor(seg_lens))
        tgt = tgt[torch.randperm(tgt.numel(), generator=g)]
        E = tgt.numel()
    else:
        tgt = torch.randint(0, U, (E,), generator=g)
    src = torch.randint(0, U, (E,), generator=g)
    node_x = torch.randn(U, M + S, generator=g)
    last_update = base + torch.randint(0, 2000, (U,), generator=g)
    t = base + torch.randint(0, 2000, (E,), generator=g)  # above AND below last_update[src]
    msg = torch.randint(0, 10, (E, D), generator=g) if int_msg else torch.randn(E, D, generator=g)
    cfg = dict(num_iters=num_iters, mean_delta_t=enc.mean_delta_t, std_delta_t=enc.std_delta_t, epsilon=enc.aconv.epsilon, gamma=enc.aconv.gamma)
    return enc, (node_x, last_update, torch.stack([src, tgt]), t, msg), cfg


def native(enc, args):
    enc = enc.to(DEV).eval()
    with torch.no_grad():
        out = enc(*[dev(a) for a in args])
    enc.check()
    return out


def parity(enc, args, cfg, label):
    sd = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
    ref = cr.ctan_forward(sd, *args, **cfg)
    f32 = cr.ctan_forward(sd, *args, dtype=torch.float32, **cfg)
    got = native(enc, args).cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32 and not torch.isnan(got).any()
    d_hip, d_f32 = cr.rel_err(got, ref), cr.rel_err(f32, ref)
    print(f'ctan parity {label}: hip {d_hip:.3e} float32 {d_f32:.3e} ratio {d_hip / max(d_f32, 1e-30):.2f}')
    assert d_hip <= ABS_BAR, (label, d_hip)
    if d_f32 >= NOISE_FLOOR:
        assert d_hip <= RATIO_BAR * d_f32, (label, d_hip, d_f32)
    return got, ref


def test_reference_unit_test_shape():
    """U 10, E 10, M 5, T 2, D 7, node_dim 1, integer msg, every default; small timestamps as the reference's test draws them."""
    enc, args, cfg = make_case(1, 10, 5, 2, 7, 1, 1, E=10, int_msg=True, defaults=True, base=0)
    args = (args[0], args[1] % 10, args[2], args[3] % 10, args[4])
    parity(enc, args, cfg, 'unit-test shape')


@pytest.mark.parametrize('M', [4, 5, 64, 100, 130, 256, 260])
@pytest.mark.parametrize('num_iters', [1, 3])
def test_widths(M, num_iters):
    """One column a lane (M <= 64), two with and without a tail, three, four (vector loads), and the hand-over to the generic walk (260)."""
    enc, args, cfg = make_case(10 + M, 40, M, 6, 9, 2, num_iters, E=300)
    parity(enc, args, cfg, f'M={M} iters={num_iters}')


@pytest.mark.parametrize('M', [5, 256])
def test_segment_lengths_and_a_hub(M):
    """Targets with 0, 1, 16, 17 (the one-wave limit), 64, 65 (a wave's block) incoming edges and one hub with 1 500."""
    enc, args, cfg = make_case(30 + M, 40, M, 8, 12, 1, 2, seg_lens=[0, 1, 16, 17, 64, 65, 1500, 3, 0, 130])
    got, ref = parity(enc, args, cfg, f'segments M={M}')
    # without the |.| the result is another one: the case has last_update on both sides of t
    sd = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
    assert (args[1][args[2][0]] > args[3]).any() and (args[1][args[2][0]] < args[3]).any()
    assert cr.rel_err(cr.ctan_forward(sd, *args, use_abs=False, **cfg), ref) > 1e-3
    # [msg | enc]: with lin_edge's column blocks read the other way round the restatement does not match
    assert cr.rel_err(got, cr.ctan_forward(sd, *args, swap_edge_blocks=True, **cfg)) > 1e-3


@pytest.mark.parametrize('U,E', [(1, 0), (1, 5), (7, 0), (33, 1)])
def test_no_edges_and_one_node(U, E):
    enc, args, cfg = make_case(50 + U, U, 12, 4, 3, 1, 2, E=E)
    parity(enc, args, cfg, f'U={U} E={E}')


def test_edge_index_dtypes_repeat_runs_and_the_native_entry(monkeypatch):
    from tgm_amd import _native

    lib = _native.load()
    calls, orig = [], lib.tgmx_ctan_forward
    monkeypatch.setattr(lib, 'tgmx_ctan_forward', lambda *a: calls.append(1) or orig(*a))
    enc, args, cfg = make_case(70, 40, 256, 16, 20, 1, 3, E=700)
    a = native(enc, args)
    b = native(enc, args)
    ei32 = dev(args[2]).to(torch.int32)
    wide = torch.zeros(2, 2 * args[2].shape[1], dtype=torch.int64, device=DEV)
    wide[:, ::2] = dev(args[2])
    with torch.no_grad():
        c = enc(dev(args[0]), dev(args[1]), ei32, dev(args[3]), dev(args[4]))
        d = enc(dev(args[0]), dev(args[1]), wide[:, ::2], dev(args[3]), dev(args[4]))
    assert not wide[:, ::2].is_contiguous()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    assert calls == [1] * 4  # the native path every time, no hand-over to torch ops
    # an edge_index entry out of range is clamped on the device and reported
    bad = dev(args[2]).clone()
    bad[0, 3] = 40
    with torch.no_grad():
        enc(dev(args[0]), dev(args[1]), bad, dev(args[3]), dev(args[4]))
    with pytest.raises(ValueError, match='outside'):
        enc.check()


def test_in_place_weight_change_is_seen():
    """An optimizer-style in-place update of aconv.W: the stacked [Wq, Wk, Wv, A] is rebuilt for the next forward."""
    enc, args, cfg = make_case(80, 20, 16, 4, 3, 1, 2, E=60)
    before = native(enc, args)
    with torch.no_grad():
        enc.aconv.W.add_(0.25 * torch.randn_like(enc.aconv.W))
        enc.aconv.phi.lin_key.bias.add_(0.5)
    got, ref = parity(enc, args, cfg, 'after an in-place update')
    assert cr.rel_err(before.cpu(), ref) > 1e-3
    opt = torch.optim.SGD(enc.parameters(), lr=0.1)
    enc.train()
    enc(*[dev(a) for a in args]).square().sum().backward()
    opt.step()
    parity(enc, args, cfg, 'after an optimizer step')


def test_attend_launch_equals_the_generic_walk():
    """tgmx_ctan_attend in mode 0 leaves what tgmx_tconv_attend leaves (H = 1), up to the order of the float32 sums."""
    from tgm_amd import _native

    lib = _native.load()
    g = torch.Generator().manual_seed(90)
    for C in (5, 100, 256):
        U, lens = 12, [0, 1, 16, 17, 64, 65, 300, 2]
        tgt = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
        E = tgt.numel()
        tgt = dev(tgt[torch.randperm(E, generator=g)])
        src = dev(torch.randint(0, U, (E,), generator=g))
        q, k, v, skip = (dev(torch.randn(U, C, generator=g)) for _ in range(4))
        e = dev(torch.randn(E, C, generator=g))
        order = torch.argsort(tgt, stable=True)
        lo = torch.searchsorted(tgt[order], torch.arange(U, device=DEV))
        hi = torch.searchsorted(tgt[order], torch.arange(U, device=DEV), right=True)
        outs = []
        for which in range(3):
            out = skip.clone()
            common = (q.data_ptr(), k.data_ptr(), v.data_ptr(), e.data_ptr(), order.data_ptr(), src.data_ptr(), lo.data_ptr(), hi.data_ptr(), U)
            if which == 0:
                _native.check(lib.tgmx_tconv_attend(*common, 1, C, C ** -0.5, out.data_ptr(), None, _native.stream_ptr()), 'tgmx_tconv_attend')
            else:
                _native.check(lib.tgmx_ctan_attend(*common, C, C ** -0.5, out.data_ptr(), None, None, 0.0, 0, _native.stream_ptr()), 'tgmx_ctan_attend')
            outs.append(out)
        assert torch.equal(outs[1], outs[2])
        assert torch.equal(outs[0][0], skip[0]) and torch.equal(outs[1][0], skip[0])  # no incoming edge
        assert cr.rel_err(outs[1].cpu(), outs[0].cpu()) < 5e-6, C


# ---- training -------------------------------------------------------------------------------------------------------------------------
def test_training_gradients_match_float64_autograd():
    """M 8, U 30, E 200, two iterations: every parameter's gradient and node_x's within 2e-4 of the gradient's largest entry (the TGN bound).
    lin_key.bias is the exception in scale only: q_i . b_k is the same for every edge of a target, so the softmax -- and the loss -- does not
    depend on it; its exact gradient is 0 (float64 autograd leaves ~1e-17 of cancellation noise) and "2e-4 of its largest entry" says nothing.
    The terms that cancel in it are those of lin_query.bias's gradient, so that gradient's largest entry is its scale."""
    enc, args, cfg = make_case(100, 30, 8, 4, 5, 2, 2, E=200)
    g = torch.Generator().manual_seed(101)
    weight = torch.randn(30, 8, generator=g)
    p64 = {k: v.detach().double().requires_grad_(k in cr.PARAMS) for k, v in enc.state_dict().items()}
    x64 = args[0].double().requires_grad_(True)
    (cr.ctan_forward(p64, x64, *args[1:], **cfg) * weight.double()).sum().backward()
    enc = enc.to(DEV).train()
    x = dev(args[0]).requires_grad_(True)
    out = enc(x, *[dev(a) for a in args[1:]])
    assert out.requires_grad
    (out * dev(weight)).sum().backward()
    named = dict(enc.named_parameters())
    assert sorted(named) == sorted(cr.PARAMS)
    for name, ref in [(k, p64[k].grad) for k in cr.PARAMS] + [('node_x', x64.grad)]:
        got = (x.grad if name == 'node_x' else named[name].grad)
        assert got is not None and ref is not None and ref.abs().max() > 0, name
        scale = ref.abs().max().item()
        if name == 'aconv.phi.lin_key.bias':
            assert scale < 1e-12, scale
            scale = p64['aconv.phi.lin_query.bias'].grad.abs().max().item()
        err = (got.cpu().double() - ref).abs().max().item() / scale
        print(f'ctan grad {name}: {err:.3e}')
        assert err <= 2e-4, (name, err)


def test_reference_unit_test_body():
    """test/unit/test_nn/test_ctan.py::test_ctan_last_aggre, on the device."""
    from tgm_amd.nn.encoder import CTAN, CTANMemory, LastAggregator

    B, S = 10, 1
    E, M, T = 7, 5, 2
    torch.manual_seed(0)
    edge_index = torch.randint(0, B, size=(2, B), device=DEV)
    edge_time = torch.randint(0, B, size=(B,), device=DEV)
    edge_feat = torch.randint(0, B, size=(B, E), device=DEV)
    memory = CTANMemory(B, M, aggr_module=LastAggregator()).to(DEV)
    encoder = CTAN(edge_dim=E, memory_dim=M, time_dim=T, node_dim=S).to(DEV)
    memory.train()
    encoder.train()
    n_id = torch.arange(B, device=DEV)  # (edge_index holds positions in [0, B): the node table is the identity, so that they are valid rows)
    z, last_update = memory(n_id)
    z = torch.cat([z, torch.rand((len(z), 1), device=DEV)], dim=-1)
    z = encoder(z, last_update, edge_index, edge_time, edge_feat)
    memory.detach()
    memory.reset_parameters()
    assert z.shape == (B, M)
    assert not torch.isnan(z).any()

    memory.eval()
    encoder.eval()
    z, last_update = memory(n_id)
    z = torch.cat([z, torch.rand((len(z), 1), device=DEV)], dim=-1)
    with torch.no_grad():
        z_native = encoder(z, last_update, edge_index, edge_time, edge_feat)
    z = encoder(z, last_update, edge_index, edge_time, edge_feat)
    assert cr.rel_err(z_native.cpu(), z.detach().cpu()) < 1e-5  # the native forward and the composed one
    memory.update_state(src=edge_index[0], pos_dst=edge_index[1], t=edge_time, src_emb=z[edge_index[0]], pos_dst_emb=z[edge_index[1]])
    memory.detach()
    memory.check()
    assert z.shape == (B, M)
    assert not torch.isnan(z).any()
    touched = torch.unique(edge_index)
    assert memory.memory[touched].abs().sum(1).min() > 0 and not memory.memory.requires_grad


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_example_loop_end_to_end():
    """examples/linkproppred/ctan.py's evaluation loop on a 2 000-event wiki-shaped stream: recency sampler [32], dedup, the sampled edge
    list, memory -> CTAN -> update_state, ten batches at M = 32, against the restatement driven with the same batches."""
    from tgm_amd import DGData, DGDataLoader, DGraph
    from tgm_amd.hooks import DeduplicationHook, HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook
    from tgm_amd.nn import sampled_edge_list
    from tgm_amd.nn.encoder import CTAN, CTANMemory, LastAggregator
    from tgm_amd.synth import make_stream

    st = make_stream('wiki', seed=21, num_edges=2000, n_src=120, n_dst=60, edge_dim=8)
    N, M, T, D = st.num_nodes, 32, 8, 8
    dg = DGraph(DGData.from_raw(st.ts, torch.stack([st.src, st.dst], 1), st.edge_x), device=DEV)
    hm = HookManager(keys=['k'])
    hm.register('k', RandomNegativeEdgeSamplerHook(120, N, seed=4))
    hm.register('k', RecencyNeighborHook(N, [32], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
    hm.register('k', DeduplicationHook(seed_nodes_keys=['neg', 'nbr_nids']))
    torch.manual_seed(22)
    t0 = int(st.ts[0])
    dts = np.diff(st.ts.numpy()).astype(np.float64)
    cfg = dict(num_iters=3, mean_delta_t=float(dts.mean() * 20), std_delta_t=float(dts.std() * 20 + 1), epsilon=0.5, gamma=0.1)
    enc = CTAN(edge_dim=D, memory_dim=M, time_dim=T, node_dim=1, **cfg).to(DEV).eval()
    mem = CTANMemory(N, M, aggr_module=LastAggregator(), init_time=t0).to(DEV).eval()
    static_x = torch.randn(N, 1)
    sd = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
    ours = cr.CTANMemoryRestated(N, M, t0)
    worst, batches = 0.0, 0
    with hm.activate('k'), torch.no_grad():
        for batch in DGDataLoader(dg, batch_size=200, hook_manager=hm):
            ei, et, ex = sampled_edge_list(batch)
            uniq = batch.unique_nids.long()
            z, lu = mem(uniq)
            z = enc(torch.cat([z, dev(static_x)[uniq]], dim=-1), lu, ei, et, ex)
            inv_src, inv_dst = batch.global_to_local(batch.edge_src).long(), batch.global_to_local(batch.edge_dst).long()
            # the restatement on the same batch, from ITS memory (equal to the device's: asserted below)
            u = uniq.cpu()
            x_ref = torch.cat([torch.from_numpy(ours.memory[u.numpy()]), static_x[u]], dim=-1)
            z_ref = cr.ctan_forward(sd, x_ref, torch.from_numpy(ours.last_update[u.numpy()]), ei.cpu(), et.cpu(), ex.cpu(), **cfg)
            worst = max(worst, cr.rel_err(z.cpu(), z_ref))
            mem.update_state(batch.edge_src, batch.edge_dst, batch.edge_time, z[inv_src], z[inv_dst])
            # the winners' embeddings are the device's own rows: the memory state must then be exact
            zc = z.cpu().numpy()
            ours.update_state(batch.edge_src.cpu().numpy(), batch.edge_dst.cpu().numpy(), batch.edge_time.cpu().numpy(), zc[inv_src.cpu().numpy()],
                              zc[inv_dst.cpu().numpy()])
            assert np.array_equal(mem.memory.cpu().numpy(), ours.memory) and np.array_equal(mem.last_update.cpu().numpy(), ours.last_update), batches
            batches += 1
    mem.check()
    enc.check()
    print(f'ctan end to end: {batches} batches, worst distance {worst:.3e}')
    assert batches == 10 and ei.shape[1] > 1000
    assert worst <= ABS_BAR
