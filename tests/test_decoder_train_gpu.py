"""Decoder training on the device against the float64 restatement of the gradients (tests/decoders_bwd_restate.py): the last layer's
backward and the table form's scatter alone through ctypes, then ``loss.backward()`` through ``LinkPredictor.forward`` /
``score_pairs`` / ``NodePredictor.forward`` in every form, the reference's recorded gradients (g30 fixtures), two calls on one module
before one backward, requires-grad subsets, an index outside the table, and the dispatch (``TGMX_DECODER_BWD``).

The kernel tests follow tests/test_tgat_bwd_blocks_gpu.py: outputs pre-filled with NaN inside allocations with sentinel columns and a
sentinel tail that must stay intact, every case launched twice and compared bit for bit.  Bars: the restatement's per-element bound
(err / bound <= 1, the worst ratio printed: ``pytest -rP``) and, for the fixtures, ``close()``'s 1e-5 of max(1, |ref|).  The end-to-end
tests also print the parity ratio -- the device's distance from float64 against float32 autograd's own on the CPU -- without asserting it.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import decoders_bwd_restate as br
import decoders_restate as dr
from test_tgat_bwd_blocks_gpu import Buf, _report, _same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
F64 = torch.float64


def _lib():
    from tgm_amd import _native

    return _native.load(), _native


# ---- tgmx_decoder_tail_bwd alone ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tail_case(R, K, O):
    """dout, x (a ReLU output: exact zeros, every fifth row all zero), W and the float64 results with their bounds -- once per shape."""
    g = torch.Generator().manual_seed(1000 * R + 10 * K + O)
    dout, W = torch.randn(R, O, generator=g), torch.empty(O, K).uniform_(-0.3, 0.3, generator=g)
    x = torch.relu(torch.randn(R, K, generator=g))
    x[2::5] = 0.0  # rows whose pre-activations were all negative
    d, w, h = dout.double(), W.double(), x.double()
    n = br.tail_bwd_chain(R)
    raw = d @ w
    want = dict(dx_relu=torch.where(h > 0, raw, torch.zeros_like(raw)), dx=raw, dW=d.t() @ h, db=d.sum(0))
    bound = dict(dx=br.gamma(O) * (d.abs() @ w.abs()), dW=br.gamma(n) * (d.abs().t() @ h.abs()), db=br.gamma(n) * d.abs().sum(0))
    bound['dx_relu'] = bound['dx']
    return dout, x, W, want, bound


def _tail_bwd(dout, x, W, relu, want_dx=True, want_sums=True):
    lib, native = _lib()
    R, K, O = x.shape[0], x.shape[1], W.shape[0]
    bd, bx, bw = Buf(R, O, ld=O + 3, lead=1, fill=7.0, data=dout), Buf(R, K, ld=K + 5, lead=2, fill=7.0, data=x), Buf(O, K, data=W)
    n = lib.tgmx_decoder_tail_bwd_workspace_floats(R, K, O)
    outs = []
    for _ in range(2):
        dx, dW, db, ws = Buf(R, K, ld=K + 3, lead=1), Buf(O, K), Buf(1, O), Buf(1, n)
        native.check(lib.tgmx_decoder_tail_bwd(bd.ptr, bd.ld, bx.ptr, bx.ld, R, K, bw.ptr, O, relu, dx.ptr if want_dx else None, dx.ld,
                                               dW.ptr if want_sums else None, db.ptr if want_sums else None, ws.ptr, n, native.stream_ptr()),
                     'tgmx_decoder_tail_bwd')  # fmt: skip
        torch.cuda.synchronize()
        for b, what in ((dx, 'dx'), (dW, 'dW'), (db, 'db'), (ws, 'workspace')):
            assert b.sentinels_intact(), f'{what}: a write outside the matrix'
        outs.append((dx.view.contiguous().clone(), dW.view.clone(), db.view.reshape(-1).clone()))
    assert all(_same_bits(a, b) for a, b in zip(*outs)), 'two launches differ'
    return outs[0]


@pytest.mark.parametrize('O', [1, 3, 16])
@pytest.mark.parametrize('K', [7, 64, 100, 300])
@pytest.mark.parametrize('R', [1, 63, 65, 200])
def test_tail_bwd_alone(R, K, O):
    """Rows: one (three idle waves), a wave short of 16 blocks, one past, the training step's; K: a partial wave with the bias column in
    it, the bias column alone in a second column block (64), two and five column blocks; outputs: one, a few, the most."""
    dout, x, W, want, bound = _tail_case(R, K, O)
    for relu in (1, 0):
        dx, dW, db = _tail_bwd(dout, x, W, relu)
        key = 'dx_relu' if relu else 'dx'
        assert _report(f'tail_bwd dx R={R} K={K} O={O} relu={relu}', dx, want[key], bound[key]) <= 1.0
        assert _report(f'tail_bwd dW R={R} K={K} O={O}', dW, want['dW'], bound['dW']) <= 1.0
        assert _report(f'tail_bwd db R={R} K={K} O={O}', db, want['db'], bound['db']) <= 1.0
        if relu:
            assert (dx.cpu()[x == 0] == 0).all()  # h == 0 gives exactly 0: whole rows among them
            if R > 2:
                assert (dx.cpu()[2] == 0).all()


def test_tail_bwd_skips_what_is_null_and_writes_nothing_for_no_rows():
    lib, native = _lib()
    dout, x, W, want, bound = _tail_case(65, 100, 3)
    dx, dW, db = _tail_bwd(dout, x, W, 1, want_dx=False)
    assert torch.isnan(dx).all() and _report('tail_bwd dW alone', dW, want['dW'], bound['dW']) <= 1.0
    full = _tail_bwd(dout, x, W, 1)
    assert _same_bits(dW, full[1]) and _same_bits(db, full[2])
    dx, dW, db = _tail_bwd(dout, x, W, 1, want_sums=False)
    assert torch.isnan(dW).all() and torch.isnan(db).all() and _same_bits(dx, full[0])
    dx, dW, db = _tail_bwd(dout[:0], x[:0], W, 1)  # R = 0
    assert torch.isnan(dx).all() and torch.isnan(dW).all() and torch.isnan(db).all()


# ---- tgmx_decoder_scatter alone -------------------------------------------------------------------------------------------------------------------
def _scatter(dh, ia, ib, NP):
    lib, native = _lib()
    R, H = dh.shape
    bh = Buf(R, H, ld=H + 4, lead=0, fill=7.0, data=dh)
    nbytes = lib.tgmx_decoder_scatter_workspace_bytes(R, NP, H)
    assert nbytes > 0 and nbytes % 4 == 0
    ia_d, ib_d = ia.to(DEV), ib.to(DEV)
    outs = []
    for _ in range(2):
        dP, ws = Buf(NP, 2 * H), Buf(1, nbytes // 4)
        native.check(lib.tgmx_decoder_scatter(bh.ptr, bh.ld, R, H, ia_d.data_ptr(), ib_d.data_ptr(), int(ia.dtype == torch.int64), NP, dP.ptr,
                                              ws.ptr, nbytes, native.stream_ptr()), 'tgmx_decoder_scatter')  # fmt: skip
        torch.cuda.synchronize()
        assert dP.sentinels_intact() and ws.sentinels_intact(), 'a write outside dP or past the workspace'
        outs.append(dP.view.clone())
    assert _same_bits(outs[0], outs[1]), 'two launches differ'
    return outs[0]


def _scatter_want(dh, ia, ib, NP):
    """dP [NP, 2H] in float64 and its bound; pairs with an index outside the table take no part"""
    R, H = dh.shape
    ia, ib = ia.long(), ib.long()
    keep = (ia >= 0) & (ia < NP) & (ib >= 0) & (ib < NP)
    d = dh.double()[keep]
    want, bound = torch.zeros(NP, 2 * H, dtype=F64), torch.zeros(NP, 2 * H, dtype=F64)
    for half, ix in enumerate((ia[keep], ib[keep])):
        counts = torch.bincount(ix, minlength=NP)
        n = torch.tensor([br.scatter_chain(int(c), 2 * R) for c in counts], dtype=F64)
        want[:, half * H : (half + 1) * H].index_add_(0, ix, d)
        bound[:, half * H : (half + 1) * H].index_add_(0, ix, d.abs())
        bound[:, half * H : (half + 1) * H] *= (n * br.U / (1 - n * br.U)).unsqueeze(1)
    return want, bound


@pytest.mark.parametrize('idx', [torch.int32, torch.int64])
@pytest.mark.parametrize('NP,R', [(1, 1), (7, 65), (64, 400), (600, 400)])
def test_scatter_alone(NP, R, idx):
    """One row, one pair; more pairs than rows (rows of ~9 and ~6 pairs); a table larger than the pair list (most rows empty).  H = 32
    reads float4, H = 7 float by float.  With more than two pairs: one pair with a == b, one row that no pair names, one index outside."""
    for H in (32, 7):
        g = torch.Generator().manual_seed(NP * 1000 + R + H)
        dh = torch.randn(R, H, generator=g)
        lo = 1 if NP > 1 else 0  # row 0 stays without a pair
        ia, ib = torch.randint(lo, NP, (R,), generator=g), torch.randint(lo, NP, (R,), generator=g)
        if R > 2:
            ib[0] = ia[0]
            ia[1] = NP  # outside: the pair (1) is dropped from BOTH halves, nothing is read through either index
            ib[2] = -1
        want, bound = _scatter_want(dh, ia, ib, NP)
        got = _scatter(dh, ia.to(idx), ib.to(idx), NP)
        assert _report(f'scatter NP={NP} R={R} H={H} {idx}', got, want, bound) <= 1.0
        if NP > 1:
            assert (got[0] == 0).all()  # a row without a pair: exact zeros, written by the kernel
        if R > 2:
            a = int(ia[0])
            only_a = (ia == a).sum() == 1 and (ib == a).sum() == 1
            if only_a:  # the pair (a, a) alone in its row lands in both halves as it is
                assert torch.equal(got[a, :H].cpu(), dh[0]) and torch.equal(got[a, H:].cpu(), dh[0])
        assert _same_bits(got, _scatter(dh, ia.to(idx), ib.to(idx), NP))


@pytest.mark.parametrize('R', [br.LONG_ROW + 1, br.VERY_LONG + 1])
def test_scatter_hub_row(R):
    """One table row holds every pair's left index: past kSpmmLongRow the four waves split it, past kSpmmVeryLong the chunk launches do
    (its right indices spread over the table)."""
    NP, H = 5, 32
    g = torch.Generator().manual_seed(R)
    dh = torch.randn(R, H, generator=g)
    ia, ib = torch.full((R,), 3), torch.randint(0, NP, (R,), generator=g)
    want, bound = _scatter_want(dh, ia, ib, NP)
    got = _scatter(dh, ia.int(), ib.int(), NP)
    assert _report(f'scatter hub R={R}', got, want, bound) <= 1.0
    assert (got[[0, 1, 2, 4], :H] == 0).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
def link_model(D=24, H=32, merge='concat', seed=0, **kw):
    from tgm_amd.nn import LinkPredictor
    from tgm_amd.nn.modules import ConcatMerge, LearnableSumMerge

    torch.manual_seed(seed)
    return LinkPredictor(D, hidden_dim=H, merge_op=(ConcatMerge if merge == 'concat' else LearnableSumMerge)(D), **kw).to(DEV).train()


def node_model(seed=0, **kw):
    from tgm_amd.nn import NodePredictor

    torch.manual_seed(seed)
    return NodePredictor(**kw).to(DEV).train()


def cpu_sd(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def is_native(t) -> bool:
    return 'DecoderFunction' in type(t.grad_fn).__name__


def f32_autograd(sd, kind, op, inputs, dout, idx=None):
    """float32 autograd of the restated forward on the CPU: name -> gradient (the parity ratio's yardstick)"""
    sd = {k: v.clone().requires_grad_() for k, v in sd.items()}
    ins = {k: v.clone().requires_grad_() for k, v in inputs.items()}
    if kind == 'node':
        out = dr.node(sd, ins['z'], torch.float32)
    elif idx is not None:
        out = dr.link(sd, op, ins['z'][idx[0].long()], ins['z'][idx[1].long()], torch.float32)
    else:
        out = dr.link(sd, op, ins['z_src'], ins['z_dst'], torch.float32)
    out.backward(dout.reshape(out.shape))
    return {**{k: v.grad for k, v in sd.items()}, **{k: v.grad for k, v in ins.items()}}


def check_grads(tag, model, kind, op, inputs, dout, got, idx=None, sd=None):
    """Every gradient in ``got`` (name -> device tensor) against the restatement under its bound; prints the parity ratios."""
    sd = cpu_sd(model) if sd is None else sd
    cpu_in = {k: v.detach().cpu() for k, v in inputs.items()}
    cpu_idx = None if idx is None else tuple(t.cpu() for t in idx)
    want = br.head_grads(sd, kind, op, cpu_in, dout.detach().cpu(), idx=cpu_idx)
    in_range = cpu_idx is None or all(bool(((t >= 0) & (t < cpu_in['z'].shape[0])).all()) for t in cpu_idx)
    f32 = f32_autograd(sd, kind, op, cpu_in, dout.detach().cpu(), cpu_idx) if in_range else None  # (autograd cannot drop a pair)
    assert set(got) == set(want), (sorted(got), sorted(want))
    worst = 0.0
    for k, (val, bound) in want.items():
        assert got[k] is not None, (tag, k)
        worst = max(worst, _report(f'{tag} d {k}', got[k], val, bound))
        if f32 is not None:
            d_hip, d_f32 = dr.rel_err(got[k].detach().cpu(), val), dr.rel_err(f32[k], val)
            print(f'decoder grad parity {tag} {k}: hip {d_hip:.3e} float32 {d_f32:.3e} ratio {d_hip / max(d_f32, 1e-30):.2f}')
    assert worst <= 1.0, (tag, worst)


def grads_of(model, inputs):
    return {**{k: p.grad for k, p in model.named_parameters()}, **{k: v.grad for k, v in inputs.items()}}


CONFIGS = [dict(merge='concat'), dict(merge='concat', nlayers=3, out_dim=3), dict(merge='concat', out_dim=20), dict(merge='sum'), dict(merge='sum', nlayers=3)]


@pytest.mark.parametrize('form', ['forward', 'table', 'pair'])
@pytest.mark.parametrize('cfg', CONFIGS, ids=lambda c: '-'.join(f'{k}={v}' for k, v in c.items()))
def test_link_gradients_end_to_end(cfg, form, monkeypatch):
    """D = 24, H = 32, R = 30: forward(z_src, z_dst), and score_pairs over a table of 17 rows with the form pinned."""
    model = link_model(seed=3, **cfg)
    g = torch.Generator().manual_seed(12)
    R, D, out_dim = 30, 24, cfg.get('out_dim', 1)
    dout = torch.randn(R * out_dim, generator=g).to(DEV)
    if form == 'forward':
        inputs = {k: torch.randn(R, D, generator=g).to(DEV).requires_grad_() for k in ('z_src', 'z_dst')}
        out = model(inputs['z_src'], inputs['z_dst'])
        idx = None
    else:
        monkeypatch.setenv('TGMX_DECODER_FORM', form)
        inputs = {'z': torch.randn(17, D, generator=g).to(DEV).requires_grad_()}
        idx = (torch.randint(0, 17, (R,), generator=g).to(DEV), torch.randint(0, 17, (R,), generator=g).to(DEV))
        out = model.score_pairs(inputs['z'], *idx)
    assert out.shape == (R * out_dim,) and (is_native(out) or form == 'pair')  # (pair: torch's index backward sits on top)
    (out * dout).sum().backward()
    model.check()
    check_grads(f'{cfg} {form}', model, 'link', cfg['merge'], inputs, dout, grads_of(model, inputs), idx)


@pytest.mark.parametrize('kw', [dict(in_dim=24, out_dim=2), dict(in_dim=7, nlayers=4, hidden_dim=33)], ids=['in24-out2', 'in7-deep'])
def test_node_gradients_end_to_end(kw):
    model = node_model(seed=4, **kw)
    g = torch.Generator().manual_seed(13)
    z = torch.randn(5, 6, kw['in_dim'], generator=g).to(DEV).requires_grad_()  # leading dimensions as the reference takes them
    out = model(z)
    assert is_native(out) and out.shape == (5, 6, kw.get('out_dim', 1))
    dout = torch.randn(out.shape, generator=g).to(DEV)
    out.backward(dout)
    check_grads(f'node {kw}', model, 'node', None, {'z': z}, dout, grads_of(model, {'z': z}))


def test_training_step_at_the_examples_dims(monkeypatch):
    """D = H = 100, B = 200, z [600, D]: positives and negatives and BCE exactly as examples/linkproppred/tgat.py's train() -- as two
    forward calls, and as one score_pairs over the table (2 B pairs into 3 B rows)."""
    B, D = 200, 100
    model = link_model(D=D, H=D, seed=5)
    sd = cpu_sd(model)
    g = torch.Generator().manual_seed(14)
    z0 = torch.randn(3 * B, D, generator=g).to(DEV)
    ar = torch.arange(B, device=DEV)
    # (a) the example's two calls; the upstream gradients are read off the outputs
    z = z0.clone().requires_grad_()
    z_src, z_dst, z_neg = z[:B], z[B : 2 * B], z[2 * B :]
    pos_out, neg_out = model(z_src, z_dst), model(z_src, z_neg)
    assert is_native(pos_out) and is_native(neg_out)
    pos_out.retain_grad(), neg_out.retain_grad()
    loss = F.binary_cross_entropy_with_logits(pos_out, torch.ones_like(pos_out))
    loss += F.binary_cross_entropy_with_logits(neg_out, torch.zeros_like(neg_out))
    loss.backward()
    ia, ib = torch.cat((ar, ar)), torch.cat((ar + B, ar + 2 * B))
    two_calls = grads_of(model, {'z': z})
    zc = z0.cpu()
    w1 = br.head_grads(sd, 'link', 'concat', {'z_src': zc[:B], 'z_dst': zc[B : 2 * B]}, pos_out.grad.cpu())
    w2 = br.head_grads(sd, 'link', 'concat', {'z_src': zc[:B], 'z_dst': zc[2 * B :]}, neg_out.grad.cpu())

    def both(k):  # autograd adds the two calls' gradients: one more float32 addition
        val = w1[k][0] + w2[k][0]
        return val, w1[k][1] + w2[k][1] + br.U * val.abs()

    for k in sd:
        assert _report(f'example dims, two calls, d {k}', two_calls[k], *both(k)) <= 1.0
    dz = two_calls['z'].cpu()
    assert _report('example dims, two calls, d z_src', dz[:B], *both('z_src')) <= 1.0
    assert _report('example dims, two calls, d z_dst', dz[B : 2 * B], *w1['z_dst']) <= 1.0
    assert _report('example dims, two calls, d z_neg', dz[2 * B :], *w2['z_dst']) <= 1.0
    # (b) one score_pairs call over the table
    monkeypatch.setenv('TGMX_DECODER_FORM', 'table')
    model.zero_grad()
    z = z0.clone().requires_grad_()
    out = model.score_pairs(z, ia, ib)
    assert is_native(out)
    out.retain_grad()
    target = torch.cat((torch.ones(B), torch.zeros(B))).to(DEV)
    (2 * F.binary_cross_entropy_with_logits(out, target)).backward()  # the mean over 2 B pairs, twice: the sum of the two calls' means
    check_grads('example dims, one score_pairs', model, 'link', 'concat', {'z': z}, out.grad, grads_of(model, {'z': z}), (ia, ib), sd=sd)


@pytest.mark.parametrize('name', br.EXPECTED_GRAD_FIXTURES)
def test_recorded_gradients(name):
    from test_decoders_gpu import build

    meta, sd, inputs, dout, grads = br.load_grad_fixture(name)
    model = build(meta, sd).train()
    dev_in = {k: v.to(DEV).requires_grad_() for k, v in inputs.items()}
    out = model(*dev_in.values())
    assert is_native(out)
    out.backward(dout.to(DEV))
    got = grads_of(model, dev_in)
    for k, ref in grads.items():
        dr.close(got[k].cpu(), ref, f'{name} {k} against the record')
    check_grads(name, model, meta['kind'], meta['op'], dev_in, dout, got, sd=sd)


# ---- what belongs to the call ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('merge', ['concat', 'sum'])
def test_two_calls_then_one_backward(merge):
    """A positive and a negative call on ONE module before one backward: each call's backward must read its own activations (shared
    buffers would hand the first call the second's)."""
    model = link_model(merge=merge, seed=6, nlayers=3)
    sd = cpu_sd(model)
    g = torch.Generator().manual_seed(15)
    a, b, c = (torch.randn(30, 24, generator=g).to(DEV).requires_grad_() for _ in range(3))
    d1, d2 = torch.randn(30, generator=g).to(DEV), torch.randn(30, generator=g).to(DEV)
    pos, neg = model(a, b), model(a, c)
    ((pos * d1).sum() + (neg * d2).sum()).backward()
    w1 = br.head_grads(sd, 'link', merge, {'z_src': a.detach().cpu(), 'z_dst': b.detach().cpu()}, d1.cpu())
    w2 = br.head_grads(sd, 'link', merge, {'z_src': a.detach().cpu(), 'z_dst': c.detach().cpu()}, d2.cpu())
    got = grads_of(model, {})
    for k in sd:  # each is the float32 sum of the two calls' gradients
        val, bound = w1[k][0] + w2[k][0], w1[k][1] + w2[k][1] + br.U * (w1[k][0] + w2[k][0]).abs()
        assert _report(f'two calls {merge} d {k}', got[k], val, bound) <= 1.0
    assert _report('two calls d z_src', a.grad, w1['z_src'][0] + w2['z_src'][0], w1['z_src'][1] + w2['z_src'][1] + br.U * (w1['z_src'][0] + w2['z_src'][0]).abs()) <= 1.0
    assert _report('two calls d z_dst', b.grad, *w1['z_dst']) <= 1.0
    assert _report('two calls d z_neg', c.grad, *w2['z_dst']) <= 1.0


def test_requires_grad_subsets():
    model = link_model(seed=7, nlayers=3)
    g = torch.Generator().manual_seed(16)
    a, b = torch.randn(30, 24, generator=g).to(DEV), torch.randn(30, 24, generator=g).to(DEV).requires_grad_()
    dout = torch.randn(30, generator=g).to(DEV)
    model.model[2].weight.requires_grad_(False)
    out = model(a, b)  # z_src without grad, one frozen parameter
    assert is_native(out)
    out.backward(dout)
    assert a.grad is None and model.model[2].weight.grad is None
    want = br.head_grads(cpu_sd(model), 'link', 'concat', {'z_src': a.cpu(), 'z_dst': b.detach().cpu()}, dout.cpu())
    got = grads_of(model, {'z_dst': b})
    for k, (val, bound) in want.items():
        if k not in ('z_src', 'model.2.weight'):
            assert _report(f'subset d {k}', got[k], val, bound) <= 1.0
    # only the inputs require grad: no parameter gradient is formed
    model.zero_grad()
    for p in model.parameters():
        p.requires_grad_(False)
    a.requires_grad_()
    out = model(a, b)
    assert is_native(out)
    out.backward(dout)
    assert all(p.grad is None for p in model.parameters())
    assert _report('inputs only d z_src', a.grad, *want['z_src']) <= 1.0
    # nothing requires grad, or no_grad: the inference path, today's bits
    x, y = a.detach(), b.detach()
    plain = model(x, y)
    assert not plain.requires_grad
    for p in model.parameters():
        p.requires_grad_(True)
    with torch.no_grad():
        quiet = model(x, y)
    assert not quiet.requires_grad and _same_bits(quiet, plain)
    dr.close(quiet.cpu(), out.detach().cpu(), 'inference against the saving forward')


@pytest.mark.parametrize('nlayers', [2, 3])
def test_index_outside_the_table_in_gradient_mode(nlayers, monkeypatch):
    """Forward as without gradients: the score is NaN and check() raises (with a hidden layer behind the merge stage the GEMM's ReLU
    epilogue turns the NaN row into zeros, with and without gradients: only check() tells).  Backward: the pair takes no part in any
    gradient, whatever the upstream gradient of its row holds."""
    monkeypatch.setenv('TGMX_DECODER_FORM', 'table')
    model = link_model(seed=8, nlayers=nlayers)
    g = torch.Generator().manual_seed(17)
    z = torch.randn(17, 24, generator=g).to(DEV).requires_grad_()
    ia, ib = torch.randint(0, 17, (30,), generator=g).to(DEV), torch.randint(0, 17, (30,), generator=g).to(DEV)
    ia[4], ib[9] = 17, -3
    out = model.score_pairs(z, ia, ib)
    assert is_native(out) and torch.isfinite(out[[0, 1, 2, 3, 5, 6, 7, 8] + list(range(10, 30))]).all()
    with torch.no_grad():
        quiet = model.score_pairs(z, ia, ib)
    assert torch.equal(torch.isnan(out), torch.isnan(quiet)) and (nlayers > 2 or torch.isnan(out[[4, 9]]).all())
    with pytest.raises(ValueError, match='outside'):
        model.check()
    dout = torch.randn(30, generator=g).to(DEV)
    dout[4] = NAN
    out.backward(dout)
    check_grads('dropped pairs', model, 'link', 'concat', {'z': z}, dout, grads_of(model, {'z': z}), (ia, ib))


# ---- dispatch -------------------------------------------------------------------------------------------------------------------------------------
def test_dispatch(monkeypatch):
    cases = []
    for cfg in CONFIGS:
        cases += [(link_model(seed=9, **cfg), form) for form in ('forward', 'table')]
    cases.append((node_model(seed=9, in_dim=24, out_dim=2, nlayers=3), 'rows'))
    g = torch.Generator().manual_seed(18)
    z0 = torch.randn(17, 24, generator=g).to(DEV)
    ia, ib = torch.randint(0, 17, (30,), generator=g).to(DEV), torch.randint(0, 17, (30,), generator=g).to(DEV)

    def run(model, form):
        model.zero_grad()
        z = z0.clone().requires_grad_()
        if form == 'forward':
            out = model(z[ia], z[ib])
        elif form == 'table':
            out = model.score_pairs(z, ia, ib)
        else:
            out = model(z)
        out.square().sum().backward()
        return out, [z.grad] + [p.grad for p in model.parameters()]

    monkeypatch.setenv('TGMX_DECODER_FORM', 'table')
    for model, form in cases:
        monkeypatch.delenv('TGMX_DECODER_BWD', raising=False)
        out, one = run(model, form)
        assert is_native(out)
        _, again = run(model, form)
        monkeypatch.setenv('TGMX_DECODER_BWD', 'py')
        out_py, by_launch = run(model, form)
        assert is_native(out_py)
        monkeypatch.setenv('TGMX_DECODER_BWD', 'torch')
        out_t, composed = run(model, form)
        assert not is_native(out_t)
        for a, b, c, d in zip(one, again, by_launch, composed):
            assert _same_bits(a, b), (form, 'two runs differ')
            assert _same_bits(a, c), (form, 'the launches issued one by one give other bits')
            dr.close(a.cpu(), d.cpu(), f'{form} against the composed path')
    # outside the envelope: the composed path, without error
    monkeypatch.delenv('TGMX_DECODER_BWD', raising=False)
    model = link_model(seed=9)
    z = z0.clone().requires_grad_()
    assert not is_native(model.query_one_vs_many(z, ia[:3], ib[:3], ib[3:9].view(3, 2)))
    with torch.autocast('cuda', dtype=torch.bfloat16):
        assert not is_native(model(z[ia], z[ib]))
    assert not is_native(model.double()(z.double()[ia], z.double()[ib]))
