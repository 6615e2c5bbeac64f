"""LinkPredictor / NodePredictor / GraphPredictor on the device against the float64 restatement (tests/decoders_restate.py): the reference's
recorded outputs (g26 fixtures), the pair GEMM, the score kernel and the pooling alone at the shapes that reach each of their branches, the
two forms of the pair head against each other, ``query_one_vs_many`` against ``score_pairs`` and against the examples' per-positive loop,
the one-call forward against the same launches issued from Python, determinism, the index range check, and the torch paths."""
import pytest
import torch

import decoders_restate as dr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# The parity bar of tests/test_roland_gpu.py.  Ratio: the device's distance from the float64 restatement against the float32 restatement's
# own, 2.0 wherever the latter is measurable (>= 1e-7).  Absolute: close()'s 1e-5 of max(1, |ref|).
RATIO_BAR, NOISE_FLOOR, ABS_BAR = 2.0, 1e-7, 1e-5


def bar(got, ref, f32, label):
    got = got.detach().cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32 and torch.isfinite(got).all(), label
    d_hip, d_f32 = dr.rel_err(got, ref), dr.rel_err(f32, ref)
    print(f'decoder parity {label}: hip {d_hip:.3e} float32 {d_f32:.3e} ratio {d_hip / max(d_f32, 1e-30):.2f}')
    assert d_hip <= ABS_BAR, (label, d_hip)
    if d_f32 >= NOISE_FLOOR:
        assert d_hip <= RATIO_BAR * d_f32, (label, d_hip, d_f32)


def build(meta, sd):
    from tgm_amd.nn import GraphPredictor, LinkPredictor, NodePredictor
    from tgm_amd.nn.modules import ConcatMerge, LearnableSumMerge, MeanEmbdPooling, SumEmbdPooling

    kw, op = meta['kw'], meta['op']
    if meta['kind'] == 'link':
        model = LinkPredictor(**kw, merge_op=(ConcatMerge if op == 'concat' else LearnableSumMerge)(kw['node_dim']))
    elif meta['kind'] == 'node':
        model = NodePredictor(**kw)
    else:
        model = GraphPredictor(**kw, graph_pooling=(MeanEmbdPooling if op == 'mean' else SumEmbdPooling)(kw['in_dim']))
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).eval()


def link_model(D=24, H=32, merge='concat', seed=0, **kw):
    from tgm_amd.nn import LinkPredictor
    from tgm_amd.nn.modules import ConcatMerge, LearnableSumMerge

    torch.manual_seed(seed)
    model = LinkPredictor(D, hidden_dim=H, merge_op=(ConcatMerge if merge == 'concat' else LearnableSumMerge)(D), **kw)
    return model.to(DEV).eval()


def cpu_sd(model):
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


# ---- the reference's recorded outputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', dr.EXPECTED_FIXTURES)
def test_fixture(name):
    meta, sd, inputs, out = dr.load_fixture(name)
    model = build(meta, sd)
    with torch.no_grad():
        got = model(*(v.to(DEV) for v in inputs.values()))
    model.check()
    assert not got.requires_grad
    dr.close(got.cpu(), out, f'{name} against the record')
    bar(got, dr.restate(meta, sd, inputs), dr.restate(meta, sd, inputs, torch.float32), name)


# ---- tgmx_decoder_pair_gemm alone ---------------------------------------------------------------------------------------------------------------
def pair_gemm(A1, ia, A2, ib, Wa, Wb, bias, act, R, bad=None):
    from tgm_amd import _native

    N = Wa.shape[0]
    C = torch.full((R, N + 3), -7.0, device=DEV)  # a wider leading dimension: nothing may be written past column N
    p = _native.ptr
    rc = _native.load().tgmx_decoder_pair_gemm(p(A1), A1.stride(0), A1.shape[0], p(ia), p(A2), 0 if A2 is None else A2.stride(0),
                                               0 if A2 is None else A2.shape[0], p(ib), p(Wa), Wa.stride(0), Wa.shape[1], p(Wb),
                                               0 if Wb is None else Wb.stride(0), 0 if Wb is None else Wb.shape[1], p(bias), act, p(C), C.stride(0),
                                               R, N, p(bad), _native.stream_ptr())  # fmt: skip
    _native.check(rc, 'tgmx_decoder_pair_gemm')
    assert (C[:, N:] == -7.0).all()
    return C[:, :N]


@pytest.mark.parametrize('N', [7, 33, 64, 100])
@pytest.mark.parametrize('D', [5, 172])
@pytest.mark.parametrize('R', [1, 63, 65, 200])
def test_pair_gemm_alone(R, D, N):
    """Rows: one, a block short of two, one past two blocks, many; K: one partial 64-chunk, two full ones and a tail; columns: a partial
    wave, partial block, one block, two."""
    g = torch.Generator().manual_seed(1000 * R + 10 * D + N)
    rows = 40
    A1, A2 = torch.randn(rows, D, generator=g), torch.randn(rows + 3, D, generator=g)
    Wa, Wb, bias = (torch.empty(s).uniform_(-0.3, 0.3, generator=g) for s in ((N, D), (N, D), (N,)))
    ia, ib = torch.randint(0, rows, (R,), generator=g), torch.randint(0, rows + 3, (R,), generator=g)
    if R > 2:
        ia[1], ib[2] = ia[0], ib[0]  # repeated indices
    X1, X2 = torch.randn(R, D, generator=g), torch.randn(R, D, generator=g)  # the operands already gathered: no indices
    d = lambda t: None if t is None else t.to(DEV)
    for indexed in (True, False):
        for two in (True, False):
            for act in (0, 1):
                a1, a2 = (A1[ia], A2[ib]) if indexed else (X1, X2)
                outs = {}
                for dt in (torch.float64, torch.float32):
                    s = a1.to(dt) @ Wa.to(dt).t() + bias.to(dt)
                    if two:
                        s = s + a2.to(dt) @ Wb.to(dt).t()
                    outs[dt] = torch.relu(s) if act else s
                got = pair_gemm(d(A1 if indexed else X1), d(ia.int()) if indexed else None, (d(A2 if indexed else X2) if two else None),
                                (d(ib.int()) if indexed and two else None), d(Wa), d(Wb) if two else None, d(bias), act, R)  # fmt: skip
                bar(got, outs[torch.float64], outs[torch.float32], f'pair gemm R={R} D={D} N={N} idx={indexed} two={two} act={act}')


# ---- tgmx_decoder_score alone -------------------------------------------------------------------------------------------------------------------
def score(P, H, ia, ib, neg, off, M, most, B, R, wl=None, bl=None, act=1, bad=None):
    from tgm_amd import _native

    O = 0 if wl is None else wl.shape[0]
    out = torch.full((R, O if O else H), -7.0, device=DEV)
    p = _native.ptr
    rc = _native.load().tgmx_decoder_score(p(P), P.stride(0), P.shape[0], H, p(ia), p(ib), p(neg), int(ia.dtype == torch.int64), p(off), M, most, B, act,
                                           p(wl), p(bl), O, p(out), out.stride(0), p(bad), _native.stream_ptr())  # fmt: skip
    _native.check(rc, 'tgmx_decoder_score')
    return out


def flat_pairs(src, dst, negs):
    ia = torch.cat([src[b].repeat(1 + len(negs[b])) for b in range(len(src))])
    ib = torch.cat([torch.cat([dst[b : b + 1], negs[b]]) for b in range(len(src))])
    return ia, ib


@pytest.mark.parametrize('idx', [torch.int32, torch.int64])
@pytest.mark.parametrize('H', [7, 16, 64, 100, 300])
def test_score_alone(H, idx):
    """Several pairs per wave (7, 16), one pair per wave with and without a second pass over the lanes (64, 100, 300); fixed M = 0, 1, 20,
    ragged lists with an empty and a single-element one; the unfused output is one float32 addition: equal bits."""
    g = torch.Generator().manual_seed(H)
    NP, B = 37, 6
    P = torch.randn(NP, 2 * H, generator=g)
    src, dst = torch.randint(0, NP, (B,), generator=g), torch.randint(0, NP, (B,), generator=g)
    lists = {f'M={M}': [torch.randint(0, NP, (M,), generator=g) for _ in range(B)] for M in (0, 1, 20)}
    lists['ragged'] = [torch.randint(0, NP, (n,), generator=g) for n in (3, 0, 1, 300, 0, 7)]  # 300: a second chunk of candidates
    d = lambda t: t.to(DEV)
    for label, negs in lists.items():
        ia, ib = flat_pairs(src, dst, negs)
        R = ia.numel()
        h64 = torch.relu(P.double()[ia, :H] + P.double()[ib, H:])
        h32 = torch.relu(P[ia, :H] + P[ib, H:])
        sizes = [len(n) for n in negs]
        ragged = label == 'ragged'
        off = d(torch.tensor([0] + sizes).cumsum(0)) if ragged else None
        M = 0 if ragged else sizes[0]
        neg = d(torch.cat(negs).to(idx))
        args = (d(P), H, d(src.to(idx)), d(dst.to(idx)), neg, off, M, max(sizes), B, R)
        flat_args = (d(P), H, d(ia.to(idx)), d(ib.to(idx)), None, None, -1, 0, R, R)
        assert torch.equal(score(*args).cpu(), h32), (H, label)
        assert torch.equal(score(*flat_args).cpu(), h32), (H, label, 'flat')
        assert torch.equal(score(*args, act=0).cpu(), P[ia, :H] + P[ib, H:]), (H, label, 'no activation')
        for O in (1, 3, 16):
            wl, bl = torch.empty(O, H).uniform_(-0.3, 0.3, generator=g), torch.empty(O).uniform_(-0.3, 0.3, generator=g)
            got = score(*args, wl=d(wl), bl=d(bl))
            assert torch.equal(got, score(*flat_args, wl=d(wl), bl=d(bl))), (H, label, O)  # grouped and flat: the same bits
            bar(got, h64 @ wl.double().t() + bl.double(), h32 @ wl.t() + bl, f'score H={H} {label} out={O} {idx}')


# ---- tgmx_pool_rows alone -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 41, 128, 129, 1000])
@pytest.mark.parametrize('D', [5, 128, 300])
def test_pool_rows_alone(N, D):
    from tgm_amd import _native

    lib = _native.load()
    x = torch.randn(N, D, generator=torch.Generator().manual_seed(N + D))
    xd = x.to(DEV)
    for mean in (1, 0):
        outs = []
        for _ in range(2):
            n = lib.tgmx_pool_rows_scratch_floats(N, D)
            assert (n > 0) == (N > 128)
            ws, out = torch.empty(max(n, 1), device=DEV), torch.empty(D, device=DEV)
            _native.check(lib.tgmx_pool_rows(xd.data_ptr(), D, N, D, mean, ws.data_ptr(), n, out.data_ptr(), _native.stream_ptr()), 'tgmx_pool_rows')
            outs.append(out)
        assert torch.equal(outs[0], outs[1])
        ref, f32 = (x.double().mean(0), x.mean(0)) if mean else (x.double().sum(0), x.sum(0))
        bar(outs[0], ref, f32, f'pool N={N} D={D} mean={mean}')


# ---- the two forms, score_pairs, query_one_vs_many ----------------------------------------------------------------------------------------------
def eval_case(seed, NP=50, B=9, D=24):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(NP, D, generator=g)
    src, dst = torch.randint(0, NP, (B,), generator=g), torch.randint(0, NP, (B,), generator=g)
    fixed = torch.randint(0, NP, (B, 20), generator=g)
    ragged = [torch.randint(0, NP, (n,), generator=g) for n in (3, 0, 1, 40, 0, 7, 2, 300, 5)]
    return z, src, dst, fixed, ragged


CONFIGS = [dict(merge='concat'), dict(merge='concat', nlayers=3, out_dim=3), dict(merge='concat', out_dim=20), dict(merge='sum'), dict(merge='sum', nlayers=3)]


@pytest.mark.parametrize('cfg', CONFIGS, ids=lambda c: '-'.join(f'{k}={v}' for k, v in c.items()))
def test_forms_and_one_vs_many(cfg, monkeypatch):
    model = link_model(seed=3, **cfg)
    sd, op = cpu_sd(model), cfg['merge']
    z, src, dst, fixed, ragged = eval_case(5)
    d = lambda t: t.to(DEV)
    for negs in (list(fixed), ragged):
        ia, ib = flat_pairs(src, dst, negs)
        ref, f32 = dr.link(sd, op, z[ia], z[ib]), dr.link(sd, op, z[ia], z[ib], torch.float32)
        with torch.no_grad():
            loop = torch.cat(dr.one_vs_many_loop(model, d(z), d(src), d(dst), [d(n) for n in negs]))  # the examples' loop, on the device
        bar(loop, ref, f32, f'{cfg} per-positive loop')
        for form in ('table', 'pair'):
            monkeypatch.setenv('TGMX_DECODER_FORM', form)
            with torch.no_grad():
                flat = model.score_pairs(d(z), d(ia), d(ib))
                flat32 = model.score_pairs(d(z), d(ia.int()), d(ib.int()))
                many = model.query_one_vs_many(d(z), d(src), d(dst), d(fixed) if negs is not ragged else [d(n) for n in negs])
                again = model.query_one_vs_many(d(z), d(src.int()), d(dst.int()), d(fixed.int()) if negs is not ragged else [d(n.int()) for n in negs])
            bar(flat, ref, f32, f'{cfg} score_pairs {form}')  # both forms within the bar
            assert torch.equal(flat, flat32)
            if negs is ragged:
                assert [t.numel() for t in many] == [(len(n) + 1) * cfg.get('out_dim', 1) for n in negs]
                assert all(t.untyped_storage().data_ptr() == many[0].untyped_storage().data_ptr() for t in many)  # views of one buffer
                many, again = torch.cat(many), torch.cat(again)
            else:
                assert tuple(many.shape) == (len(src), 21 * cfg.get('out_dim', 1))
            assert torch.equal(many.reshape(-1), flat)  # one-vs-many IS score_pairs on the flattened pairs, bit for bit
            assert torch.equal(again.reshape(-1), flat)  # two runs, int32 indices: the same bits
            dr.close(many.reshape(-1).cpu(), loop.cpu(), f'{cfg} {form} against the loop')
    model.check()


def test_default_form_follows_the_table_size():
    model = link_model()
    assert model._form(10, 10) == 'table' and model._form(20, 10) == 'table' and model._form(21, 10) == 'pair'  # N' <= 2 R, as measured
    assert link_model(H=600)._form(10, 100) == 'pair'  # a half row wider than the score kernel keeps


# ---- one call against the same launches from Python ---------------------------------------------------------------------------------------------
def test_one_call_forward_equals_the_launches_issued_one_by_one(monkeypatch):
    from tgm_amd.nn import GraphPredictor, NodePredictor
    from tgm_amd.nn.modules import SumEmbdPooling

    z, src, dst, fixed, ragged = (t.to(DEV) if isinstance(t, torch.Tensor) else [n.to(DEV) for n in t] for t in eval_case(7))
    torch.manual_seed(1)
    calls = []
    for cfg in CONFIGS:
        model = link_model(seed=2, **cfg)
        calls += [lambda m=model: m(z[:40], z[10:50]), lambda m=model: torch.cat(m.query_one_vs_many(z, src, dst, ragged))]
        for form in ('table', 'pair'):
            calls.append(lambda m=model, f=form: (monkeypatch.setenv('TGMX_DECODER_FORM', f), m.query_one_vs_many(z, src, dst, fixed))[1])
    node = NodePredictor(24, 10, nlayers=3).to(DEV).eval()
    wide = NodePredictor(24, 40).to(DEV).eval()
    graph = GraphPredictor(24, 2, graph_pooling=SumEmbdPooling(24)).to(DEV).eval()
    big = torch.randn(300, 24, device=DEV)
    calls += [lambda: node(z), lambda: wide(z), lambda: graph(z), lambda: graph(big)]
    for i, call in enumerate(calls):
        monkeypatch.delenv('TGMX_DECODER_FORM', raising=False)
        monkeypatch.delenv('TGMX_DECODER_PY', raising=False)
        with torch.no_grad():
            one = call()
            twice = call()
            monkeypatch.setenv('TGMX_DECODER_PY', '1')
            by_launch = call()
        assert torch.isfinite(one).all()
        assert torch.equal(one, twice), i  # two runs give the same bits
        assert torch.equal(one, by_launch), i


# ---- the range check ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['table', 'pair'])
def test_out_of_range_index_gives_nan_and_check_raises_once(form, monkeypatch):
    monkeypatch.setenv('TGMX_DECODER_FORM', form)
    model = link_model()
    z, src, dst, fixed, _ = (t.to(DEV) if isinstance(t, torch.Tensor) else t for t in eval_case(9))
    with torch.no_grad():
        good = model.query_one_vs_many(z, src, dst, fixed)
        model.check()  # nothing to report
        bad_neg = fixed.clone()
        bad_neg[2, 5], bad_neg[4, 0] = z.shape[0], -1
        got = model.query_one_vs_many(z, src, dst, bad_neg)
    mask = torch.zeros_like(good, dtype=torch.bool)
    mask[2, 6] = mask[4, 1] = True
    assert torch.isnan(got[mask]).all() and torch.equal(got[~mask], good[~mask])
    with pytest.raises(ValueError, match='outside'):
        model.check()
    model.check()  # reported once
    bad_src = src.clone()
    bad_src[3] = 10**6
    with torch.no_grad():
        got = model.query_one_vs_many(z, bad_src, dst, fixed)
        flat = model.score_pairs(z, bad_src, dst)
    assert torch.isnan(got[3]).all() and torch.equal(got[[0, 1, 2, 4, 5, 6, 7, 8]], good[[0, 1, 2, 4, 5, 6, 7, 8]])
    assert torch.isnan(flat[3]) and torch.equal(flat[:3], good[:3, 0])
    with pytest.raises(ValueError, match='outside'):
        model.check()


# ---- the torch paths ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('merge', ['concat', 'sum'])
def test_gradient_mode_takes_the_torch_path_and_matches_autograd(merge):
    model = link_model(merge=merge).train()
    g = torch.Generator().manual_seed(4)
    a, b = torch.randn(30, 24, generator=g).to(DEV).requires_grad_(), torch.randn(30, 24, generator=g).to(DEV).requires_grad_()
    out = model(a, b)
    assert out.requires_grad
    out.square().sum().backward()
    sd = {k: v.detach().clone().requires_grad_() for k, v in model.state_dict().items()}
    a2, b2 = a.detach().clone().requires_grad_(), b.detach().clone().requires_grad_()
    ref = dr.link(sd, merge, a2, b2, torch.float32)  # the reference's arithmetic, under autograd
    ref.square().sum().backward()
    dr.close(out.detach().cpu(), ref.detach().cpu(), 'forward')
    dr.close(a.grad.cpu(), a2.grad.cpu(), 'grad z_src')
    dr.close(b.grad.cpu(), b2.grad.cpu(), 'grad z_dst')
    for k, p in model.named_parameters():
        dr.close(p.grad.cpu(), sd[k].grad.cpu(), f'grad {k}')
    with torch.no_grad():
        native = model(a, b)
    dr.close(native.cpu(), ref.detach().cpu(), 'native against the torch path')
    z = torch.randn(12, 24, device=DEV, requires_grad=True)
    idx = torch.arange(12, device=DEV)
    assert model.score_pairs(z, idx, idx.flip(0)).requires_grad and model.query_one_vs_many(z, idx[:3], idx[3:6], idx[6:].view(3, 2)).requires_grad


def test_outside_the_envelope_falls_back_without_error():
    from tgm_amd.nn import GraphPredictor, LinkPredictor, NodePredictor

    g = torch.Generator().manual_seed(6)
    z = torch.randn(20, 24, generator=g)
    zd, idx = z.to(DEV), torch.arange(20, device=DEV)

    class Product:  # an Aggregator that is none of the four shipped
        out_channels = 24

        def __call__(self, a, b=None):
            return a * b if b is not None else a.max(dim=0).values

    with torch.no_grad():
        wide = link_model(H=600)  # hidden layer wider than the score kernel's half row: the pair form
        bar(wide.score_pairs(zd, idx, idx.flip(0)), dr.link(cpu_sd(wide), 'concat', z, z.flip(0)), dr.link(cpu_sd(wide), 'concat', z, z.flip(0), torch.float32), 'H=600')
        custom = LinkPredictor(24, merge_op=Product()).to(DEV).eval()  # the merge in torch, the MLP natively
        ref = dr.mlp({k: v.double() for k, v in cpu_sd(custom).items()}, (z * z.flip(0)).double()).reshape(-1)
        dr.close(custom(zd, zd.flip(0)).cpu(), ref.float(), 'custom merge')
        dr.close(custom.score_pairs(zd, idx, idx.flip(0)).cpu(), ref.float(), 'custom merge, score_pairs')
        pooled = GraphPredictor(24, 3, graph_pooling=Product()).to(DEV).eval()
        dr.close(pooled(zd).cpu(), dr.mlp({k: v.double() for k, v in cpu_sd(pooled).items()}, z.max(dim=0).values.double()).float(), 'custom pooling')
        strided = link_model()
        strided.model[0].weight = torch.nn.Parameter(strided.model[0].weight.detach().t().contiguous().t())  # not contiguous
        dr.close(strided(zd, zd.flip(0)).cpu(), dr.link(cpu_sd(strided), 'concat', z, z.flip(0)).float(), 'strided weight')
        double = NodePredictor(24, 2).to(DEV).double().eval()
        out = double(zd.double())
        assert out.dtype == torch.float64 and tuple(out.shape) == (20, 2)
        deep = NodePredictor(24, 2, nlayers=10).to(DEV).eval()  # nine Linears: more than the native head takes
        dr.close(deep(zd).cpu(), dr.node(cpu_sd(deep), z).float(), 'ten layers')
        assert tuple(NodePredictor(24, 2).to(DEV)(zd.view(4, 5, 24)).shape) == (4, 5, 2)


def test_graph_predictor_output_shape():
    from tgm_amd.nn import GraphPredictor

    z = torch.randn(9, 24, device=DEV)
    with torch.no_grad():
        for out_dim in (1, 4, 20):
            model = GraphPredictor(24, out_dim).to(DEV).eval()
            got = model(z)
            assert tuple(got.shape) == (out_dim,) == tuple(model.cpu()(z.cpu()).shape)  # what the reference's squeeze leaves
