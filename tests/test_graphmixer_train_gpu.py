"""GraphMixer's native training path on the device (``tgm_amd/nn/_graphmixer_train.py``, ``csrc/mixer_bwd.hip``).

The new kernels alone, through ctypes, against the float64 restatement of ``tests/graphmixer_bwd_restate.py``: outputs pre-filled with NaN
inside ``Buf`` allocations whose sentinel columns and tail must stay intact, every case launched twice and compared bit for bit, and the
assertion err / bound <= 1 with bound = chain * 2^-24 * magnitude (``pytest -rP`` prints the worst ratio).  The token kernel at K in
{1, 2, 5, 20} (K = 1 at expansion 0.5: no hidden unit), C in {1, 128, 129, 172} (one ragged chunk, one full, two with a ragged second), S in
{1, 7}, with and without dropout; the GELU' and tail kernels at 1, 63, 64, 65 rows.

End to end against float64 autograd through the restatement at the project's bar for gradients (each within 1e-4 of its largest entry), on
the first batch of a stream (every slot padded) and a later one; then bit equality with the no-grad forward, repeat runs, the py mode, the
dispatch, frozen parameters, call sharing across an optimizer step, dropout with the regenerated masks, and ``MLPMixer`` on its own.
"""
import copy
import functools

import pytest
import torch

import graphmixer_bwd_restate as br
import graphmixer_restate as gr
from oracle.tgat_bwd_ref import EPS
from test_graphmixer_gpu import CFG2, _composed_spy, sampled_batches
from test_tgat_bwd_blocks_gpu import Buf, _report, _same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-4
F64 = torch.float64
ODD = dict(time_dim=7, embed_dim=9, num_tokens=5, node_dim=3, edge_dim=13, num_layers=3, token_dim_expansion=1.3, channel_dim_expansion=2.1)


@pytest.fixture(autouse=True)
def _native_mode(monkeypatch):
    """Every test here is about the native path, whichever way the default points."""
    monkeypatch.setenv('TGMX_GRAPHMIXER_BWD', 'native')


def _lib():
    from tgm_amd import _native

    return _native.load(), _native


def up4(n):
    return (n + 3) // 4 * 4


# ---- the token kernel alone ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _token_case(K, C, S, ft, p):
    g = torch.Generator().manual_seed(1000 * K + 10 * C + S + int(10 * ft))
    Ht = int(ft * K)
    P = [torch.randn(s, generator=g) * 0.5 + o for s, o in (((K,), 1.0), ((K,), 0.0), ((Ht, K), 0.0), ((Ht,), 0.0), ((K, Ht), 0.0), ((K,), 0.0))]
    x, dz1 = torch.randn(S, K, C, generator=g) * 1.5, torch.randn(S, K, C, generator=g)
    m = br.layer_masks(p, 77, 192, 1, S, K, C, Ht, 1)
    want = br.token_backward([t.double() for t in P], x.double(), dz1.double(), m[0], m[1])
    return P, x, dz1, Ht, want


def _launch_token(K, C, S, ft, p, with_rows=True):
    lib, nat = _lib()
    P, x, dz1, Ht, _ = _token_case(K, C, S, ft, p)
    W, ldw = 4 * K + 2 * Ht, up4(4 * K + 2 * Ht)
    dP = [t.to(DEV).contiguous() for t in P]
    xb, db = Buf(S * K, C, ld=up4(C) + 4, data=x.view(S * K, C).to(DEV), fill=0.0), Buf(S * K, C, ld=C + 1, data=dz1.view(S * K, C).to(DEV), fill=0.0)
    dx, rows = Buf(S * K, C, ld=up4(C) + 8), Buf(S * C, ldw)
    nat.check(lib.tgmx_mixer_token_backward(xb.ptr, xb.ld, db.ptr, db.ld, S, K, C, dP[0].data_ptr(), dP[1].data_ptr(), nat.ptr(dP[2]) if Ht else None,
                                            nat.ptr(dP[3]) if Ht else None, Ht, nat.ptr(dP[4]) if Ht else None, 1e-5, dx.ptr, dx.ld,
                                            rows.ptr if with_rows else None, ldw, nat.dropout_desc(p, 77, 192 + 4), nat.dropout_desc(p, 77, 192 + 5),
                                            nat.stream_ptr()), 'tgmx_mixer_token_backward')  # fmt: skip
    torch.cuda.synchronize()
    return dx, rows, W


@pytest.mark.parametrize('C', [1, 128, 129, 172])
@pytest.mark.parametrize('K', [1, 2, 5, 20])
def test_token_backward_alone(K, C):
    worst = 0.0
    for S in (1, 7):
        for ft in (0.5, 1.3, 0.9):
            for p in (0.0, 0.5):
                _, _, _, Ht, want = _token_case(K, C, S, ft, p)
                chain = br.token_chain(K, Ht) * EPS
                runs = [_launch_token(K, C, S, ft, p) for _ in range(2)]
                (dx, rows, W), (dx2, rows2, _) = runs
                assert _same_bits(dx.flat, dx2.flat) and _same_bits(rows.flat, rows2.flat)
                assert dx.sentinels_intact() and rows.sentinels_intact()
                tag = f'token bwd K={K} C={C} S={S} Ht={Ht} p={p}'
                worst = max(worst, _report(tag + ' dx', dx.view, want['dx'].reshape(S * K, C), chain * want['dx_m'].reshape(S * K, C)))
                worst = max(worst, _report(tag + ' rows', rows.view[:, :W].contiguous(), want['rows'], chain * want['rows_m']))
                assert not rows.view[:, W:].any()  # the pad columns are written as zeros
                nr, _, _ = _launch_token(K, C, S, ft, p, with_rows=False)  # no parameter gradient wanted: the same dx
                assert _same_bits(nr.flat, dx.flat)
    assert worst <= 1.0


def test_token_backward_refuses_what_does_not_fit():
    lib, nat = _lib()
    z = torch.zeros(2 * 125 * 8, device=DEV)  # K = 125: 500 values a column, 66 000 bytes at 32 channels a pass
    rc = lib.tgmx_mixer_token_backward(z.data_ptr(), 8, z.data_ptr(), 8, 1, 125, 8, z.data_ptr(), z.data_ptr(), None, None, 0, None, 1e-5,
                                       z.data_ptr() + 4 * 1000, 8, None, 500, None, None, nat.stream_ptr())  # fmt: skip
    assert rc == nat.E_UNSUPPORTED and not lib.tgmx_mixer_train_supported(125, 1, 0) and lib.tgmx_mixer_train_supported(124, 1, 0)


# ---- GELU', the tail and the channel norm alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('C', [7, 130])
@pytest.mark.parametrize('R', [1, 63, 64, 65])
def test_gelu_backward_alone(R, C, p):
    lib, nat = _lib()
    g = torch.Generator().manual_seed(R * 131 + C)
    a, dh = torch.randn(R, C, generator=g) * 2.5, torch.randn(R, C, generator=g)
    m = br.layer_masks(p, 9, 64, 0, R, 1, 1, 1, C)[2]
    a64 = a.double()
    want_h, want_d = br.gelu(a64) * m, dh.double() * m * br.gelu_grad(a64)
    mag_h, mag_d = br.gelu_m(a64) * m, dh.double().abs() * m * br.gelu_grad_m(a64)
    outs = []
    for _ in range(2):
        ab, hb = Buf(R, C, ld=C + 3, data=a.to(DEV)), Buf(R, C, ld=up4(C) + 4, data=dh.to(DEV))
        nat.check(lib.tgmx_mixer_gelu_backward(ab.ptr, ab.ld, hb.ptr, hb.ld, R, C, nat.dropout_desc(p, 9, 64 + 2), nat.stream_ptr()), 'tgmx_mixer_gelu_backward')
        torch.cuda.synchronize()
        outs.append((ab, hb))
    assert all(_same_bits(u.flat, v.flat) and u.sentinels_intact() for u, v in zip(*outs))
    assert _report(f'gelu bwd R={R} C={C} p={p} hd', outs[0][0].view, want_h, br.gelu_chain() * EPS * mag_h) <= 1.0
    assert _report(f'gelu bwd R={R} C={C} p={p} da', outs[0][1].view, want_d, br.gelu_chain() * EPS * mag_d) <= 1.0


@pytest.mark.parametrize('C', [5, 130])
@pytest.mark.parametrize('S,K', [(1, 1), (9, 7), (8, 8), (13, 5)])
def test_tail_backward_alone(S, K, C):
    lib, nat = _lib()
    g = torch.Generator().manual_seed(S * 17 + K + C)
    nids = torch.randint(0, 50, (S, K), generator=g, dtype=torch.int32)
    nids[torch.rand(S, K, generator=g) < 0.4] = -1
    nids[0] = -1  # a seed with no valid slot
    nids[-1] = 3  # (for S = 1 the only seed: every slot valid)
    dcat = torch.randn(S, C, generator=g)
    want = br.tail_backward(dcat, nids, K)
    dnids = nids.to(DEV)
    outs = []
    for _ in range(2):
        cb, dz = Buf(S, C, ld=C + 2, data=dcat.to(DEV)), Buf(S * K, C, ld=up4(C) + 4)
        nat.check(lib.tgmx_mixer_tail_backward(cb.ptr, cb.ld, dnids.data_ptr(), S, K, C, dz.ptr, dz.ld, nat.stream_ptr()), 'tgmx_mixer_tail_backward')
        torch.cuda.synchronize()
        outs.append(dz)
    assert _same_bits(outs[0].flat, outs[1].flat) and outs[0].sentinels_intact()
    assert _report(f'tail bwd S={S} K={K} C={C}', outs[0].view, want, br.tail_chain() * EPS * want.abs()) <= 1.0
    if S > 1:
        assert not outs[0].view[:K].any()  # no valid slot: zeros


@pytest.mark.parametrize('C', [1, 129])
@pytest.mark.parametrize('R', [1, 63, 64, 65])
def test_channel_norm_alone(R, C):
    """y = LN_C(z1) again, within the forward's bar of float64."""
    lib, nat = _lib()
    g = torch.Generator().manual_seed(R + C)
    z1, cg, cb = torch.randn(R, C, generator=g) * 1.5, torch.randn(C, generator=g), torch.randn(C, generator=g)
    zb, y = Buf(R, C, ld=C + 1, data=z1.to(DEV)), Buf(R, C, ld=up4(C) + 4)
    dg, db = cg.to(DEV), cb.to(DEV)
    nat.check(lib.tgmx_mixer_channel_norm(zb.ptr, zb.ld, R, C, dg.data_ptr(), db.data_ptr(), 1e-5, y.ptr, y.ld, nat.stream_ptr()),
              'tgmx_mixer_channel_norm')  # fmt: skip
    torch.cuda.synchronize()
    want = torch.nn.functional.layer_norm(z1.double(), (C,), cg.double(), cb.double(), 1e-5)
    assert y.sentinels_intact() and gr.rel_err(y.view, want) < BAR


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batches(key):
    dims, E, bs = {'odd': (ODD, 1200, 100), 'cfg2': (CFG2, 200, 10), 'flat': ({**ODD, 'num_layers': 0}, 1200, 100), 'wide': (dict(CFG2, num_tokens=64), 200, 10)}[key]
    torch.manual_seed(3)
    _, batches = sampled_batches(dims, E=E, bs=bs)
    return dims, batches, torch.randn(400, dims['node_dim'], device=DEV)


def _encoder(key, dropout=0.0, seed=0):
    from tgm_amd.nn import GraphMixerEncoder

    dims, batches, node_feat = _batches(key)
    torch.manual_seed(seed)
    enc = GraphMixerEncoder(**dims, dropout=dropout).to(DEV).train()
    with torch.no_grad():
        for p in enc.parameters():
            if p.requires_grad:
                p.add_(0.1 * torch.randn_like(p))
    return enc, batches, node_feat


def _weight(S, E, seed=7):
    return torch.randn(S, E, generator=torch.Generator().manual_seed(seed))


def _device(enc, b, node_feat, w):
    """One forward and backward on the device: (out, name -> gradient or None)."""
    enc.zero_grad(set_to_none=True)
    out = enc(b, node_feat)
    (out * w.to(DEV)).sum().backward()
    return out.detach(), {k: (None if p.grad is None else p.grad.clone()) for k, p in enc.named_parameters() if not k.startswith('time_encoder')}


def _host_args(b, node_feat):
    return dict(nbr_edge_x=b.nbr_edge_x[0].cpu(), seed_times=b.seed_times[0].cpu(), nbr_edge_time=b.nbr_edge_time[0].cpu(), nbr_nids=b.nbr_nids[0].cpu(),
                seeds=torch.cat([b.edge_src, b.edge_dst, b.neg]).cpu(), tg_lists=gr.hook_lists(b.time_gap_nbr, b.time_gap_lo, b.time_gap_cnt),
                node_feat=node_feat.cpu())  # fmt: skip


def _reference(enc, b, node_feat, w, masks=None):
    """(out, name -> gradient, name -> magnitude): float64 autograd through the restatement, and the restated backward's magnitudes."""
    sd = {k: v.detach().cpu().double() for k, v in enc.state_dict().items()}
    leaf = {k: v.clone().requires_grad_(not k.startswith('time_encoder')) for k, v in sd.items()}
    args = _host_args(b, node_feat)
    if masks is None:
        out = gr.encoder_forward(leaf, enc.num_layers, args['nbr_edge_x'], args['seed_times'], args['nbr_edge_time'], args['nbr_nids'], args['seeds'],
                                 args['tg_lists'], args['node_feat'])  # fmt: skip
    else:
        out = br.encoder_forward(leaf, enc.num_layers, masks=masks, **args)
    (out * w.double()).sum().backward()
    keep = {}
    br.encoder_forward(sd, enc.num_layers, masks=masks, keep=keep, **args)
    mags = {k: m for k, (_, m) in br.encoder_backward(sd, enc.num_layers, keep, w, masks).items()}
    return out.detach(), {k: leaf[k].grad for k in mags}, mags


def _check_bar(label, got, ref, mags):
    """Every gradient within BAR of its largest entry.  A gradient that is exactly 0 (the first batch: every slot padded, so nothing flows
    below the output layer) has no such scale: where the reference's largest entry is below 1e-12 of the restated magnitude's, that
    magnitude is the scale, and where the magnitude is 0 too the gradient must be exactly 0."""
    worst = 0.0
    for name, r in ref.items():
        g = got[name]
        assert g is not None and g.dtype == torch.float32 and torch.isfinite(g).all(), (label, name)
        r = torch.zeros(g.shape, dtype=F64) if r is None else r
        if r.numel() == 0:
            assert g.shape == r.shape
            continue
        scale, m = r.abs().max().item(), mags[name].max().item()
        if scale <= 1e-12 * m:
            scale = m
        dist = (g.cpu().double() - r).abs().max().item()
        if scale == 0.0:
            assert dist == 0.0, (label, name, dist)
            continue
        print(f'graphmixer train {label} {name}: {dist / scale:.3e}')
        worst = max(worst, dist / scale)
        assert dist / scale <= BAR, (label, name, dist / scale)
    print(f'graphmixer train {label}: worst ratio {worst:.3e}')
    return worst


@pytest.mark.parametrize('which', ['first', 'later'])
@pytest.mark.parametrize('key', ['odd', 'cfg2', 'flat'])
def test_gradients_match_float64_autograd(key, which):
    enc, batches, node_feat = _encoder(key)
    b = batches[0] if which == 'first' else batches[len(batches) // 2]
    pads = int((b.nbr_nids[0] == -1).sum())
    assert (pads == b.nbr_nids[0].numel()) if which == 'first' else (pads < b.nbr_nids[0].numel())
    w = _weight(3 * b.edge_src.numel(), enc.embed_dim)
    out, got = _device(enc, b, node_feat, w)
    assert 'GraphMixerFunction' in type(enc(b, node_feat).grad_fn).__name__
    zr, ref, mags = _reference(enc, b, node_feat, w)
    assert gr.rel_err(out, zr) < BAR and sorted(got) == sorted(ref)
    _check_bar(f'{key} {which}', got, ref, mags)


def _equal_grads(a, b, skip=()):
    for name in a:
        if name.startswith(tuple(skip)) and skip:
            continue
        assert (a[name] is None) == (b[name] is None), name
        assert a[name] is None or _same_bits(a[name], b[name]), name


@pytest.mark.parametrize('key', ['odd', 'cfg2', 'flat'])
def test_forward_bits_repeat_runs_and_py_mode(key, monkeypatch):
    monkeypatch.setenv('TGMX_GRAPHMIXER_BWD', 'native')
    enc, batches, node_feat = _encoder(key)
    for b in (batches[0], batches[-2]):
        w = _weight(3 * b.edge_src.numel(), enc.embed_dim)
        with torch.no_grad():
            plain = enc(b, node_feat)
        out, ga = _device(enc, b, node_feat, w)
        assert _same_bits(out, plain)  # the grad-enabled forward is the inference call
        _, ga2 = _device(enc, b, node_feat, w)
        _equal_grads(ga, ga2)
        monkeypatch.setenv('TGMX_GRAPHMIXER_BWD', 'py')
        out_py, gpy = _device(enc, b, node_feat, w)
        monkeypatch.setenv('TGMX_GRAPHMIXER_BWD', 'native')
        assert _same_bits(out_py, plain)
        _equal_grads(ga, gpy)
    enc.eval()  # eval mode under gradients: the same
    out_eval, ge = _device(enc, b, node_feat, w)
    assert _same_bits(out_eval, plain)
    _equal_grads(ga, ge)


def test_dispatch(monkeypatch):
    """Inside the envelope ``_torch_forward`` is not called and ``backward()`` is one ``tgmx_graphmixer_backward``; every way out of the
    envelope composes, and returns gradients."""
    lib, _ = _lib()
    from tgm_amd.nn import _graphmixer_train as gt

    monkeypatch.delenv('TGMX_GRAPHMIXER_BWD')  # the default, pinned to native for this test

    monkeypatch.setattr(gt, 'DEFAULT', 'native')
    calls, orig = [], lib.tgmx_graphmixer_backward
    monkeypatch.setattr(lib, 'tgmx_graphmixer_backward', lambda *a: calls.append(1) or orig(*a))
    enc, batches, node_feat = _encoder('odd')
    b = batches[5]
    w = _weight(3 * b.edge_src.numel(), enc.embed_dim)
    took = []
    _composed_spy(monkeypatch, enc, took)
    _, native = _device(enc, b, node_feat, w)
    assert took == [] and calls == [1]

    def composed(**kw):
        took.clear()
        nf = kw.get('node_feat', node_feat)
        bb = kw.get('batch', b)
        enc.zero_grad(set_to_none=True)
        out = enc(bb, nf)
        assert took == ['composed'] and out.requires_grad
        (out.float() * w.to(DEV)).sum().backward()
        assert enc.output_layer.weight.grad is not None and calls == [1]

    composed(node_feat=node_feat.clone().requires_grad_(True))
    b_grad = copy.copy(b)
    b_grad.nbr_edge_x = [b.nbr_edge_x[0].clone().requires_grad_(True)]
    composed(batch=b_grad)
    monkeypatch.setenv('TGMX_GRAPHMIXER_BWD', 'torch')
    composed()
    monkeypatch.delenv('TGMX_GRAPHMIXER_BWD')
    enc.time_encoder.w.weight.requires_grad_(True)
    composed()
    enc.time_encoder.w.weight.requires_grad_(False)
    enc.time_encoder.w.weight.grad = None
    took.clear()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        try:
            enc(b, node_feat)
        except RuntimeError:  # (what the composed path makes of autocast is its own business, unchanged here)
            pass
    assert took == ['composed']
    _, again = _device(enc, b, node_feat, w)  # the module is intact after the composed calls
    assert calls == [1, 1]
    _equal_grads(native, again)
    monkeypatch.setenv('TGMX_GRAPHMIXER_BWD', 'py')
    _, py = _device(enc, b, node_feat, w)
    assert calls == [1, 1]
    _equal_grads(native, py)


def test_training_outside_the_lds_envelope_composes(monkeypatch):
    """K = 64 at D = 172: neither token kernel holds the tile; training composes, without error and without a warning about inference."""
    enc, batches, node_feat = _encoder('wide')
    b = batches[-2]
    took = []
    _composed_spy(monkeypatch, enc, took)
    out = enc(b, node_feat)
    assert took == ['composed'] and 'GraphMixerFunction' not in type(out.grad_fn).__name__
    out.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in enc.parameters() if p.requires_grad)


def test_needs_input_grad_is_honoured():
    enc, batches, node_feat = _encoder('odd')
    b = batches[6]
    w = _weight(3 * b.edge_src.numel(), enc.embed_dim)
    _, full = _device(enc, b, node_feat, w)
    for frozen in ('output_layer', 'mlp_mixers.1', 'mlp_mixers.0', 'projection_layer'):
        for n, p in enc.named_parameters():
            p.requires_grad_(not n.startswith(('time_encoder', frozen)))
        _, part = _device(enc, b, node_feat, w)
        assert all((part[k] is None) == k.startswith(frozen) for k in part), frozen
        _equal_grads(full, part, skip=(frozen,))
    # only the output layer trains: the chain below it is skipped altogether
    for n, p in enc.named_parameters():
        p.requires_grad_(n.startswith('output_layer'))
    _, top = _device(enc, b, node_feat, w)
    assert all((top[k] is None) != k.startswith('output_layer') for k in top)
    _equal_grads({k: v for k, v in full.items() if k.startswith('output_layer')}, {k: v for k, v in top.items() if k.startswith('output_layer')})


def test_call_sharing_across_an_optimizer_step():
    """Forward A, SGD step, forward B, backward B, backward A: A's gradients are those of the run without B in between -- and those of
    A's own weights (forward A, backward A), because the call keeps the weights it ran with."""
    enc0, batches, node_feat = _encoder('odd')
    bA, bB = batches[4], batches[7]
    wA, wB = _weight(3 * bA.edge_src.numel(), enc0.embed_dim).to(DEV), _weight(3 * bB.edge_src.numel(), enc0.embed_dim, seed=8).to(DEV)

    def run(with_b, step=True):
        enc = copy.deepcopy(enc0)
        params = [p for p in enc.parameters() if p.requires_grad]
        opt = torch.optim.SGD(params, lr=0.05)
        for p in params:
            p.grad = torch.full_like(p, 0.3)
        out_a = enc(bA, node_feat)
        if step:
            opt.step()
        if with_b:
            out_b = enc(bB, node_feat)
            torch.autograd.grad((out_b * wB).sum(), params)
        return torch.autograd.grad((out_a * wA).sum(), params)

    with_b, without_b, own = run(True), run(False), run(False, step=False)
    for x, y, z in zip(with_b, without_b, own):
        assert _same_bits(x, y) and _same_bits(x, z)


# ---- dropout ----------------------------------------------------------------------------------------------------------------------------------------
def _masks_of(enc, S):
    """The masks of the forward call the module has just made."""
    first = enc.__dict__['_tgmx_drop_calls'] * 64
    m = enc.mlp_mixers[0] if enc.num_layers else None
    return [br.layer_masks(enc.dropout, torch.initial_seed(), first, l, S, enc.num_tokens, enc.edge_dim, m.token_feedforward.ffn[0].out_features,
                           m.channel_feedforward.ffn[0].out_features) for l in range(enc.num_layers)]  # fmt: skip


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('key', ['odd', 'cfg2'])
def test_dropout_matches_the_restatement_with_the_regenerated_masks(key, p, monkeypatch):
    monkeypatch.setenv('TGMX_GRAPHMIXER_BWD', 'native')
    enc, batches, node_feat = _encoder(key, dropout=p)
    b = batches[len(batches) // 2]
    S = 3 * b.edge_src.numel()
    w = _weight(S, enc.embed_dim)
    took = []
    _composed_spy(monkeypatch, enc, took)
    out, got = _device(enc, b, node_feat, w)
    assert took == []
    masks = _masks_of(enc, S)
    zr, ref, mags = _reference(enc, b, node_feat, w, masks)
    assert gr.rel_err(out, zr) < BAR
    _check_bar(f'{key} p={p}', got, ref, mags)
    out2, _ = _device(enc, b, node_feat, w)
    assert not torch.equal(out, out2)  # a fresh stream per forward call
    monkeypatch.setenv('TGMX_GRAPHMIXER_BWD', 'py')
    out3, gpy = _device(enc, b, node_feat, w)
    zr3, ref3, mags3 = _reference(enc, b, node_feat, w, _masks_of(enc, S))
    assert gr.rel_err(out3, zr3) < BAR
    _check_bar(f'{key} p={p} py', gpy, ref3, mags3)


def test_train_mode_without_dropout_and_eval_mode_give_the_inference_bits():
    enc, batches, node_feat = _encoder('odd', dropout=0.0)
    b = batches[3]
    with torch.no_grad():
        plain = enc(b, node_feat)
    assert _same_bits(enc(b, node_feat).detach(), plain)
    enc2, _, _ = _encoder('odd', dropout=0.3)
    enc2.eval()
    with torch.no_grad():
        plain2 = enc2(b, node_feat)
    out = enc2(b, node_feat)
    assert out.requires_grad and _same_bits(out.detach(), plain2)


# ---- MLPMixer alone -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('K,C', [(5, 13), (20, 172)])
def test_mlp_mixer_alone(K, C, p, monkeypatch):
    from tgm_amd.nn import MLPMixer

    monkeypatch.setenv('TGMX_GRAPHMIXER_BWD', 'native')
    torch.manual_seed(K + C)
    m = MLPMixer(K, C, 1.3 if K == 5 else 0.5, 2.1 if K == 5 else 4.0, dropout=p).to(DEV).train()
    with torch.no_grad():
        for q in m.parameters():
            q.add_(0.1 * torch.randn_like(q))
    B = 7
    x = (torch.randn(B, K, C, device=DEV) * 1.5).requires_grad_(True)
    w = torch.randn(B, K, C, generator=torch.Generator().manual_seed(1))
    took = []
    _composed_spy(monkeypatch, m, took)
    out = m(x)
    assert took == [] and 'MixerFunction' in type(out.grad_fn).__name__
    (out * w.to(DEV)).sum().backward()
    Ht, Hc = m.token_feedforward.ffn[0].out_features, m.channel_feedforward.ffn[0].out_features
    masks = br.layer_masks(p, torch.initial_seed(), m.__dict__['_tgmx_drop_calls'] * 64, 0, B, K, C, Ht, Hc) if p else br.unit_masks(B, K, C, Ht, Hc)
    P = [q.detach().cpu().double().requires_grad_(True) for q in (m.get_parameter(n) for n in br.LAYER_NAMES)]
    xr = x.detach().cpu().double().requires_grad_(True)
    keep = {}
    zr = br.mixer_forward(P, xr, masks, keep=keep)
    if not p:
        sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
        assert gr.rel_err(zr, gr.mixer_forward(sd, '', xr.detach())) < 1e-12
        with torch.no_grad():
            assert _same_bits(out.detach(), m(x))  # the inference bits
    (zr * w.double()).sum().backward()
    assert gr.rel_err(out, zr) < BAR
    r = br.mixer_backward([q.detach() for q in P], xr.detach(), keep['z1'], w.double(), masks)
    got = {n: m.get_parameter(n).grad for n in br.LAYER_NAMES}
    got['dx'] = x.grad
    ref = {n: q.grad for n, q in zip(br.LAYER_NAMES, P)}
    ref['dx'] = xr.grad
    _check_bar(f'mixer K={K} C={C} p={p}', got, ref, {n: r[n + '_m'] for n in ref})
    # an input that asks for nothing, and frozen parameters with an input that does
    for q in m.parameters():
        q.grad = None
    if not p:
        (m(x.detach()) * w.to(DEV)).sum().backward()
        for n in br.LAYER_NAMES:
            assert _same_bits(m.get_parameter(n).grad, got[n]), n
        for q in m.parameters():
            q.requires_grad_(False)
            q.grad = None
        m.token_norm.bias.requires_grad_(True)
        x2 = x.detach().clone().requires_grad_(True)
        (m(x2) * w.to(DEV)).sum().backward()
        assert _same_bits(x2.grad, got['dx']) and m.channel_norm.weight.grad is None
