"""The four entry points of ``csrc/tgn_bwd.hip`` one by one against the float64 restatements of ``oracle/tgn_bwd_ref.py`` (which
``tests/test_tgn_bwd_ref_cpu.py`` pins to autograd), through ctypes: ``tgmx_tgn_gru_gate_backward``,
``tgmx_tgn_aggregate_backward``, ``tgmx_tconv_edge_attr_backward``, ``tgmx_tconv_attend_backward``; and the empty branches of their
wrappers in ``tgm_amd/nn/_tgn_train.py``.  The conventions are those of ``tests/test_tgat_bwd_blocks_gpu.py`` (whose helpers are
imported):

* outputs are pre-filled with NaN (dk / dv with zeros, as the header requires) and followed by a sentinel tail of 4096 floats that
  must be unchanged; input columns a kernel has no business reading (the non-time columns of d_aggr, the message columns of
  d_attr) hold NaN;
* every case is launched twice: equal bits everywhere except dk / dv (float atomics have no fixed order), which meet the bound
  both times;
* bars: elementwise ``n * 2^-24 * magnitude`` with n counted from the kernel code (``gru_chain``, ``aggregate_chain``,
  ``edge_attr_chain``, ``attend_chain``), nothing tuned on the device's result; the structural zeros are exact.
  ``pytest -rP`` prints the worst err / bound per case.

Measured on an MI355X, worst err / bound over the cases of each kernel: gru_gate_backward 0.092 (dgi 0.074, dgh 0.092, both at
(41944, 100)); aggregate_backward 0.149 (LAST, T = 64); edge_attr_backward 0.189 (at (41944, 100, 0)); attend_backward dq 0.0018,
dk 0.0015, dv 0.0043, de 0.284 (de at (2, 64, 0.5): an edge whose weight sits at float32's underflow threshold; 0.005 elsewhere).
The attention's bound is a worst case over chains of up to ~1300 operations (the 300-edge target, the 300-fold source row) with
first-order sensitivities for the softmax: the device's error, a random walk over tree-shaped sums, stays far below it; what the
bound still catches is listed in ``oracle.tgn_bwd_ref.MUTATIONS``.  The end-to-end case without edges and messages: 1.5e-7.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import tgn_bwd_ref as ref
from test_tgat_bwd_blocks_gpu import DEV, Buf, _lib, _report, _same_bits

pytestmark = pytest.mark.gpu

gru_case = functools.lru_cache(maxsize=None)(ref.gru_case)
aggr_case = functools.lru_cache(maxsize=None)(ref.aggr_case)
edge_case = functools.lru_cache(maxsize=None)(ref.edge_case)
attend_case = functools.lru_cache(maxsize=None)(ref.attend_case)
gru_bounds = functools.lru_cache(maxsize=None)(lambda R, M: ref.gru_bounds(gru_case(R, M)))
aggr_bounds = functools.lru_cache(maxsize=None)(lambda mean, T, M, D: ref.aggr_bounds(aggr_case(T, M, D), mean))
edge_bounds = functools.lru_cache(maxsize=None)(lambda E, T, D: ref.edge_bounds(edge_case(E, T, D)))
attend_bounds = functools.lru_cache(maxsize=None)(lambda H, C, p: ref.attend_bounds(attend_case(H, C, p)))


def _dev(t):
    return t.to(DEV).contiguous()


def _untouched(*bufs):
    return all(bool(torch.isnan(b.flat).all()) for b in bufs)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tgn_gru_gate_backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R,M', ref.GRU_CASES + [ref.GRU_BIG_CASE])
def test_gru_gate_backward(R, M):
    """(1,1), (3,5), (7,100): one thread, a ragged block, several blocks.  (41944,100): 96 elements past 16384 blocks x 256 -- the
    block cap holds and the grid stride takes a second trip for exactly the tail.  Rows (oracle.tgn_bwd_ref.gru_case): the band
    with pre-activations +-30 and +-95 (expf overflows, the sigmoid derivative is 0, tanh saturates: finite outputs, and the bound
    gets the floor 2^-126 * A * (A + 1) of gru_underflow_floor there), and the row with h == n (the cancellation in dz)."""
    lib, native = _lib()
    c = gru_case(R, M)
    (dgi, dgh), (bi, bh) = gru_bounds(R, M)
    gi, gh, h, dout = (_dev(c[n]) for n in ('gi', 'gh', 'h', 'dout'))
    outs = []
    for _ in range(2):
        bGi, bGh = Buf(R, 3 * M), Buf(R, 3 * M)
        native.check(lib.tgmx_tgn_gru_gate_backward(gi.data_ptr(), gh.data_ptr(), h.data_ptr(), dout.data_ptr(), M, R, bGi.ptr, bGh.ptr,
                                                    native.stream_ptr()), 'gru_gate_backward')
        torch.cuda.synchronize()
        assert bGi.sentinels_intact() and bGh.sentinels_intact(), 'a write past [R, 3M]'
        outs.append((bGi.view.clone(), bGh.view.clone()))
    assert _same_bits(outs[0][0], outs[1][0]) and _same_bits(outs[0][1], outs[1][1]), 'two launches differ'
    assert _report(f'gru_gate_backward {(R, M)} dgi', outs[0][0], dgi, bi) <= 1.0
    assert _report(f'gru_gate_backward {(R, M)} dgh', outs[0][1], dgh, bh) <= 1.0
    # the r and z gates' gradients are the same numbers in dgi and dgh
    assert _same_bits(outs[0][0][:, :2 * M], outs[0][1][:, :2 * M])


def test_gru_gate_backward_no_rows():
    lib, native = _lib()
    bGi, bGh = Buf(0, 3), Buf(0, 3)
    native.check(lib.tgmx_tgn_gru_gate_backward(None, None, None, None, 1, 0, bGi.ptr, bGh.ptr, native.stream_ptr()), 'gru_gate_backward R = 0')
    torch.cuda.synchronize()
    assert _untouched(bGi, bGh)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tgn_aggregate_backward
# ---------------------------------------------------------------------------------------------------------------------------
def _aggregate(c, mean, R=None):
    lib, native = _lib()
    R = c['R'] if R is None else R
    T = c['T']
    d = {n: _dev(c[n]) for n in ('lo_s', 'cnt_s', 'lo_d', 'cnt_d', 'lu', 'log_t', 'tw', 'tb', 'd_aggr')}
    assert d['cnt_s'].dtype == torch.int32 and d['lo_s'].dtype == torch.int64
    part = Buf(R, 2 * T)
    native.check(lib.tgmx_tgn_aggregate_backward(R, d['lo_s'].data_ptr(), d['cnt_s'].data_ptr(), d['lo_d'].data_ptr(), d['cnt_d'].data_ptr(),
                                                 d['lu'].data_ptr(), d['log_t'].data_ptr(), c['M'], c['D'], d['tw'].data_ptr(), d['tb'].data_ptr(), T,
                                                 mean, d['d_aggr'].data_ptr(), part.ptr, native.stream_ptr()), 'aggregate_backward')
    torch.cuda.synchronize()
    return part


@pytest.mark.parametrize('mean,T,M,D', ref.AGGR_CASES)
def test_aggregate_backward(mean, T, M, D):
    """One wave per row, four rows per block, R = 23 (the last block is ragged and ends on an empty row).  T = 1, 64, 65, 100: one
    lane, every lane once, a second column trip of one lane, of 36.  (M, D) = (1, 0) | (100, 172): the time columns start at 2 | 372
    of d_aggr, everything before them is NaN.  Rows (oracle.tgn_bwd_ref.aggr_case): empty, single, one window only (either),
    the destination window below the source window, totals of 64 / 65 / 130 (the lane-strided scan's second and third trip), the
    maximum at walk index 0 / 129 / 127, float32 ties between distinct unix-scale times within one lane's two trips, across
    lanes, across the two windows (first in walk order wins), dt == 0 (the tw part exactly 0), dt up to 2^31 - 1."""
    c = aggr_case(T, M, D)
    want, bound = aggr_bounds(mean, T, M, D)
    a, b = _aggregate(c, mean), _aggregate(c, mean)
    assert a.sentinels_intact() and b.sentinels_intact(), 'a write past [R, 2T]'
    assert _same_bits(a.view, b.view), 'two launches differ'
    got = a.view.cpu()
    empty = (c['cnt_s'] + c['cnt_d']) == 0
    assert int(empty.sum()) >= 2 and torch.equal(got[empty], torch.zeros(int(empty.sum()), 2 * T)), 'rows without events: exact zeros'
    assert torch.equal(got[ref.AGGR_ROW['dt_zero'], :T], torch.zeros(T)), 'dt == 0: the tw contribution is exactly 0'
    assert _report(f'aggregate_backward mean={mean} T={T} M={M} D={D}', got, want, bound) <= 1.0


def test_aggregate_backward_no_rows():
    lib, native = _lib()
    part = Buf(0, 16)
    native.check(lib.tgmx_tgn_aggregate_backward(0, None, None, None, None, None, None, 1, 0, None, None, 8, 0, None, part.ptr, native.stream_ptr()),
                 'aggregate_backward R = 0')
    torch.cuda.synchronize()
    assert _untouched(part)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tconv_edge_attr_backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E,T,D', ref.EDGE_CASES + [ref.EDGE_BIG_CASE])
def test_edge_attr_backward(E, T, D):
    """(1,1,0), (5,8,3), (37,100,172): one thread, one ragged block, several blocks with a row stride T + D of d_attr whose message
    columns are NaN.  (41944,100,0): E * T is 96 past 16384 blocks x 256 (the cap and the grid stride's second trip).  lu and t
    are near 1.7e9 with differences within +-40 (subtract in int64, THEN round: float first is off by up to 128), and 0, 2^31 - 3,
    -(2^31 - 7)."""
    lib, native = _lib()
    c = edge_case(E, T, D)
    want, bound = edge_bounds(E, T, D)
    d = {n: _dev(c[n]) for n in ('lu_local', 'src', 't', 'tw', 'tb', 'd_attr')}
    outs = []
    for _ in range(2):
        part = Buf(E, 2 * T)
        native.check(lib.tgmx_tconv_edge_attr_backward(d['lu_local'].data_ptr(), d['src'].data_ptr(), d['t'].data_ptr(), d['tw'].data_ptr(),
                                                       d['tb'].data_ptr(), d['d_attr'].data_ptr(), T, D, E, part.ptr, native.stream_ptr()),
                     'edge_attr_backward')
        torch.cuda.synchronize()
        assert part.sentinels_intact(), 'a write past [E, 2T]'
        outs.append(part.view.clone())
    assert _same_bits(outs[0], outs[1]), 'two launches differ'
    got = outs[0].cpu()
    if E >= 5:
        assert torch.equal(got[0, :T], torch.zeros(T)), 'dt == 0: the tw contribution is exactly 0'
    assert _report(f'edge_attr_backward {(E, T, D)}', got, want, bound) <= 1.0


def test_edge_attr_backward_no_edges():
    lib, native = _lib()
    part = Buf(0, 16)
    native.check(lib.tgmx_tconv_edge_attr_backward(None, None, None, None, None, None, 8, 3, 0, part.ptr, native.stream_ptr()), 'edge_attr_backward E = 0')
    torch.cuda.synchronize()
    assert _untouched(part)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tconv_attend_backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,C,p', ref.ATTEND_CASES)
def test_attend_backward(H, C, p):
    """(H, C, p): C = 1, 8, 33, 64 (``lane < C``: one lane, a few, past a half wave, all), H = 1, 2, 3, p = 0, 0.1, 0.5.  One wave per
    target, U = 11 in three blocks of four.  Targets (oracle.tgn_bwd_ref.attend_case) have 0, 1, 2, 64, 65, 300, 12, 0, 5, 3, 0
    incoming edges through a non-identity ``order``; one edge: ds cancels to within the bound; source 7 feeds target 5 300 times and
    three more targets (a long atomic chain into one dk / dv row); a self loop; target 6's scores spread by 120 (expf underflows to
    0 for its weak edges: their de is exactly 0); p = 0.5: target 1's only edge is dropped in head 0."""
    lib, native = _lib()
    c = attend_case(H, C, p)
    want, bound = attend_bounds(H, C, p)
    U, E, HC = c['U'], c['E'], H * C
    d = {n: _dev(c[n]) for n in ('q', 'k', 'v', 'eproj', 'order', 'src', 'seg_lo', 'seg_hi', 'dout')}
    outs = []
    for _ in range(2):
        bQ, bE = Buf(U, HC), Buf(E, HC)
        bK, bV = Buf(U, HC, data=torch.zeros(U, HC)), Buf(U, HC, data=torch.zeros(U, HC))
        native.check(lib.tgmx_tconv_attend_backward(d['q'].data_ptr(), d['k'].data_ptr(), d['v'].data_ptr(), d['eproj'].data_ptr(), d['order'].data_ptr(),
                                                    d['src'].data_ptr(), d['seg_lo'].data_ptr(), d['seg_hi'].data_ptr(), U, H, C, c['scale'],
                                                    d['dout'].data_ptr(), bQ.ptr, bK.ptr, bV.ptr, bE.ptr, native.dropout_desc(p, ref.DROP_SEED, c['stream']),
                                                    native.stream_ptr()), 'attend_backward')
        torch.cuda.synchronize()
        for name, b in (('dq', bQ), ('dk', bK), ('dv', bV), ('de', bE)):
            assert b.sentinels_intact(), f'{name}: a write past its last row'
        outs.append(dict(dq=bQ.view.clone(), dk=bK.view.clone(), dv=bV.view.clone(), de=bE.view.clone()))
    assert _same_bits(outs[0]['dq'], outs[1]['dq']) and _same_bits(outs[0]['de'], outs[1]['de']), 'two launches differ (dq / de)'
    none = c['seg_hi'] == c['seg_lo']
    assert torch.equal(outs[0]['dq'].cpu()[none], torch.zeros(int(none.sum()), HC)), 'a target without edges: dq must be exactly 0'
    worst = {}
    for name in ('dq', 'de', 'dk', 'dv'):
        for launch in ((0, 1) if name in ('dk', 'dv') else (0,)):
            worst[name, launch] = _report(f'attend_backward {(H, C, p)} {name} launch {launch}', outs[launch][name], want[name], bound[name])
    assert max(worst.values()) <= 1.0, worst
    # the spread target's weakest edge: alpha underflowed to exactly 0, and with it ds and de
    sp = (c['tgt'] == ref.ATTEND_SPREAD_TARGET).nonzero()[:, 0]
    weakest = sp[torch.argmin(c['eproj'][sp, 0])]
    assert torch.equal(outs[0]['de'].cpu()[weakest], torch.zeros(HC))


def test_attend_backward_no_targets():
    lib, native = _lib()
    outs = [Buf(0, 8) for _ in range(4)]
    native.check(lib.tgmx_tconv_attend_backward(None, None, None, None, None, None, None, None, 0, 2, 4, 0.5, None, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                                outs[3].ptr, None, native.stream_ptr()), 'attend_backward U = 0')
    torch.cuda.synchronize()
    assert _untouched(*outs)


# ---------------------------------------------------------------------------------------------------------------------------
# the empty branches of the wrappers (tgm_amd/nn/_tgn_train.py)
# ---------------------------------------------------------------------------------------------------------------------------
def _is_zero_like(grad, param):
    return grad is not None and grad.shape == param.shape and grad.dtype == param.dtype and grad.device == param.device and not bool(grad.any())


@pytest.mark.parametrize('bias', [True, False])
def test_linear_fn_without_rows(bias):
    from tgm_amd.nn._tgn_train import LinearFn

    x = torch.zeros(0, 5, device=DEV, requires_grad=True)
    w = torch.randn(3, 5, device=DEV, requires_grad=True)
    b = torch.randn(3, device=DEV, requires_grad=True) if bias else None
    y = LinearFn.apply(x, w, b)
    assert y.shape == (0, 3)
    y.sum().backward()
    assert _is_zero_like(x.grad, x) and _is_zero_like(w.grad, w) and (b is None or _is_zero_like(b.grad, b))


def test_edge_attr_fn_without_edges():
    from tgm_amd.nn._tgn_train import EdgeAttrFn

    T, D = 8, 3
    tw, tb = torch.randn(T, 1, device=DEV, requires_grad=True), torch.randn(T, device=DEV, requires_grad=True)
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=DEV)
    out = EdgeAttrFn.apply(tw, tb, i64(4), i64(0), i64(0), torch.zeros(0, D, device=DEV))
    assert out.shape == (0, T + D)
    out.sum().backward()
    assert _is_zero_like(tw.grad, tw) and _is_zero_like(tb.grad, tb)


def test_aggregate_fn_without_rows():
    from tgm_amd.nn import IdentityMessage, LastAggregator, TGNMemory
    from tgm_amd.nn._tgn_train import AggregateFn

    N, D, M, T = 10, 3, 4, 8
    mem = TGNMemory(N, D, M, T, IdentityMessage(D, M, T), LastAggregator()).to(DEV).train()
    mem.reset_state()  # allocates the message store's windows (forward() does it on its first call)
    tw, tb = mem.time_enc.w.weight, mem.time_enc.w.bias
    aggr, new_lu = AggregateFn.apply(tw, tb, mem, torch.zeros(0, dtype=torch.int32, device=DEV), None, 0)
    assert aggr.shape == (0, 2 * M + D + T) and new_lu.shape == (0,)
    aggr.sum().backward()
    assert _is_zero_like(tw.grad, tw) and _is_zero_like(tb.grad, tb)


@pytest.mark.parametrize('aggr', ['last', 'mean'])
def test_tgn_gradients_without_edges_and_without_messages(aggr):
    """The setup of tests/test_tgn_backward_gpu.py with E = 0 and an n_id of nodes that hold no messages: every aggregation row
    takes the kernel's ``total == 0`` branch, TransformerConv returns its skip path.  Bar: that file's, 2e-4 of each gradient's
    maximum (floored at 2e-3) against autograd through the oracle; a parameter nothing reaches has no gradient or a zero one on
    both sides."""
    from oracle.tgn_ref import graph_attention_embedding_ref
    from test_tgn_backward_gpu import _setup

    mem, enc, oracle, mp, ep, batches, rng, (N, D, M, T_) = _setup(aggr)
    with torch.no_grad():
        for src, dst, t, raw in batches[:2]:
            mem.update_state(src.to(DEV), dst.to(DEV), t.to(DEV), raw.to(DEV))
            oracle.update_state(src, dst, t, raw)
    # eval() commits every node's stored messages and clears the stores (tgn.py:245-251): back in train mode no node holds a
    # message and the memory rows are not zero
    with torch.no_grad():  # (memory is a buffer: the oracle's commit must not tie it to the parameters)
        mem.eval()
        oracle.eval()
    mem.train()
    oracle.train()
    n_id = torch.from_numpy(np.sort(rng.choice(N, 13, replace=False)).astype(np.int32))
    assert not oracle.store[0] and not oracle.store[1] and bool(oracle.memory[n_id.long()].abs().sum(1).gt(0).any())
    assert int((mem._st_cnt[0] + mem._st_cnt[1]).sum()) == 0
    U = n_id.numel()
    edge_index, e_t, e_x = torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(0, D)
    G = torch.from_numpy(rng.standard_normal((U, 16)).astype(np.float32))

    z, lu = mem(n_id.to(DEV))
    z2 = enc(z, lu, edge_index.to(DEV), e_t.to(DEV), e_x.to(DEV))
    loss = (z2 * G.to(DEV)).sum()
    src, dst, t, raw = batches[2]
    mem.update_state(src.to(DEV), dst.to(DEV), t.to(DEV), raw.to(DEV))  # before backward, like the reference loop
    loss.backward()

    zr, lur = oracle.forward(n_id.long())
    z2r = graph_attention_embedding_ref(ep, zr, lur, edge_index, e_t, e_x)
    assert torch.equal(lu.cpu(), lur)
    assert ((z2.detach().cpu() - z2r.detach()).abs() <= 1e-5 * z2r.detach().abs().clamp(min=1)).all()
    (z2r * G).sum().backward()

    named = list(mem.named_parameters()) + [(f'enc.{k}', v) for k, v in enc.named_parameters() if not k.startswith('time_enc.')]
    refs = dict(mp)
    refs.update({f'enc.{k}': v for k, v in ep.items() if not k.startswith('time_enc.')})
    reached, worst = 0, ('', 0.0)
    for name, p in named:
        r = refs[name].grad
        r = torch.zeros_like(refs[name]) if r is None else r
        got = torch.zeros_like(r) if p.grad is None else p.grad.cpu()
        assert got.shape == r.shape, name
        reached += bool(r.any())
        err = ((got - r).abs().max() / r.abs().max().clamp(min=2e-3)).item()
        if err > worst[1]:
            worst = (name, err)
    print(f'[blocks] tgn without edges / messages ({aggr}): worst relative gradient error {worst}')
    assert reached >= 4, 'the GRU and the skip projection must be reached'
    for p in mem.time_enc.parameters():  # rows without events and no edge: nothing reaches Time2Vec
        assert p.grad is None or not bool(p.grad.any())
    assert worst[1] <= 2e-4, worst
