"""The forward float kernels of ``csrc/tgn.hip`` one by one against the float64 restatements of ``oracle/tgn_fwd_ref.py`` (which
``tests/test_tgn_fwd_ref_cpu.py`` pins to ``oracle/tgn_ref.py``), through ctypes: ``tgmx_tgn_gru_gate``, ``tgmx_tgn_aggregate``,
``tgmx_tconv_edge_attr``, ``tgmx_tconv_attend``; the composites ``tgmx_tgn_memory_forward`` and ``tgmx_tconv_forward`` bit for bit
against their parts; and the exact kernels ``tgmx_tgn_store_batch`` (against ``tgmx_tgn_store``) and ``tgmx_tgn_commit_assoc``.
The conventions are those of ``tests/test_tgn_bwd_blocks_gpu.py`` (helpers from ``tests/test_tgat_bwd_blocks_gpu.py``):

* outputs sit in NaN-filled ``Buf``s followed by a sentinel tail of 4096 floats that must be unchanged (integer outputs: a tail of
  sentinel words);
* every case is launched twice and must give equal bits (no forward kernel here adds floats atomically);
* columns that are plain copies are bit-exact (``mem[v]``, ``mem[other]``, ``raw`` under LAST, ``msg`` in edge_attr, ``ws_h``),
  structural zeros are exact (rows without events, ``new_lu = 0``, a (target, head) whose every edge is dropped);
* everything else: elementwise ``n * 2^-24 * magnitude`` with n counted from the kernel code (``gru_chain``, ``aggregate_chain``,
  ``edge_attr_chain``, ``attend_chain``), nothing tuned on the device's result.  ``pytest -rP`` prints the worst err / bound per
  case.

Measured on an MI355X, worst err / bound over the cases of each kernel: gru_gate 0.114 (at (41944, 100)); aggregate 0.108 LAST
(T = 100, M = 100, D = 172) and 0.238 MEAN (M = 100, D = 172, either T); edge_attr 0.121 (every argument in [3e6, 8e6); 0.118 at
(41944, 100, 0)); attend 0.0043 (generic walk, (1, 1); four floats per lane 0.0041 at (2, 4), two 0.0040 at (2, 2); the alignment trio
0.0026; dropout 0.0029); tconv_forward's attention 0.0006; the GRU GEMMs of memory_forward 0.038 of 2e-5 sqrt(K).  The attention's
bound is a worst case over chains of up to ~7 400 operations (the 2049-edge target: 513 edges per wave, a rescale at every edge,
both the sum's and the normaliser's chain) with first-order sensitivities for the softmax: the device's error, a random walk, stays
far below it; what the bound still catches is listed in ``oracle.tgn_fwd_ref.MUTATIONS`` and in
``test_attend_bound_sees_a_lost_last_edge``.  Every bit-for-bit assertion held; no kernel change was needed.
"""
import functools

import pytest
import torch

from oracle import tgn_fwd_ref as ref
from test_tgat_bwd_blocks_gpu import DEV, Buf, _lib, _report, _same_bits

pytestmark = pytest.mark.gpu

gru_case = functools.lru_cache(maxsize=None)(ref.gru_case)
aggr_case = functools.lru_cache(maxsize=None)(ref.aggr_case)
edge_fwd_case = functools.lru_cache(maxsize=None)(ref.edge_fwd_case)
attend_fwd_case = functools.lru_cache(maxsize=None)(ref.attend_fwd_case)
gru_bounds = functools.lru_cache(maxsize=None)(lambda R, M: ref.gru_bounds(gru_case(R, M)))
NEGATIVE_ROW = 3  # the row of aggr_case whose node is handed over as v - N
aggr_tables = functools.lru_cache(maxsize=None)(lambda T, M, D: ref.aggr_tables(aggr_case(T, M, D), negative_row=NEGATIVE_ROW))
aggr_bounds = functools.lru_cache(maxsize=None)(lambda mean, T, M, D: ref.aggr_bounds(aggr_case(T, M, D), mean, aggr_tables(T, M, D)))
edge_bounds = functools.lru_cache(maxsize=None)(lambda case: ref.edge_bounds(edge_fwd_case(case)))
attend_bounds = functools.lru_cache(maxsize=None)(lambda H, C, p: ref.attend_bounds(attend_fwd_case(H, C, p)))

ISENT = -7777


def _dev(t):
    return t.to(DEV).contiguous()


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _untouched(*bufs):
    return all(bool(torch.isnan(b.flat).all()) for b in bufs)


class IBuf:
    """An integer device vector [n] followed by 64 sentinel words."""

    def __init__(self, n, dtype=torch.int64, fill=ISENT):
        self.flat = torch.full((n + 64,), fill, dtype=dtype, device=DEV)
        self.view, self.n, self.fill = self.flat[:n], n, fill
        self.ptr = self.flat.data_ptr()

    def sentinels_intact(self):
        return bool((self.flat[self.n:] == self.fill).all())


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tgn_gru_gate
# ---------------------------------------------------------------------------------------------------------------------------
def _gru_gate(gi, gh, h, R, M):
    lib, native = _lib()
    out = Buf(R, M)
    native.check(lib.tgmx_tgn_gru_gate(_ptr(gi), _ptr(gh), _ptr(h), M, R, out.ptr, native.stream_ptr()), 'gru_gate')
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('R,M', ref.GRU_CASES + [ref.GRU_BIG_CASE])
def test_gru_gate(R, M):
    """(1,1), (3,5), (7,100): one thread, a ragged block, several blocks.  (41944,100): 96 elements past 16384 blocks x 256 -- the
    block cap holds and the grid stride takes a second trip for exactly the tail.  Rows (oracle.tgn_bwd_ref.gru_case): the band with
    pre-activations +-30 and +-95 (expf overflows or lands in the denormals, a gate is exactly 0 or 1: finite outputs, the bound
    gets gru_underflow_floor there), and the row with h == n."""
    c = gru_case(R, M)
    want, bound = gru_bounds(R, M)
    gi, gh, h = (_dev(c[n]) for n in ('gi', 'gh', 'h'))
    a, b = _gru_gate(gi, gh, h, R, M), _gru_gate(gi, gh, h, R, M)
    assert a.sentinels_intact() and b.sentinels_intact(), 'a write past [R, M]'
    assert _same_bits(a.view, b.view), 'two launches differ'
    got = a.view.cpu()
    if R >= 3:
        assert c['band'] and c['hn_row'] is not None and bool(torch.isfinite(got[c['band']]).all())
    assert _report(f'gru_gate {(R, M)}', got, want, bound) <= 1.0


def test_gru_gate_no_rows():
    out = _gru_gate(None, None, None, 0, 3)
    assert _untouched(out)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tgn_aggregate
# ---------------------------------------------------------------------------------------------------------------------------
AGGR_NAMES = ('memory', 'last_update', 'st_lo_s', 'st_cnt_s', 'st_lo_d', 'st_cnt_d', 'log_other', 'log_t', 'log_raw', 'tw', 'tb')


def _aggregate(c, d, nodes, mean, assoc=None, stamp=0):
    """One launch over the row list ``nodes`` (a CPU int32 tensor): (aggr Buf, new_lu IBuf)."""
    lib, native = _lib()
    R, W = nodes.numel(), 2 * c['M'] + c['D'] + c['T']
    nd = _dev(nodes)
    aggr, new_lu = Buf(R, W), IBuf(R)
    assert d['st_cnt_s'].dtype == torch.int32 and d['st_lo_s'].dtype == torch.int64 and d['log_other'].dtype == torch.int32 and nd.dtype == torch.int32
    native.check(lib.tgmx_tgn_aggregate(_ptr(nd), R, d['memory'].data_ptr(), d['last_update'].data_ptr(), c['M'], c['N'], d['st_lo_s'].data_ptr(),
                                        d['st_cnt_s'].data_ptr(), d['st_lo_d'].data_ptr(), d['st_cnt_d'].data_ptr(), d['log_other'].data_ptr(),
                                        d['log_t'].data_ptr(), _ptr(d['log_raw']), c['D'], d['tw'].data_ptr(), d['tb'].data_ptr(), c['T'], mean, aggr.ptr,
                                        new_lu.ptr, None if assoc is None else assoc.ptr, stamp, native.stream_ptr()), 'aggregate')
    torch.cuda.synchronize()
    assert aggr.sentinels_intact() and new_lu.sentinels_intact(), 'a write past [R, W] / [R]'
    return aggr, new_lu


@pytest.mark.parametrize('mean,T,M,D', ref.AGGR_CASES)
def test_aggregate(mean, T, M, D):
    """One wave per row, four rows per block, R = 23 (the last block is ragged and ends on an empty row); lanes across the
    W = 2M + D + T message columns.  (M, D) = (1, 0): W = 3, 66, 67, 102 -- T = 1 | 64 | 65 | 100 puts the time columns on one lane,
    into a second column trip by two lanes, by three, by 38.  (M, D) = (100, 172): W = 373 | 472, six | eight column trips, the last
    ragged, the copies' three sources meeting inside a trip.  Rows (oracle.tgn_bwd_ref.aggr_case): empty (exact zeros, new_lu = 0),
    single, one window only (either), the destination window at LOWER log positions than the source window, totals of 64 / 65 /
    130 (the lane-strided scan's second and third trip), the maximum at walk index 0 / 129 / 127 (a lane's second trip), float32
    ties between distinct unix-scale times within one lane's two trips, across lanes, across the two windows (the FIRST in walk
    order wins: told by its bit-exact raw columns), dt == 0, dt up to 2^31 - 1.  Row 3's node is given as v - N.
    Launch 1 and 2: assoc given (distinct nodes).  Launch 3: assoc NULL, two nodes listed a second time."""
    c, tab = aggr_case(T, M, D), aggr_tables(T, M, D)
    (want, want_lu), bound = aggr_bounds(mean, T, M, D)
    d = {n: _dev(tab[n]) for n in AGGR_NAMES}
    R, N, toff, stamp = c['R'], c['N'], 2 * M + D, 5
    assert int(tab['nodes'][NEGATIVE_ROW]) < 0
    outs = []
    for _ in range(2):
        assoc = IBuf(N, fill=-1)
        aggr, new_lu = _aggregate(c, d, tab['nodes'], mean, assoc, stamp)
        assert assoc.sentinels_intact()
        expect = torch.full((N,), -1, dtype=torch.int64)
        expect[c['nodes'].long()] = (stamp << 32) | torch.arange(R)
        assert torch.equal(assoc.view.cpu(), expect), 'assoc[v] == (stamp << 32) | row for the listed nodes, the sentinel elsewhere'
        outs.append((aggr.view.clone(), new_lu.view.clone()))
    assert _same_bits(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), 'two launches differ'
    got, got_lu = outs[0][0].cpu(), outs[0][1].cpu()
    assert torch.equal(got_lu, want_lu), 'new_lu: the int64 maximum (ties and the 2^31 row included), 0 without events'
    empty = (c['cnt_s'] + c['cnt_d']) == 0
    assert int(empty.sum()) >= 2 and _same_bits(got[empty], torch.zeros(int(empty.sum()), toff + T)) and not bool(got_lu[empty].any())
    if not mean:
        assert _same_bits(got[:, :toff], want[:, :toff].float()), 'LAST: mem[v] | mem[other] | raw are copies'
        for name in ('tie_one_lane', 'tie_lanes', 'tie_windows'):
            r = ref.AGGR_ROW[name]
            walk = c['walk'](r)
            t = c['log_t'][walk]
            first, second = (t.float() == t.float().max()).nonzero()[:, 0].tolist()
            assert int(t[second]) > int(t[first]), 'the later tied event has the larger int64 time'
            assert _same_bits(got[r, M:2 * M], c['memory'][c['log_other'][walk[first]].long()])
            if D:
                assert _same_bits(got[r, 2 * M:toff], c['log_raw'][walk[first]]) and not torch.equal(got[r, 2 * M:toff], c['log_raw'][walk[second]])
    assert _report(f'aggregate mean={mean} T={T} M={M} D={D}', got, want, bound) <= 1.0
    # a row list in which two nodes appear twice, assoc NULL: identical rows
    twice = [ref.AGGR_ROW['total130'], ref.AGGR_ROW['tie_windows']]
    aggr3, lu3 = _aggregate(c, d, torch.cat([tab['nodes'], tab['nodes'][twice]]), mean)
    assert _same_bits(aggr3.view[:R], outs[0][0]) and _same_bits(aggr3.view[R:], outs[0][0][twice])
    assert torch.equal(lu3.view[:R].cpu(), want_lu) and torch.equal(lu3.view[R:].cpu(), want_lu[twice])


def test_aggregate_no_rows():
    c, tab = aggr_case(1, 1, 0), aggr_tables(1, 1, 0)
    d = {n: _dev(tab[n]) for n in AGGR_NAMES}
    assoc = IBuf(c['N'], fill=-1)
    aggr, new_lu = _aggregate(c, d, torch.zeros(0, dtype=torch.int32), 0, assoc, 5)
    assert _untouched(aggr) and bool((new_lu.flat == ISENT).all()) and bool((assoc.flat == -1).all())


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tconv_edge_attr
# ---------------------------------------------------------------------------------------------------------------------------
def _edge_attr(d, E, T, D):
    lib, native = _lib()
    out = Buf(E, T + D)
    native.check(lib.tgmx_tconv_edge_attr(_ptr(d['lu_local']), _ptr(d['src']), _ptr(d['t']), _ptr(d['msg']) if D else None, _ptr(d['tw']), _ptr(d['tb']),
                                          T, D, E, out.ptr, native.stream_ptr()), 'edge_attr')
    torch.cuda.synchronize()
    assert out.sentinels_intact(), 'a write past [E, T + D]'
    return out


@pytest.mark.parametrize('case', ref.EDGE_FWD_CASES, ids=str)
def test_edge_attr(case):
    """(1,1,0), (5,8,3), (37,100,172): one thread, one ragged block, several blocks with the message columns behind the time columns
    (D = 0 passes msg = NULL).  (41944,100,0): E * T is 96 past 16384 blocks x 256 (the cap and the grid stride's second trip).
    lu and t are near 1.7e9 with differences within +-40 (subtract in int64, THEN round), and 0, 2^31 - 3, -(2^31 - 7): arguments up
    to 2.1e9, where their waves take cos_t2v_big.  The two forward-only cases (oracle.tgn_fwd_ref.edge_fwd_case): every argument in
    [3e6, 8e6) -- every wave on cos_t2v_small near its limit, where the one-off correction of k acts; and one edge of 40 that takes
    its wave, and no other, onto cos_t2v_big."""
    c = edge_fwd_case(case)
    want, bound = edge_bounds(case)
    E, T, D = c['E'], c['T'], c['D']
    d = {n: _dev(c[n]) for n in ('lu_local', 'src', 't', 'tw', 'tb', 'msg')}
    a, b = _edge_attr(d, E, T, D), _edge_attr(d, E, T, D)
    assert _same_bits(a.view, b.view), 'two launches differ'
    got = a.view.cpu()
    if D:
        assert _same_bits(got[:, T:], c['msg']), 'the message columns are copies'
    assert _report(f'edge_attr {case}', got, want, bound) <= 1.0


def test_edge_attr_no_edges():
    out = _edge_attr(dict(lu_local=None, src=None, t=None, msg=None, tw=None, tb=None), 0, 8, 3)
    assert _untouched(out)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tconv_attend
# ---------------------------------------------------------------------------------------------------------------------------
def _shifted(t, floats):
    """A contiguous device copy of ``t`` whose first element sits ``floats`` floats past a 256-byte aligned address."""
    base = torch.empty(t.numel() + 8, dtype=torch.float32, device=DEV)
    assert base.data_ptr() % 256 == 0
    view = base[floats:floats + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _attend(c, d, e_dev, expect_walk):
    """One launch on the sorted route (``order`` is the stable sort by target), ``out`` pre-filled with the skip block."""
    lib, native = _lib()
    U, H, C = c['U'], c['H'], c['C']
    out = Buf(U, H * C, data=c['out0'])
    walk = ref.tconv_walk(H, C, d['q'].data_ptr(), d['k'].data_ptr(), d['v'].data_ptr(), e_dev.data_ptr(), out.ptr)
    assert walk == expect_walk, f'(H, C) = {(H, C)}: tconv_short_ok gives walk {walk}, the table expects {expect_walk}'
    native.check(lib.tgmx_tconv_attend(d['q'].data_ptr(), d['k'].data_ptr(), d['v'].data_ptr(), e_dev.data_ptr(), d['order'].data_ptr(),
                                       d['src'].data_ptr(), d['seg_lo'].data_ptr(), d['seg_hi'].data_ptr(), U, H, C, c['scale'], out.ptr,
                                       native.dropout_desc(c['p'], ref.DROP_SEED, c['stream']), native.stream_ptr()), 'attend')
    torch.cuda.synchronize()
    assert out.sentinels_intact(), 'a write past [U, H * C]'
    return out.view.clone()


def _check_attend(tag, c, got, want, bound):
    none = c['seg_hi'] == c['seg_lo']
    assert int(none.sum()) == 2 and _same_bits(got.cpu()[none], c['out0'][none]), 'a target without edges keeps the skip bits'
    return _report(tag, got, want, bound)


@pytest.mark.parametrize('H,C', list(ref.ATTEND_FWD_WIDTHS))
def test_attend(H, C):
    """One workgroup of four waves per target, U = 19 targets with 0, 1, 2, 3, 4, 5, 16, 17, 64, 65, 255, 256, 257, 300, 1024, 1025,
    2049, 12, 0 incoming edges (oracle.tgn_fwd_ref.attend_fwd_case): the blocks of four edges end ragged or full (1 .. 5), the
    one-wave walk ends at 16 | 17, a wave's 64-position trip at 256 | 257 and 1024 | 1025, 2049 leaves one wave a third trip of one
    edge; one source feeds the 2049-edge target throughout, a self loop, and two targets whose scores spread by 120 (weights
    underflow to exactly 0; at the 300-edge one wave 2's whole share lies below the others' maximum: its merge factor is 0); the LAST
    position of the 5-, 17-, 65-, 257-, 1025- and 2049-edge segments carries most of its target's weight, so a walk that loses the
    edge past a boundary leaves the bound (tests/test_tgn_fwd_ref_cpu.py::test_attend_bound_sees_a_lost_last_edge).
    The walk each width reaches (oracle.tgn_fwd_ref.ATTEND_FWD_WIDTHS, asserted from tconv_short_ok's rule on the real pointers):
    four floats per lane (2,4) one lane on | (2,64) 16 | (2,128) all 32; two floats per lane (2,2) one | (2,50) 25 | (2,62) 31;
    generic (2,3) odd C | (2,65) two column trips | (2,132) three | (1,1) | (1,64) | (3,33) | (3,70) two trips, three heads."""
    c = attend_fwd_case(H, C, 0.0)
    want, bound = attend_bounds(H, C, 0.0)
    d = {n: _dev(c[n]) for n in ('q', 'k', 'v', 'eproj', 'order', 'src', 'seg_lo', 'seg_hi')}
    walk = ref.ATTEND_FWD_WIDTHS[H, C]
    a, b = _attend(c, d, d['eproj'], walk), _attend(c, d, d['eproj'], walk)
    assert _same_bits(a, b), 'two launches differ'
    assert _check_attend(f'attend {(H, C)} walk {walk}', c, a, want, bound) <= 1.0


def test_attend_alignment():
    """(2, 8) with eproj on the 16-byte grid, 8 bytes off it and 4 bytes off it (only that pointer moves): the four-float walk, the
    two-float walk and the generic walk, one restatement, each within the bound."""
    H, C = ref.ATTEND_FWD_ALIGN
    c = attend_fwd_case(H, C, 0.0)
    want, bound = attend_bounds(H, C, 0.0)
    d = {n: _dev(c[n]) for n in ('q', 'k', 'v', 'order', 'src', 'seg_lo', 'seg_hi')}
    worst = {}
    for floats, walk in ((0, 4), (2, 2), (1, 0)):
        e_dev = _shifted(c['eproj'], floats)
        a, b = _attend(c, d, e_dev, walk), _attend(c, d, e_dev, walk)
        assert _same_bits(a, b), 'two launches differ'
        worst[walk] = _check_attend(f'attend {(H, C)} eproj {4 * floats} bytes off the grid, walk {walk}', c, a, want, bound)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('H,C,p', ref.ATTEND_FWD_DROPOUT)
def test_attend_dropout(H, C, p):
    """Dropout through tgmx_dropout_t on the four-float walk (2, 64) and the generic walk (3, 33), keep from dropout_scale: the
    softmax normalises over every edge, dropout then zeroes / rescales single coefficients.  p = 0.5: target 1's only edge is
    dropped in head 0 -- that head's columns keep the skip bits."""
    c = attend_fwd_case(H, C, p)
    want, bound = attend_bounds(H, C, p)
    d = {n: _dev(c[n]) for n in ('q', 'k', 'v', 'eproj', 'order', 'src', 'seg_lo', 'seg_hi')}
    walk = ref.ATTEND_FWD_WIDTHS[H, C]
    a, b = _attend(c, d, d['eproj'], walk), _attend(c, d, d['eproj'], walk)
    assert _same_bits(a, b), 'two launches differ'
    if p == 0.5:
        e1 = int((c['tgt'] == 1).nonzero()[0])
        assert float(c['keep'][e1, 0]) == 0.0 and _same_bits(a.cpu()[1, :C], c['out0'][1, :C]), 'every edge dropped: exactly 0 is added'
    assert _check_attend(f'attend {(H, C)} p={p} walk {walk}', c, a, want, bound) <= 1.0


def test_attend_no_targets():
    lib, native = _lib()
    out = Buf(0, 8)
    native.check(lib.tgmx_tconv_attend(None, None, None, None, None, None, None, None, 0, 2, 4, 0.5, out.ptr, None, native.stream_ptr()), 'attend U = 0')
    torch.cuda.synchronize()
    assert _untouched(out)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tgn_memory_forward: aggregate (with the h_out rider) -> the two GRU GEMMs -> the gates
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,M,D', [(100, 100, 172), (65, 32, 16)])
def test_memory_forward_equals_its_parts(T, M, D):
    """R = 23 (the aggr_case rows, LAST then MEAN): ws_aggr and out_lu carry tgmx_tgn_aggregate's bits, ws_h is memory[nodes]
    exactly (the ``h_out`` rider, reachable only here; row 3's node is negative), out_mem is tgmx_tgn_gru_gate of the workspaces the
    call left, bit for bit, and ws_gi / ws_gh lie within the bar of tests/test_gemm_gpu.py (2e-5 sqrt(K)) of the float64 product of
    the device's own operands."""
    lib, native = _lib()
    c, tab = aggr_case(T, M, D), aggr_tables(T, M, D)
    d = {n: _dev(tab[n]) for n in AGGR_NAMES}
    R, N, W = c['R'], c['N'], 2 * M + D + T
    g = torch.Generator().manual_seed(17 * T + M)
    W_ih, b_ih, W_hh, b_hh = torch.randn(3 * M, W, generator=g), torch.randn(3 * M, generator=g), torch.randn(3 * M, M, generator=g), torch.randn(3 * M, generator=g)
    wd = [_dev(t) for t in (W_ih, b_ih, W_hh, b_hh)]
    nd = _dev(tab['nodes'])
    for mean in (0, 1):
        part_aggr, part_lu = _aggregate(c, d, tab['nodes'], mean)
        runs = []
        for _ in range(2):
            ws = dict(aggr=Buf(R, W), h=Buf(R, M), gi=Buf(R, 3 * M), gh=Buf(R, 3 * M), out=Buf(R, M))
            out_lu, assoc = IBuf(R), IBuf(N, fill=-1)
            a = native.TgnMemoryFwd()
            a.nodes, a.R, a.memory, a.last_update, a.M, a.num_nodes = nd.data_ptr(), R, d['memory'].data_ptr(), d['last_update'].data_ptr(), M, N
            a.st_lo_s, a.st_cnt_s, a.st_lo_d, a.st_cnt_d = (d[n].data_ptr() for n in ('st_lo_s', 'st_cnt_s', 'st_lo_d', 'st_cnt_d'))
            a.log_other, a.log_t, a.log_raw, a.D = d['log_other'].data_ptr(), d['log_t'].data_ptr(), _ptr(d['log_raw']), D
            a.tw, a.tb, a.T, a.mean = d['tw'].data_ptr(), d['tb'].data_ptr(), T, mean
            a.W_ih, a.b_ih, a.W_hh, a.b_hh = (t.data_ptr() for t in wd)
            a.ws_aggr, a.ws_h, a.ws_gi, a.ws_gh = ws['aggr'].ptr, ws['h'].ptr, ws['gi'].ptr, ws['gh'].ptr
            a.out_mem, a.out_lu, a.assoc, a.stamp = ws['out'].ptr, out_lu.ptr, assoc.ptr, 9
            native.check(lib.tgmx_tgn_memory_forward(a, native.stream_ptr()), 'memory_forward')
            torch.cuda.synchronize()
            assert all(b.sentinels_intact() for b in ws.values()) and out_lu.sentinels_intact() and assoc.sentinels_intact()
            runs.append({k: b.view.clone() for k, b in ws.items()})
        assert all(_same_bits(runs[0][k], runs[1][k]) for k in runs[0]), 'two launches differ'
        r = runs[0]
        assert _same_bits(r['aggr'], part_aggr.view) and torch.equal(out_lu.view, part_lu.view), 'the composite aggregates as tgmx_tgn_aggregate does'
        assert int(assoc.view[int(c['nodes'][NEGATIVE_ROW])]) == (9 << 32) | NEGATIVE_ROW
        assert _same_bits(r['h'].cpu(), c['memory'][c['nodes'].long()]), 'ws_h = memory[nodes]'
        gate = _gru_gate(r['gi'].contiguous(), r['gh'].contiguous(), r['h'].contiguous(), R, M)
        assert _same_bits(r['out'], gate.view), 'out_mem = tgmx_tgn_gru_gate(ws_gi, ws_gh, ws_h)'
        gi64 = r['aggr'].cpu().double() @ W_ih.double().T + b_ih.double()
        gh64 = r['h'].cpu().double() @ W_hh.double().T + b_hh.double()
        assert _report(f'memory_forward {(T, M, D)} mean={mean} ws_gi', r['gi'], gi64, 2e-5 * W ** 0.5) <= 1.0
        assert _report(f'memory_forward {(T, M, D)} mean={mean} ws_gh', r['gh'], gh64, 2e-5 * M ** 0.5) <= 1.0


def test_memory_forward_no_rows():
    lib, native = _lib()
    out, out_lu = Buf(0, 4), IBuf(0)
    a = native.TgnMemoryFwd()
    a.R, a.M, a.D, a.T, a.num_nodes, a.out_mem, a.out_lu = 0, 4, 0, 8, 10, out.ptr, out_lu.ptr
    native.check(lib.tgmx_tgn_memory_forward(a, native.stream_ptr()), 'memory_forward R = 0')
    torch.cuda.synchronize()
    assert _untouched(out) and out_lu.sentinels_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tconv_forward: the counting grouping against the segment-sort route, its attention against the restatement
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tconv_inputs(H, C):
    tgt, src, order, seg_lo, seg_hi = ref.attend_fwd_graph()
    U, E, HC, in_ch, T, D = ref.ATTEND_FWD_U, tgt.numel(), H * C, 100, 100, 172
    g = torch.Generator().manual_seed(31 * C + H)
    tw, tb = ref.time2vec_params(T, g)
    lu = ref.UNIX + torch.randint(0, 1_000_000, (U,), generator=g)
    t = lu[src] - torch.randint(-40, 41, (E,), generator=g)
    return dict(tgt=tgt, src=src, order=order, seg_lo=seg_lo, seg_hi=seg_hi, U=U, E=E, in_ch=in_ch, T=T, D=D, tw=tw, tb=tb, lu=lu, t=t,
                x=torch.randn(U, in_ch, generator=g), msg=torch.randn(E, D, generator=g), W4=torch.randn(4, HC, in_ch, generator=g) / in_ch ** 0.5,
                b4=torch.randn(4, HC, generator=g), W_edge=torch.randn(HC, T + D, generator=g) / (T + D) ** 0.5)


def _tconv_forward(H, C, route):
    """One call: route 'sort' (no histogram buffers), 'count' (tgt_count, cursor, order_big given) or 'skip' (E = 0).
    Returns (qkvs [4, U, HC], eproj [E, HC], tgt_count, status, (q, k, v, eproj, out) pointers)."""
    lib, native = _lib()
    i = _tconv_inputs(H, C)
    U, E, HC, T, D = i['U'], (0 if route == 'skip' else i['E']), H * C, i['T'], i['D']
    d = {n: _dev(i[n]) for n in ('x', 'lu', 'src', 'tgt', 't', 'msg', 'tw', 'tb', 'W4', 'b4', 'W_edge')}
    qkvs, attr, eproj = Buf(4 * U, HC), Buf(i['E'], T + D), Buf(i['E'], HC)
    order, seg_lo, seg_hi, cursor, order_big = IBuf(i['E']), IBuf(U), IBuf(U), IBuf(U), IBuf(i['E'])
    count = torch.zeros(U + 64, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(int(lib.tgmx_segment_sort_workspace_bytes(i['E'])), 256), dtype=torch.uint8, device=DEV)
    a = native.TconvFwd()
    a.x, a.U, a.in_ch, a.last_update_local = d['x'].data_ptr(), U, i['in_ch'], d['lu'].data_ptr()
    a.src, a.tgt, a.t, a.msg, a.E, a.D, a.T = d['src'].data_ptr(), d['tgt'].data_ptr(), d['t'].data_ptr(), d['msg'].data_ptr(), E, D, T
    a.tw, a.tb, a.W4, a.b4, a.W_edge, a.H, a.C = d['tw'].data_ptr(), d['tb'].data_ptr(), d['W4'].data_ptr(), d['b4'].data_ptr(), d['W_edge'].data_ptr(), H, C
    a.edge_attr, a.qkvs, a.eproj = attr.ptr, qkvs.ptr, eproj.ptr
    a.order, a.seg_lo, a.seg_hi = order.ptr, seg_lo.ptr, seg_hi.ptr
    a.sort_ws, a.sort_ws_bytes, a.status = ws.data_ptr(), ws.numel(), status.data_ptr()
    if route == 'count':
        a.tgt_count, a.cursor, a.order_big = count.data_ptr(), cursor.ptr, order_big.ptr
    native.check(lib.tgmx_tconv_forward(a, native.stream_ptr()), f'tconv_forward ({route})')
    torch.cuda.synchronize()
    assert all(b.sentinels_intact() for b in (qkvs, attr, eproj, order, seg_lo, seg_hi, cursor, order_big))
    ptrs = (qkvs.ptr, qkvs.ptr + 4 * U * HC, qkvs.ptr + 8 * U * HC, eproj.ptr, qkvs.ptr + 12 * U * HC)
    return qkvs.view.clone().view(4, U, HC), eproj.view.clone(), count, int(status.item()), ptrs, (seg_lo.view.clone(), seg_hi.view.clone())


@pytest.mark.parametrize('H,C,walk', [(2, 50, 2), (2, 64, 4)])
def test_tconv_forward_counting_route(H, C, walk, monkeypatch):
    """The segment table of test_attend through the one-call layer (in_ch = 100, T = 100, D = 172).  On the counting route ``order``
    holds a target's edge ids as the atomics placed them and the attention sorts them first: ranked in registers (up to 16
    edges), ranked in LDS (17 .. 1024), runs of 1024 merged through ``order_big`` (1025, 2049) -- ascending edge id is the stable
    order, so the result equals the segment-sort route bit for bit, with TGMX_TCONV_GROUP_FUSED 1 (scan + placement in one
    launch; the attention clears the histogram) and 0; ``tgt_count`` is left zero.  The q | k | v blocks of all calls carry equal
    bits; out against ``attend`` on the blocks the call left, the skip block taken from a call with E = 0."""
    monkeypatch.delenv('TGMX_TCONV_COUNTING', raising=False)
    i = _tconv_inputs(H, C)
    U, E = i['U'], i['E']
    qs, es, _, st, ptrs, seg = _tconv_forward(H, C, 'sort')
    assert st == 0 and ref.tconv_walk(H, C, *ptrs) == walk
    assert torch.equal(seg[0].cpu(), i['seg_lo']) and torch.equal(seg[1].cpu(), i['seg_hi'])
    q0, _, _, _, _, _ = _tconv_forward(H, C, 'skip')
    assert _same_bits(q0[:3], qs[:3]), 'q | k | v of the call without edges'
    for fused in ('1', '0'):
        monkeypatch.setenv('TGMX_TCONV_GROUP_FUSED', fused)
        runs = [_tconv_forward(H, C, 'count') for _ in range(2)]
        for qc, ec, count, stc, ptrs_c, seg_c in runs:
            assert stc == 0 and not bool(count.any()), 'tgt_count is left zero'
            assert ref.tconv_walk(H, C, *ptrs_c) == walk
            assert torch.equal(seg_c[0].cpu(), i['seg_lo']) and torch.equal(seg_c[1].cpu(), i['seg_hi'])
            assert _same_bits(ec, es), 'eproj'
            assert _same_bits(qc[:3], qs[:3]), 'q | k | v'
            assert _same_bits(qc[3], qs[3]), f'the counting grouping (fused={fused}) against the segment-sort route'
    qc = runs[0][0].cpu()
    skip = q0[3].cpu()
    c = dict(q=qc[0], k=qc[1], v=qc[2], eproj=es.cpu(), order=i['order'], src=i['src'], seg_lo=i['seg_lo'], seg_hi=i['seg_hi'], H=H, C=C,
             scale=float(torch.tensor(1.0) / torch.sqrt(torch.tensor(float(C)))), out0=skip, keep=torch.ones(E, H))
    want, bound = ref.attend_bounds(c)
    none = i['seg_hi'] == i['seg_lo']
    assert _same_bits(qc[3][none], skip[none]), 'a target without edges keeps the skip bits'
    assert _report(f'tconv_forward {(H, C)} counting route, walk {walk}', qc[3], want, bound) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tgn_store_batch against tgmx_tgn_store, tgmx_tgn_commit_assoc (exact)
# ---------------------------------------------------------------------------------------------------------------------------
STORE_NODES, STORE_BASE = 50, 5


def _store_buffers(n, D):
    cap = STORE_BASE + 2 * n + 3
    return dict(log_other=torch.full((cap,), ISENT, dtype=torch.int32, device=DEV), log_t=torch.full((cap,), ISENT, dtype=torch.int64, device=DEV),
                log_raw=torch.full((cap, D), float('nan'), device=DEV), st_lo=torch.full((2, STORE_NODES), ISENT, dtype=torch.int64, device=DEV),
                st_cnt=torch.full((2, STORE_NODES), ISENT, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize('D', [0, 3])
@pytest.mark.parametrize('n', [1, 2, 1023, 1024])
def test_store_batch_equals_store(n, D):
    """One launch for both roles (workgroup ``role`` sorts its n keys in LDS: 64 threads at n = 1, 2, 1024 at 1023 -- one idle thread --
    and 1024) against tgmx_tgn_store fed from a stable torch.sort on the host, and both against a Python grouping: the log rows
    [base + role * n, + n) in node-sorted, then batch order and every node's (lo, cnt) window, exactly; nodes repeat (50 ids), a node
    sits in both roles (n = 1: a self event), windows of nodes outside the batch and the log around the rows stay untouched."""
    lib, native = _lib()
    g = torch.Generator().manual_seed(100 * n + D)
    if n == 1:
        src, dst = torch.tensor([7]), torch.tensor([7])
    elif n == 2:
        src, dst = torch.tensor([3, 3]), torch.tensor([5, 3])
    else:
        src, dst = torch.randint(0, STORE_NODES - 4, (n,), generator=g), torch.randint(0, STORE_NODES - 4, (n,), generator=g)
        assert src.unique().numel() < n and bool(torch.isin(src, dst).any())
    src, dst = src.to(torch.int32), dst.to(torch.int32)
    t = ref.UNIX + torch.randint(0, 1_000_000, (n,), generator=g)
    raw = torch.randn(n, D, generator=g)
    # the Python grouping
    cap = STORE_BASE + 2 * n + 3
    e_other, e_t = torch.full((cap,), ISENT, dtype=torch.int32), torch.full((cap,), ISENT, dtype=torch.int64)
    e_raw = torch.full((cap, D), float('nan'))
    e_lo, e_cnt = torch.full((2, STORE_NODES), ISENT, dtype=torch.int64), torch.full((2, STORE_NODES), ISENT, dtype=torch.int32)
    for role, (ids, oth) in enumerate(((src, dst), (dst, src))):
        groups = {}
        for e, v in enumerate(ids.tolist()):
            groups.setdefault(v, []).append(e)
        p = STORE_BASE + role * n
        for v in sorted(groups):
            e_lo[role, v], e_cnt[role, v] = p, len(groups[v])
            for e in groups[v]:
                e_other[p], e_t[p], e_raw[p] = oth[e], t[e], raw[e]
                p += 1
    sd, dd, td, rd = _dev(src), _dev(dst), _dev(t), _dev(raw)
    one = _store_buffers(n, D)
    native.check(lib.tgmx_tgn_store_batch(sd.data_ptr(), dd.data_ptr(), td.data_ptr(), _ptr(rd), D, n, STORE_BASE, one['log_other'].data_ptr(),
                                          one['log_t'].data_ptr(), _ptr(one['log_raw']), one['st_lo'][0].data_ptr(), one['st_cnt'][0].data_ptr(),
                                          one['st_lo'][1].data_ptr(), one['st_cnt'][1].data_ptr(), native.stream_ptr()), 'store_batch')
    two = _store_buffers(n, D)
    for role, (ids, oth) in enumerate(((sd, dd), (dd, sd))):
        srt, perm = torch.sort(ids, stable=True)
        left = torch.searchsorted(srt, srt, right=False)
        right = torch.searchsorted(srt, srt, right=True)
        native.check(lib.tgmx_tgn_store(perm.data_ptr(), srt.data_ptr(), left.data_ptr(), right.data_ptr(), oth.data_ptr(), td.data_ptr(), _ptr(rd), D, n,
                                        STORE_BASE + role * n, two['log_other'].data_ptr(), two['log_t'].data_ptr(), _ptr(two['log_raw']),
                                        two['st_lo'][role].data_ptr(), two['st_cnt'][role].data_ptr(), native.stream_ptr()), 'store')
    torch.cuda.synchronize()
    for got in (one, two):
        assert torch.equal(got['log_other'].cpu(), e_other) and torch.equal(got['log_t'].cpu(), e_t)
        assert _same_bits(got['log_raw'].cpu(), e_raw)
        assert torch.equal(got['st_lo'].cpu(), e_lo) and torch.equal(got['st_cnt'].cpu(), e_cnt)
    assert int((e_lo[0] == ISENT).sum()) >= 4, 'nodes outside the batch'


def test_commit_assoc():
    """memory[v] = val[row(v)], last_update[v] = lu[row(v)] for every entry of [src | dst] whose node carries the forward's stamp;
    M = 100 (two column trips), duplicate endpoints write the same values, one node is given as v - N; a node with a STALE stamp
    sets *status to 1 and keeps its row; every other row of memory / last_update is untouched."""
    lib, native = _lib()
    g = torch.Generator().manual_seed(3)
    N, M, R, stamp = 30, 100, 12, 6
    fw = torch.randperm(N, generator=g)[:R]  # the rows of the preceding forward
    stale = int(fw[4])
    assoc = torch.full((N,), -1, dtype=torch.int64)
    assoc[fw] = (stamp << 32) | torch.arange(R)
    assoc[stale] = ((stamp - 1) << 32) | 4
    val, lu = torch.randn(R, M, generator=g), ref.UNIX + torch.randint(0, 1_000_000, (R,), generator=g)
    mem0, lu0 = torch.randn(N, M, generator=g), torch.randint(0, 1000, (N,), generator=g)
    src = torch.tensor([int(fw[0]), int(fw[1]), int(fw[0]), int(fw[2]) - N, stale], dtype=torch.int32)
    dst = torch.tensor([int(fw[1]), int(fw[3]), int(fw[0]), int(fw[5]), int(fw[6])], dtype=torch.int32)
    for with_stale in (True, False):
        n = 5 if with_stale else 4
        memory, last = Buf(N, M, data=mem0), IBuf(N)
        last.view.copy_(lu0)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        ad, vd, ld, sd, dd = _dev(assoc), _dev(val), _dev(lu), _dev(src[:n]), _dev(dst[:n])
        native.check(lib.tgmx_tgn_commit_assoc(sd.data_ptr(), dd.data_ptr(), n, ad.data_ptr(), stamp, vd.data_ptr(), ld.data_ptr(), M, N, memory.ptr,
                                               last.ptr, status.data_ptr(), native.stream_ptr()), 'commit_assoc')
        torch.cuda.synchronize()
        assert memory.sentinels_intact() and last.sentinels_intact()
        e_mem, e_lu = mem0.clone(), lu0.clone()
        for v in torch.cat([src[:n], dst[:n]]).tolist():
            v = v + N if v < 0 else v
            if v != stale:
                row = int(assoc[v]) & 0xffffffff
                e_mem[v], e_lu[v] = val[row], lu[row]
        assert int(status.item()) == (1 if with_stale else 0)
        assert _same_bits(memory.view.cpu(), e_mem) and torch.equal(last.view.cpu(), e_lu)
        assert _same_bits(memory.view.cpu()[stale], mem0[stale]) and int(last.view[stale]) == int(lu0[stale])
