"""Keeps ``oracle/tgn_fwd_ref.py`` honest without a GPU: the float64 restatements that ``tests/test_tgn_fwd_blocks_gpu.py`` holds the
forward float kernels of ``csrc/tgn.hip`` against

* equal ``oracle/tgn_ref.py`` evaluated in float64 (1e-10): ``TGNMemoryRef._gru``, the aggregators through ``_updated``,
  ``transformer_conv_ref`` and ``graph_attention_embedding_ref``; ``attend`` at p = 0 equals a dense softmax written here,
* come with bounds ``n * 2^-24 * magnitude`` that a float32 evaluation of the same formulas meets at EVERY case the GPU file runs,
* lose to every listed mutation at a case in which it can show, and
* are fed by case builders that contain the rows they claim, and that hand the backward tests the tensors they always had.
"""
import contextlib
import functools
import hashlib

import pytest
import torch

from oracle import tgn_fwd_ref as ref
from oracle import tgn_ref
from oracle.tgat_bwd_ref import worst_ratio
from oracle.tgn_ref import TGNMemoryRef, graph_attention_embedding_ref, transformer_conv_ref

F64 = torch.float64
F32 = torch.float32

gru_case = functools.lru_cache(maxsize=None)(ref.gru_case)
aggr_case = functools.lru_cache(maxsize=None)(ref.aggr_case)
edge_fwd_case = functools.lru_cache(maxsize=None)(ref.edge_fwd_case)
attend_fwd_case = functools.lru_cache(maxsize=None)(ref.attend_fwd_case)
gru_bounds = functools.lru_cache(maxsize=None)(lambda R, M: ref.gru_bounds(gru_case(R, M)))
aggr_bounds = functools.lru_cache(maxsize=None)(lambda mean, T, M, D: ref.aggr_bounds(aggr_case(T, M, D), mean))
edge_bounds = functools.lru_cache(maxsize=None)(lambda case: ref.edge_bounds(edge_fwd_case(case)))
attend_bounds = functools.lru_cache(maxsize=None)(lambda H, C, p: ref.attend_bounds(attend_fwd_case(H, C, p)))


def _close(got, want, tol=1e-10):
    return float((got.double() - want.double()).abs().max()) <= tol * max(1.0, float(want.abs().max()))


@contextlib.contextmanager
def _float64_reference(monkeypatch):
    """``oracle/tgn_ref.py`` evaluated in float64: its buffers (``torch.zeros``) follow the default dtype, and its Time2Vec keeps the
    float32 argument of ``tgat_ref.time2vec`` (one fma rounded once) but takes the cosine of it in float64."""
    def time2vec64(t, w, b):
        x = t.unsqueeze(-1).float().double()
        return torch.cos((x * w.reshape(-1).double() + b.double()).float().double())

    monkeypatch.setattr(tgn_ref, 'time2vec', time2vec64)
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatements equal oracle/tgn_ref.py in float64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R,M', ref.GRU_CASES)
def test_gru_gate_equals_the_reference(R, M):
    """Through ``TGNMemoryRef._gru`` itself: W_ih = I (x = gi), W_hh = 0 and a per-row 'bias' gh."""
    c = gru_case(R, M)
    p = {'memory_updater.weight_ih': torch.eye(3 * M, dtype=F64), 'memory_updater.bias_ih': torch.zeros(3 * M, dtype=F64),
         'memory_updater.weight_hh': torch.zeros(3 * M, M, dtype=F64), 'memory_updater.bias_hh': c['gh'].double()}
    want = TGNMemoryRef(1, 0, M, 1, p)._gru(c['gi'].double(), c['h'].double())
    got, mag = ref.gru_gate(c['gi'], c['gh'], c['h'])
    assert got.dtype == F64 and _close(got, want) and bool((mag >= got.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('mean,T,M,D', [(0, 8, 3, 2), (1, 8, 3, 2), (0, 1, 1, 0), (1, 65, 1, 0)])
def test_aggregate_equals_the_reference(mean, T, M, D, monkeypatch):
    """Through ``TGNMemoryRef._updated`` with the GRU replaced by the identity on its first operand: the store holds every row's
    windows as (other, t, raw) per role; one row's node is given as v - N to the restatement."""
    c = aggr_case(T, M, D)
    tab = ref.aggr_tables(c, negative_row=3)
    with _float64_reference(monkeypatch):
        o = TGNMemoryRef(c['N'], D, M, T, {'time_enc.w.weight': c['tw'][:, None], 'time_enc.w.bias': c['tb']}, aggr='mean' if mean else 'last')
        o.memory, o.last_update = c['memory'].double(), tab['last_update'].clone()
        for r, v in enumerate(c['nodes'].tolist()):
            for role, (lo, cnt) in enumerate(((c['lo_s'], c['cnt_s']), (c['lo_d'], c['cnt_d']))):
                if int(cnt[r]):
                    pos = int(lo[r]) + torch.arange(int(cnt[r]))
                    o.store[role][v] = (c['log_other'][pos], c['log_t'][pos], c['log_raw'][pos].double())
        o._gru = lambda x, h: x
        want, want_lu = o._updated(c['nodes'].long())
    got, new_lu, _ = ref.aggregate(*ref.aggr_args(tab, mean))
    assert want.dtype == F64 and _close(got, want) and torch.equal(new_lu, want_lu)
    empty = (c['cnt_s'] + c['cnt_d']) == 0
    assert int(empty.sum()) >= 2 and not bool(got[empty].any()) and not bool(new_lu[empty].any())


def _conv_params(H, C, in_ch, Wd, g):
    HC = H * C
    p = {}
    for name in ('lin_query', 'lin_key', 'lin_value', 'lin_skip'):
        p[f'conv.{name}.weight'] = torch.randn(HC, in_ch, generator=g, dtype=F64) / in_ch ** 0.5
        p[f'conv.{name}.bias'] = torch.randn(HC, generator=g, dtype=F64)
    p['conv.lin_edge.weight'] = torch.randn(HC, Wd, generator=g, dtype=F64) / Wd ** 0.5
    return p


@pytest.mark.parametrize('H,C,p', [(2, 2, 0.0), (2, 8, 0.0), (3, 33, 0.5), (2, 64, 0.1), (1, 1, 0.0)])
def test_attend_equals_transformer_conv_ref(H, C, p):
    """Through ``transformer_conv_ref`` itself: x = [q | k | v | out0] with selector weights, lin_edge = I, and its own dropout mask
    from (p, seed, stream) -- the keep the case carries."""
    c = attend_fwd_case(H, C, p)
    HC = H * C
    sel = lambda i: torch.eye(4 * HC, dtype=F64)[i * HC:(i + 1) * HC]
    prm = {'lin_query.weight': sel(0), 'lin_key.weight': sel(1), 'lin_value.weight': sel(2), 'lin_skip.weight': sel(3),
           'lin_edge.weight': torch.eye(HC, dtype=F64)}
    x = torch.cat([c[n].double() for n in ('q', 'k', 'v', 'out0')], 1)
    want = transformer_conv_ref(prm, '', H, x, torch.stack([c['src'], c['tgt']]), c['eproj'].double(), dropout=(p, ref.DROP_SEED, c['stream']) if p else None)
    got, _ = ref.attend(*ref.attend_args(c))
    assert _close(got, want)
    none = c['seg_hi'] == c['seg_lo']
    assert int(none.sum()) == 2 and torch.equal(got[none], c['out0'].double()[none])


@pytest.mark.parametrize('H,C', [(2, 3), (1, 64), (2, 50)])
def test_attend_equals_a_dense_softmax(H, C):
    """p = 0 against a dense [U, E] score matrix per head, masked to the target's edges, softmax over the row."""
    c = attend_fwd_case(H, C, 0.0)
    U, E = c['U'], c['E']
    q, k, v, e = (c[n].double().view(-1, H, C) for n in ('q', 'k', 'v', 'eproj'))
    want = c['out0'].double().clone().view(U, H, C)
    incoming = c['tgt'][None, :] == torch.arange(U)[:, None]  # [U, E]
    for h in range(H):
        key, val = k[c['src'], h] + e[:, h], v[c['src'], h] + e[:, h]  # [E, C]
        score = (q[:, h] @ key.T) / C ** 0.5
        score = score.masked_fill(~incoming, -float('inf'))
        a = torch.softmax(score, 1)
        a = torch.where(incoming.any(1, keepdim=True), a, torch.zeros_like(a))
        want[:, h] += a @ val
    got, _ = ref.attend(*ref.attend_args(c))
    assert _close(got, want.view(U, H * C))


@pytest.mark.parametrize('C', [4, 25])
def test_edge_attr_and_attend_equal_graph_attention_embedding_ref(C, monkeypatch):
    """edge_attr -> (float64 product with lin_edge) -> attend, on the shared segment table with unix-scale times, against
    ``graph_attention_embedding_ref`` (two heads)."""
    H, T, D, in_ch = 2, 8, 3, 5
    c = attend_fwd_case(H, C, 0.0)
    U, E, HC = c['U'], c['E'], H * C
    g = torch.Generator().manual_seed(5)
    p = _conv_params(H, C, in_ch, T + D, g)
    tw, tb = ref.time2vec_params(T, g)
    p['time_enc.w.weight'], p['time_enc.w.bias'] = tw[:, None], tb
    x = torch.randn(U, in_ch, generator=g, dtype=F64)
    lu = ref.UNIX + torch.randint(0, 1_000_000, (U,), generator=g)
    t = lu[c['src']] - torch.randint(-40, 41, (E,), generator=g)
    msg = torch.randn(E, D, generator=g)
    with _float64_reference(monkeypatch):
        want = graph_attention_embedding_ref(p, x, lu, torch.stack([c['src'], c['tgt']]), t, msg.double())
    attr, _ = ref.edge_attr(lu, c['src'], t, msg, tw, tb)
    lin = lambda n: x @ p[f'conv.{n}.weight'].T + p[f'conv.{n}.bias']
    got, _ = ref.attend(lin('lin_query'), lin('lin_key'), lin('lin_value'), attr @ p['conv.lin_edge.weight'].T, c['order'], c['src'], c['seg_lo'],
                        c['seg_hi'], H, C, float(C) ** -0.5, lin('lin_skip'), torch.ones(E, H))
    assert want.dtype == F64 and _close(got, want)


# ---------------------------------------------------------------------------------------------------------------------------
# the bounds leave room for float32: the same formulas in float32 stay inside at EVERY case of the GPU file
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R,M', ref.GRU_CASES + [ref.GRU_BIG_CASE])
def test_gru_gate_float32_within_the_bound(R, M):
    c = gru_case(R, M)
    got = ref.gru_gate(c['gi'], c['gh'], c['h'], dtype=F32)[0]
    assert got.dtype == F32 and bool(torch.isfinite(got).all())
    w = worst_ratio(got, *gru_bounds(R, M))
    print(f'[float32] gru_gate {(R, M)}: {w:.3f}')
    assert w <= 1.0


@pytest.mark.parametrize('mean,T,M,D', ref.AGGR_CASES)
def test_aggregate_float32_within_the_bound(mean, T, M, D):
    c = aggr_case(T, M, D)
    (want, want_lu), bound = aggr_bounds(mean, T, M, D)
    got, new_lu, _ = ref.aggregate(*ref.aggr_args(ref.aggr_tables(c), mean), dtype=F32)
    w = worst_ratio(got, want, bound)
    print(f'[float32] aggregate {(mean, T, M, D)}: {w:.3f}')
    assert w <= 1.0 and torch.equal(new_lu, want_lu)
    if not mean:  # the plain copies: equal bits
        toff = 2 * M + D
        assert torch.equal(got[:, :toff].double(), want[:, :toff])


@pytest.mark.parametrize('case', ref.EDGE_FWD_CASES, ids=str)
def test_edge_attr_float32_within_the_bound(case):
    c = edge_fwd_case(case)
    got = ref.edge_attr(c['lu_local'], c['src'], c['t'], c['msg'], c['tw'], c['tb'], dtype=F32)[0]
    w = worst_ratio(got, *edge_bounds(case))
    print(f'[float32] edge_attr {case}: {w:.3f}')
    assert w <= 1.0


@pytest.mark.parametrize('H,C,p', ref.ATTEND_FWD_CASES)
def test_attend_float32_within_the_bound(H, C, p):
    c = attend_fwd_case(H, C, p)
    got = ref.attend(*ref.attend_args(c), dtype=F32)[0]
    assert bool(torch.isfinite(got).all())
    w = worst_ratio(got, *attend_bounds(H, C, p))
    print(f'[float32] attend {(H, C, p)}: {w:.3f}')
    assert w <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# the bounds notice what they must
# ---------------------------------------------------------------------------------------------------------------------------
def _applies(mutation, kernel, **info):
    where, applies = ref.MUTATIONS[mutation]
    return kernel in where.split('+') and applies(**info)


def _mutation_ratios(mutation):
    """{case: err / bound} of the mutated restatement over every case of the GPU file in which the mutation can show (the large
    GRU / edge cases are left to the small ones: the same rows, 4 M elements)."""
    out = {}
    for R, M in ref.GRU_CASES:
        if _applies(mutation, 'gru'):
            c = gru_case(R, M)
            out['gru', R, M] = worst_ratio(ref.gru_gate(c['gi'], c['gh'], c['h'], mutate=mutation)[0], *gru_bounds(R, M))
    for mean, T, M, D in ref.AGGR_CASES:
        if _applies(mutation, 'aggregate', mean=mean):
            (want, _), bound = aggr_bounds(mean, T, M, D)
            got = ref.aggregate(*ref.aggr_args(ref.aggr_tables(aggr_case(T, M, D)), mean), mutate=mutation)[0]
            out['aggregate', mean, T, M, D] = worst_ratio(got, want, bound)
    for case in ref.EDGE_FWD_CASES:
        if _applies(mutation, 'edge_attr') and case != ref.EDGE_BIG_CASE:
            c = edge_fwd_case(case)
            got = ref.edge_attr(c['lu_local'], c['src'], c['t'], c['msg'], c['tw'], c['tb'], mutate=mutation)[0]
            out['edge_attr', case] = worst_ratio(got, *edge_bounds(case))
    for H, C, p in ref.ATTEND_FWD_CASES:
        if _applies(mutation, 'attend', H=H, C=C, p=p):
            got = ref.attend(*ref.attend_args(attend_fwd_case(H, C, p)), mutate=mutation)[0]
            out['attend', H, C, p] = worst_ratio(got, *attend_bounds(H, C, p))
    return out


REQUIRED_MUTATIONS = ['last_tie_last_wins', 'last_argmax_int64', 'ignore_destination_window', 'mean_divides_by_source_count', 'dt_float_first',
                      'mem_other_reads_mem_self', 'edge_attr_dt_sign', 'gru_r_on_whole_n', 'gru_z_swapped', 'score_skips_channel_C-1',
                      'key_without_edge', 'value_without_edge', 'dropout_inside_normaliser', 'dropout_head_index_dropped', 'scale_missing',
                      'skip_not_added']


def test_mutation_table_is_complete():
    assert set(REQUIRED_MUTATIONS) <= set(ref.MUTATIONS)
    assert set(ref.MUTATIONS['dt_float_first'][0].split('+')) == {'aggregate', 'edge_attr'}


@pytest.mark.parametrize('mutation', sorted(ref.MUTATIONS))
def test_mutation_breaks_the_bound(mutation):
    """Every case in which the mutation can show exceeds its bound (not just one of them)."""
    ratios = _mutation_ratios(mutation)
    assert ratios, 'no case in which the mutation can show'
    kernels = {k[0] for k in ratios}
    assert kernels == set(ref.MUTATIONS[mutation][0].split('+')), kernels
    quiet = {k: v for k, v in ratios.items() if not v > 1.0}
    print(f'[mutation] {mutation}: {len(ratios)} cases, smallest err / bound {min(ratios.values()):.3g}')
    assert not quiet, quiet


# ---------------------------------------------------------------------------------------------------------------------------
# the case builders
# ---------------------------------------------------------------------------------------------------------------------------
def _digest(c, names):
    m = hashlib.sha256()
    for n in names:
        t = c[n].contiguous()
        m.update(n.encode())
        m.update(str(t.dtype).encode())
        m.update(str(tuple(t.shape)).encode())
        m.update(t.numpy().tobytes())
    return m.hexdigest()[:16]


# sha256 (first 16 hex digits) over the tensors the backward tests read, recorded before the builders were extended
AGGR_DIGESTS = {(1, 1, 0): '3a851a32777e1f4e', (1, 100, 172): '1a773d7926978ef1', (64, 1, 0): '1ff7f0a32d12e646', (64, 100, 172): '40236c7b9081d7a5',
                (65, 1, 0): '0b1eed9430abadde', (65, 100, 172): 'e3ba6f4559c88471', (100, 1, 0): '6c9b162abda65f1b', (100, 100, 172): '6f07313534503e96'}
EDGE_DIGESTS = {(1, 1, 0): '42800d523ed419de', (5, 8, 3): '1be5b909cf71f0e9', (37, 100, 172): '967f1d1719401eb3', (41944, 100, 0): '661240122520a63d'}


def test_extended_builders_keep_the_backward_tensors():
    for key, want in AGGR_DIGESTS.items():
        assert _digest(aggr_case(*key), ('lo_s', 'cnt_s', 'lo_d', 'cnt_d', 'lu', 'log_t', 'tw', 'tb', 'd_aggr')) == want, key
    for key, want in EDGE_DIGESTS.items():
        assert _digest(edge_fwd_case(key), ('lu_local', 'src', 't', 'tw', 'tb', 'd_attr')) == want, key
    assert {(T, M, D) for _, T, M, D in ref.AGGR_CASES} <= set(AGGR_DIGESTS) and set(ref.EDGE_CASES + [ref.EDGE_BIG_CASE]) == set(EDGE_DIGESTS)


def test_aggr_case_forward_inputs():
    c = aggr_case(100, 100, 172)
    N, R = c['N'], c['R']
    assert c['nodes'].dtype == torch.int32 and c['nodes'].unique().numel() == R < N and not torch.equal(c['nodes'].long(), torch.arange(R))
    assert c['memory'].shape == (N, 100) and c['log_raw'].shape == (4096, 172) and c['log_other'].dtype == torch.int32
    assert 0 <= int(c['log_other'].min()) and int(c['log_other'].max()) < N
    tab = ref.aggr_tables(c, negative_row=3)
    assert int(tab['nodes'][3]) == int(c['nodes'][3]) - N < 0
    v = c['nodes'].long()
    assert torch.equal(tab['last_update'][v], c['lu']) and torch.equal(tab['st_lo_d'][v], c['lo_d']) and torch.equal(tab['st_cnt_s'][v], c['cnt_s'])
    rest = torch.ones(N, dtype=torch.bool)
    rest[v] = False
    assert not bool((tab['st_cnt_s'][rest] + tab['st_cnt_d'][rest]).any())
    # the three tie rows: the tied events differ in their raw columns (the GPU file tells the winner by them)
    for name in ('tie_one_lane', 'tie_lanes', 'tie_windows'):
        r = ref.AGGR_ROW[name]
        t = c['log_t'][c['walk'](r)]
        i, j = (t.float() == t.float().max()).nonzero()[:, 0].tolist()
        pi, pj = c['walk'](r)[i], c['walk'](r)[j]
        assert not torch.equal(c['log_raw'][pi], c['log_raw'][pj])


def test_edge_fwd_cases():
    c = edge_fwd_case(ref.EDGE_SMALL_LIMIT_CASE)
    arg = ref._fma32((c['lu_local'][c['src']] - c['t']).float(), c['tw'], c['tb'])
    assert c['T'] == 64 and c['D'] == 0 and float(arg.min()) >= 3e6 and float(arg.max()) < 8e6
    c = edge_fwd_case(ref.EDGE_MIXED_WAVE_CASE)
    arg = ref._fma32((c['lu_local'][c['src']] - c['t']).float(), c['tw'], c['tb']).abs()
    big = (arg >= 8e6).any(1).nonzero()[:, 0].tolist()
    assert big == [11] and 64 % (c['T'] + c['D']) == 0 and c['E'] * c['T'] > 64 * 2
    for case in ref.EDGE_CASES:
        c = edge_fwd_case(case)
        assert c['msg'].shape == (c['E'], c['D'])


def test_attend_fwd_case_rows():
    tgt, src, order, seg_lo, seg_hi = ref.attend_fwd_graph()
    U, E = ref.ATTEND_FWD_U, tgt.numel()
    L = (seg_hi - seg_lo).tolist()
    assert L == ref.ATTEND_FWD_COUNTS and E == 5355 and U == 19 and L[0] == 0 == L[-1]
    assert set([0, 1, 2, 3, 4, 5, 16, 17, 64, 65, 255, 256, 257, 300, 1024, 1025, 2049, 12]) == set(L)
    assert not torch.equal(order, torch.arange(E)) and torch.equal(order.sort()[0], torch.arange(E))
    assert torch.equal(ref.edge_targets(order, seg_lo, seg_hi, E), tgt)
    for i in range(U):  # a segment lists its edges in ascending id: what the counting grouping's in-kernel sort restores
        seg = order[int(seg_lo[i]):int(seg_hi[i])]
        assert bool((seg[1:] > seg[:-1]).all())
    assert bool((src[tgt == ref.ATTEND_FWD_HUB_TARGET] == ref.ATTEND_FWD_HUB_SOURCE).all()) and L[ref.ATTEND_FWD_HUB_TARGET] == 2049
    assert bool(((src == tgt) & (tgt == ref.ATTEND_FWD_LOOP)).any())
    assert L[ref.ATTEND_FWD_SPREAD12] == 12 and L[ref.ATTEND_FWD_SPREAD300] == 300
    for H, C, p in [(2, 64, 0.5), (3, 33, 0.1), (2, 132, 0.0)]:
        c = attend_fwd_case(H, C, p)
        s = c['scale'] * ((c['q'].double()[tgt]).view(E, H, C) * (c['k'].double()[src] + c['eproj'].double()).view(E, H, C)).sum(-1)
        for t_ in (ref.ATTEND_FWD_SPREAD12, ref.ATTEND_FWD_SPREAD300):
            sp = (tgt == t_).nonzero()[:, 0]
            assert float((s[sp].max(0)[0] - s[sp].min(0)[0]).min()) > 100.0
            assert bool((torch.exp((s[sp] - s[sp].max(0)[0]).float()) == 0).any(0).all()), 'float32 expf must underflow to exactly 0'
        sp = (tgt == ref.ATTEND_FWD_SPREAD300).nonzero()[:, 0]
        weak = torch.arange(300) % 4 == ref.ATTEND_FWD_WEAK_WAVE
        gap = s[sp][~weak].max(0)[0] - s[sp][weak].max(0)[0]
        assert float(gap.min()) > 104.0, 'one wave\'s whole share must lie below exp\'s float32 range under the others\' maximum'
        if p == 0.5:
            dropped = torch.zeros(U, H).index_add_(0, tgt, (c['keep'] != 0).float()) == 0
            assert bool(dropped[1, 0]) and L[1] == 1
        if p:
            assert 0 < int((c['keep'] == 0).sum()) < c['keep'].numel()


@pytest.mark.parametrize('H,C', [(2, 64), (2, 50), (3, 33), (2, 132), (2, 4)])
def test_attend_bound_sees_a_lost_last_edge(H, C):
    """The last position of the 5-, 17-, 65-, 257-, 1025- and 2049-edge segments (one past a block of four, past the one-wave walk,
    alone in a wave's next trip) carries a heavy weight: a walk that loses that one edge -- here: its keep set to 0 -- leaves the
    bound at that target, and at no other."""
    c = attend_fwd_case(H, C, 0.0)
    want, bound = attend_bounds(H, C, 0.0)
    L = ref.ATTEND_FWD_COUNTS
    assert [L[t] for t in ref.ATTEND_FWD_HEAVY_LAST] == [5, 17, 65, 257, 1025, 2049]
    for t_, e in zip(ref.ATTEND_FWD_HEAVY_LAST, c['heavy']):
        assert int(c['tgt'][e]) == t_ and int(c['order'][int(c['seg_hi'][t_]) - 1]) == e
        keep = c['keep'].clone()
        keep[e] = 0.0
        args = list(ref.attend_args(c))
        args[-1] = keep
        got = ref.attend(*args)[0]
        ratio = ((got - want).abs() / bound).max(1)[0]
        assert float(ratio[t_]) > 1.0 and float(ratio.sum() - ratio[t_]) == 0.0, (t_, float(ratio[t_]))


def test_attend_walk_table():
    """The walk every width reaches, by tconv_short_ok's rule, with every operand on the 16-byte grid; and the (2, 8) alignment trio."""
    for (H, C), walk in ref.ATTEND_FWD_WIDTHS.items():
        assert ref.tconv_walk(H, C, 0x1000) == walk, (H, C)
    assert sorted(C // 4 for (H, C), w in ref.ATTEND_FWD_WIDTHS.items() if w == 4) == [1, 16, 32]  # lanes on: one, half, all 32
    assert sorted(C // 2 for (H, C), w in ref.ATTEND_FWD_WIDTHS.items() if w == 2) == [1, 25, 31]
    trips = {(H, C): -(-C // 64) for (H, C), w in ref.ATTEND_FWD_WIDTHS.items() if w == 0}
    assert trips[2, 65] == 2 and trips[2, 132] == 3 and trips[3, 70] == 2 and trips[2, 3] == 1
    H, C = ref.ATTEND_FWD_ALIGN
    assert [ref.tconv_walk(H, C, 0x1000, 0x1000 + off) for off in (0, 8, 4)] == [4, 2, 0]
