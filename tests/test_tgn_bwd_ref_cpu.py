"""Keeps ``oracle/tgn_bwd_ref.py`` honest without a GPU: the float64 restatements that ``tests/test_tgn_bwd_blocks_gpu.py`` holds the
four kernels of ``csrc/tgn_bwd.hip`` against

* equal torch float64 autograd through the forward formula (1e-10 relative): ``TGNMemoryRef._gru``, Time2Vec of the selected /
  averaged events, ``transformer_conv_ref`` given q, k, v, e and the keep mask -- on every case of the shared tables,
* come with bounds ``n * 2^-24 * magnitude`` that a float32 evaluation of the same formulas meets with a factor two to spare,
* lose to every listed mutation on every case in which it can show, and
* are fed by case builders that contain the row kinds they claim.
"""
import functools

import pytest
import torch

from oracle import tgat_ref
from oracle import tgn_bwd_ref as ref
from oracle.tgat_bwd_ref import EPS, worst_ratio
from oracle.tgn_ref import TGNMemoryRef, transformer_conv_ref

F64 = torch.float64
F32 = torch.float32


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp(min=1e-300))


gru_case = functools.lru_cache(maxsize=None)(ref.gru_case)
aggr_case = functools.lru_cache(maxsize=None)(ref.aggr_case)
edge_case = functools.lru_cache(maxsize=None)(ref.edge_case)
attend_case = functools.lru_cache(maxsize=None)(ref.attend_case)


# ---------------------------------------------------------------------------------------------------------------------------
# bounds (shared with the GPU file's arithmetic: n * EPS * magnitude, per kernel)
# ---------------------------------------------------------------------------------------------------------------------------
def gru_ratio(c, got):
    want, bound = ref.gru_bounds(c)
    return max(worst_ratio(got[0], want[0], bound[0]), worst_ratio(got[1], want[1], bound[1]))


def aggr_ratio(c, mean, got):
    return worst_ratio(got, *ref.aggr_bounds(c, mean))


def edge_ratio(c, got):
    return worst_ratio(got, *ref.edge_bounds(c))


def attend_ratios(c, got):
    want, bound = ref.attend_bounds(c)
    return {name: worst_ratio(got[name], want[name], bound[name]) for name in bound}


# ---------------------------------------------------------------------------------------------------------------------------
# the restatements equal autograd
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R,M', ref.GRU_CASES)
def test_gru_gate_backward_equals_autograd(R, M):
    """Through ``TGNMemoryRef._gru`` itself: W_ih = I (x = gi), W_hh = 0 and a per-row 'bias' gh (h reaches the output only
    through z h: a buffer row)."""
    c = gru_case(R, M)
    gi, gh = (c[n].double().clone().requires_grad_(True) for n in ('gi', 'gh'))
    p = {'memory_updater.weight_ih': torch.eye(3 * M, dtype=F64), 'memory_updater.bias_ih': torch.zeros(3 * M, dtype=F64),
         'memory_updater.weight_hh': torch.zeros(3 * M, M, dtype=F64), 'memory_updater.bias_hh': gh}
    out = TGNMemoryRef(1, 0, M, 1, p)._gru(gi, c['h'].double())
    (out * c['dout'].double()).sum().backward()
    dgi, dgh, _, _ = ref.gru_gate_backward(c['gi'], c['gh'], c['h'], c['dout'])
    assert _rel(dgi, gi.grad) <= 1e-10 and _rel(dgh, gh.grad) <= 1e-10


def _time2vec_at_rounded_argument(dt32, tw, tb, tw0, tb0):
    """Time2Vec in float64 around the float32-rounded argument the kernels (and tgat_ref.time2vec) evaluate at: autograd cannot
    see a rounding, so the argument is arg32 + dt (tw - tw0) + (tb - tb0) -- at tw = tw0, tb = tb0 the value is cos(arg32), the
    gradient -sin(arg32) dt | -sin(arg32)."""
    arg32 = (dt32.double()[:, None] * tw0.double() + tb0.double()).float()
    return torch.cos(arg32.double() + dt32.double()[:, None] * (tw - tw0.double()) + (tb - tb0.double()))


@pytest.mark.parametrize('mean,T,M,D', ref.AGGR_CASES)
def test_aggregate_backward_equals_autograd(mean, T, M, D):
    """Forward: per row the walk (source window, then destination window), Time2Vec(t - lu) of the event torch.argmax(t.float())
    picks (LAST) or of all, averaged (MEAN), as in ``TGNMemoryRef._updated``; loss = sum of the row times d_aggr's time columns."""
    c = aggr_case(T, M, D)
    tw, tb = (c[n].double().clone().requires_grad_(True) for n in ('tw', 'tb'))
    toff, loss = 2 * M + D, 0.0
    for r in range(c['R']):
        pos = c['walk'](r)
        if pos.numel() == 0:
            continue
        t = c['log_t'][pos]
        dt32 = (t - c['lu'][r]).float()
        enc = _time2vec_at_rounded_argument(dt32, tw, tb, c['tw'], c['tb'])
        assert float((enc.detach() - tgat_ref.time2vec(t - c['lu'][r], c['tw'][:, None], c['tb']).double()).abs().max()) <= 1e-6
        row = enc.mean(0) if mean else enc[int(torch.argmax(t.float()))]
        loss = loss + (row * c['d_aggr'][r, toff:toff + T].double()).sum()
    loss.backward()
    part, _ = ref.aggregate_backward(*ref.aggr_args(c, mean))
    assert _rel(part[:, :T].sum(0), tw.grad) <= 1e-10 and _rel(part[:, T:].sum(0), tb.grad) <= 1e-10
    empty = (c['cnt_s'] + c['cnt_d']) == 0
    assert torch.equal(part[empty], torch.zeros(int(empty.sum()), 2 * T, dtype=F64))


@pytest.mark.parametrize('E,T,D', ref.EDGE_CASES)
def test_edge_attr_backward_equals_autograd(E, T, D):
    c = edge_case(E, T, D)
    tw, tb = (c[n].double().clone().requires_grad_(True) for n in ('tw', 'tb'))
    dt32 = (c['lu_local'][c['src']] - c['t']).float()
    enc = _time2vec_at_rounded_argument(dt32, tw, tb, c['tw'], c['tb'])
    (enc * c['d_attr'][:, :T].double()).sum().backward()
    part, _ = ref.edge_attr_backward(c['lu_local'], c['src'], c['t'], c['tw'], c['tb'], c['d_attr'], D)
    assert _rel(part[:, :T].sum(0), tw.grad) <= 1e-10 and _rel(part[:, T:].sum(0), tb.grad) <= 1e-10


@pytest.mark.parametrize('H,C,p', ref.ATTEND_CASES)
def test_attend_backward_equals_autograd(H, C, p):
    """Through ``transformer_conv_ref`` itself: x = [q | k | v] with selector weights, lin_edge = I, lin_skip = 0, and its own
    dropout mask from (p, seed, stream) -- the keep the case carries."""
    c = attend_case(H, C, p)
    HC, U = H * C, c['U']
    q, k, v, e = (c[n].double().clone().requires_grad_(True) for n in ('q', 'k', 'v', 'eproj'))
    sel = lambda i: torch.eye(3 * HC, dtype=F64)[i * HC:(i + 1) * HC]
    prm = {'lin_query.weight': sel(0), 'lin_key.weight': sel(1), 'lin_value.weight': sel(2), 'lin_edge.weight': torch.eye(HC, dtype=F64),
           'lin_skip.weight': torch.zeros(HC, 3 * HC, dtype=F64)}
    out = transformer_conv_ref(prm, '', H, torch.cat([q, k, v], 1), torch.stack([c['src'], c['tgt']]), e,
                               dropout=(p, ref.DROP_SEED, c['stream']) if p else None)
    (out * c['dout'].double()).sum().backward()
    got = ref.attend_backward(*ref.attend_args(c))
    for name, want in (('dq', q.grad), ('dk', k.grad), ('dv', v.grad), ('de', e.grad)):
        assert _rel(got[name], want) <= 1e-10, name
    none = c['seg_hi'] == c['seg_lo']
    assert torch.equal(got['dq'][none], torch.zeros(int(none.sum()), HC, dtype=F64))


# ---------------------------------------------------------------------------------------------------------------------------
# the bounds leave room for float32: the same formulas in float32 stay within half of each
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R,M', ref.GRU_CASES)
def test_gru_gate_backward_float32_within_half_the_bound(R, M):
    c = gru_case(R, M)
    got = ref.gru_gate_backward(c['gi'], c['gh'], c['h'], c['dout'], dtype=F32)
    assert all(bool(torch.isfinite(t).all()) for t in got[:2])
    w = gru_ratio(c, got)
    print(f'[float32] gru {(R, M)}: {w:.3f}')
    assert w <= 0.5


@pytest.mark.parametrize('mean,T,M,D', ref.AGGR_CASES)
def test_aggregate_backward_float32_within_half_the_bound(mean, T, M, D):
    c = aggr_case(T, M, D)
    w = aggr_ratio(c, mean, ref.aggregate_backward(*ref.aggr_args(c, mean), dtype=F32)[0])
    print(f'[float32] aggregate {(mean, T, M, D)}: {w:.3f}')
    assert w <= 0.5


@pytest.mark.parametrize('E,T,D', ref.EDGE_CASES)
def test_edge_attr_backward_float32_within_half_the_bound(E, T, D):
    c = edge_case(E, T, D)
    w = edge_ratio(c, ref.edge_attr_backward(c['lu_local'], c['src'], c['t'], c['tw'], c['tb'], c['d_attr'], D, dtype=F32)[0])
    print(f'[float32] edge_attr {(E, T, D)}: {w:.3f}')
    assert w <= 0.5


@pytest.mark.parametrize('H,C,p', ref.ATTEND_CASES)
def test_attend_backward_float32_within_half_the_bound(H, C, p):
    c = attend_case(H, C, p)
    ratios = attend_ratios(c, ref.attend_backward(*ref.attend_args(c), dtype=F32))
    print(f'[float32] attend {(H, C, p)}: ' + ', '.join(f'{n} {v:.3f}' for n, v in ratios.items()))
    assert max(ratios.values()) <= 0.5, ratios


# ---------------------------------------------------------------------------------------------------------------------------
# the bounds notice what they must
# ---------------------------------------------------------------------------------------------------------------------------
def _mutations(kernel, **info):
    return [m for m, (where, applies) in ref.MUTATIONS.items() if kernel in where.split('+') and applies(**info)]


def test_every_listed_mutation_is_exercised():
    seen = {m for R, M in ref.GRU_CASES for m in _mutations('gru')}
    seen |= {m for mean, T, M, D in ref.AGGR_CASES for m in _mutations('aggregate', mean=mean)}
    seen |= {m for _ in ref.EDGE_CASES for m in _mutations('edge_attr')}
    seen |= {m for H, C, p in ref.ATTEND_CASES for m in _mutations('attend', H=H, p=p)}
    assert seen == set(ref.MUTATIONS)


@pytest.mark.parametrize('case,mutation', [(c, m) for c in ref.GRU_CASES for m in _mutations('gru')], ids=str)
def test_gru_mutations_break_the_bound(case, mutation):
    c = gru_case(*case)
    assert gru_ratio(c, ref.gru_gate_backward(c['gi'], c['gh'], c['h'], c['dout'], mutate=mutation)) > 1.0


@pytest.mark.parametrize('case,mutation', [(c, m) for c in ref.AGGR_CASES for m in _mutations('aggregate', mean=c[0])], ids=str)
def test_aggregate_mutations_break_the_bound(case, mutation):
    mean, T, M, D = case
    c = aggr_case(T, M, D)
    assert aggr_ratio(c, mean, ref.aggregate_backward(*ref.aggr_args(c, mean), mutate=mutation)[0]) > 1.0


@pytest.mark.parametrize('case,mutation', [(c, m) for c in ref.EDGE_CASES for m in _mutations('edge_attr')], ids=str)
def test_edge_attr_mutations_break_the_bound(case, mutation):
    c = edge_case(*case)
    got = ref.edge_attr_backward(c['lu_local'], c['src'], c['t'], c['tw'], c['tb'], c['d_attr'], c['D'], mutate=mutation)[0]
    assert edge_ratio(c, got) > 1.0


@pytest.mark.parametrize('case,mutation', [(c, m) for c in ref.ATTEND_CASES for m in _mutations('attend', H=c[0], p=c[2])], ids=str)
def test_attend_mutations_break_the_bound(case, mutation):
    c = attend_case(*case)
    ratios = attend_ratios(c, ref.attend_backward(*ref.attend_args(c), mutate=mutation))
    assert max(ratios.values()) > 1.0, ratios


# ---------------------------------------------------------------------------------------------------------------------------
# the case builders contain the row kinds they claim
# ---------------------------------------------------------------------------------------------------------------------------
def test_case_tables_cover_every_axis_value():
    assert {c[1] for c in ref.AGGR_CASES} == set(ref.T2V_AXES['T']) and {c[2:] for c in ref.AGGR_CASES} == set(ref.T2V_AXES['MD'])
    for T in ref.T2V_AXES['T']:
        assert {c[0] for c in ref.AGGR_CASES if c[1] == T} == {0, 1}
    for MD in ref.T2V_AXES['MD']:
        assert {c[0] for c in ref.AGGR_CASES if c[2:] == MD} == {0, 1}
    for i, axis in enumerate(('H', 'C', 'p')):
        assert {c[i] for c in ref.ATTEND_CASES} == set(ref.ATTEND_AXES[axis])
    for big, threads in ((ref.GRU_BIG_CASE, ref.GRU_BIG_CASE[0] * ref.GRU_BIG_CASE[1]), (ref.EDGE_BIG_CASE, ref.EDGE_BIG_CASE[0] * ref.EDGE_BIG_CASE[1])):
        assert threads == 16384 * 256 + 96, big


@pytest.mark.parametrize('R,M', ref.GRU_CASES[1:])
def test_gru_case_rows(R, M):
    c = gru_case(R, M)
    pre = (c['gi'] + c['gh'])[c['band']][:, :2 * M]
    assert len(c['band']) >= 1 and {float(x) for x in pre.unique()} <= set(ref.GRU_BAND)
    if M >= 4:
        assert {float(x) for x in pre.unique()} == set(ref.GRU_BAND)
    assert float(torch.exp(torch.tensor(95.0))) == float('inf')  # float32 expf overflows there
    r = c['hn_row']
    n = torch.tanh(c['gi'][r, 2 * M:].double() + torch.sigmoid((c['gi'][r, :M] + c['gh'][r, :M]).double()) * c['gh'][r, 2 * M:].double())
    assert float((c['h'][r].double() - n).abs().max()) <= EPS and r not in c['band']


def test_aggr_case_rows():
    c = aggr_case(8, 1, 0)
    K, cs, cd = ref.AGGR_ROW, c['cnt_s'], c['cnt_d']
    tot = (cs + cd).tolist()
    assert c['R'] == 23 and c['R'] % 4 != 0 and c['log_t'].numel() == 4096
    assert tot[K['empty']] == 0 and tot[K['empty_last']] == 0 and tot[K['one']] == 1
    assert cs[K['src_only']] > 0 and cd[K['src_only']] == 0 and cs[K['dst_only']] == 0 < cd[K['dst_only']]
    r = K['dst_below_src']
    assert cs[r] > 0 and cd[r] > 0 and c['lo_d'][r] + cd[r] <= c['lo_s'][r]
    assert (tot[K['total64']], tot[K['total65']], tot[K['total130']]) == (64, 65, 130)
    assert cs[K['dst_only_70']] == 0 and cd[K['dst_only_70']] > 64
    # no two windows share a log position
    used = torch.cat([c['walk'](r) for r in range(c['R'])])
    assert used.unique().numel() == used.numel() and int(used.max()) < 4096 and int(used.min()) > 0
    for r, idx in ((K['max_first'], 0), (K['max_last'], 129), (K['max_127'], 127)):
        f = c['log_t'][c['walk'](r)].float()
        assert tot[r] == 130 and int(torch.argmax(f)) == idx and int((f == f.max()).sum()) == 1
    for r, (i, j) in ((K['tie_one_lane'], (5, 69)), (K['tie_lanes'], (10, 20)), (K['tie_windows'], (7, 43))):
        t = c['log_t'][c['walk'](r)]
        f = t.float()
        assert (f == f.max()).nonzero()[:, 0].tolist() == [i, j] and int(t.min()) > 2 ** 24
        assert int(torch.argmax(f)) == i and int(torch.argmax(t)) == j, 'the int64 argmax must break the tie differently'
        dt = (t[[i, j]] - c['lu'][r]).float()
        assert float(dt[0]) != float(dt[1]), 'the tied events need different dt'
    r = K['tie_windows']
    assert 7 < cs[r] <= 43
    r = K['dt_zero']
    assert int(c['log_t'][c['walk'](r)][0] - c['lu'][r]) == 0
    dt = (c['log_t'][c['walk'](K['dt_2_31'])] - c['lu'][K['dt_2_31']])
    assert int(dt.max()) == 2 ** 31 - 1
    c100 = aggr_case(100, 100, 172)
    assert abs(float(c100['tw'][0]) - 1.0) < 1e-6 and abs(float(c100['tw'][-1]) - 1e-9) < 1e-12
    assert bool(torch.isnan(c100['d_aggr'][:, :372]).all()) and bool(torch.isfinite(c100['d_aggr'][:, 372:]).all())


def test_edge_case_rows():
    for E, T, D in ref.EDGE_CASES + [ref.EDGE_BIG_CASE]:
        c = edge_case(E, T, D)
        assert c['lu_local'].numel() == (1 if E <= 5 else 17)
        if E > 1:
            assert c['src'].unique().numel() < E, 'src must repeat'
        diff = c['lu_local'][c['src']] - c['t']
        assert int(c['lu_local'].min()) > 2 ** 30 and bool(torch.isnan(c['d_attr'][:, T:]).all())
        if E >= 5:
            assert diff[:3].tolist() == [0, 2 ** 31 - 3, -(2 ** 31 - 7)] and int(diff[3:].abs().max()) <= 40
            wrong = c['lu_local'][c['src']].float() - c['t'].float()
            assert float((wrong - diff.float()).abs().max()) >= 32, 'float-first must be visibly off'


@pytest.mark.parametrize('H,C,p', ref.ATTEND_CASES)
def test_attend_case_rows(H, C, p):
    c = attend_case(H, C, p)
    U, E, tgt, src = c['U'], c['E'], c['tgt'], c['src']
    assert U == 11 and U % 4 != 0
    L = (c['seg_hi'] - c['seg_lo']).tolist()
    assert L == ref.ATTEND_COUNTS and {0, 1, 2, 64, 65, 300} <= set(L) and L[U - 1] == 0
    assert not torch.equal(c['order'], torch.arange(E)) and torch.equal(c['order'].sort()[0], torch.arange(E))
    assert torch.equal(ref.edge_targets(c['order'], c['seg_lo'], c['seg_hi'], E), tgt)
    hub = src == ref.ATTEND_HUB_SOURCE
    assert int((hub & (tgt == ref.ATTEND_HUB_TARGET)).sum()) == 300 and tgt[hub].unique().numel() >= 4
    assert bool(((src == tgt) & (tgt == ref.ATTEND_LOOP)).any())
    s = c['scale'] * ((c['q'].double()[tgt]).view(E, H, C) * (c['k'].double()[src] + c['eproj'].double()).view(E, H, C)).sum(-1)
    sp = tgt == ref.ATTEND_SPREAD_TARGET
    assert float((s[sp].max(0)[0] - s[sp].min(0)[0]).min()) > 100.0
    a32 = torch.exp((s[sp] - s[sp].max(0)[0]).float())
    assert bool((a32 == 0).any(0).all()), 'float32 expf must underflow to exactly 0 for the weak edges of every head'
    if p:
        inv = float(torch.tensor(1.0 / (1.0 - float(torch.tensor(p, dtype=F32))), dtype=F64).float())
        assert bool(((c['keep'] == 0) | (c['keep'] == inv)).all()) and 0 < int((c['keep'] == 0).sum()) < c['keep'].numel()
    else:
        assert bool((c['keep'] == 1).all())
    if p == 0.5:
        all_dropped = torch.zeros(U, H).index_add_(0, tgt, (c['keep'] != 0).float()) == 0
        has_edges = torch.tensor(L)[:, None] > 0
        assert bool((all_dropped & has_edges).any()), 'a (target, head) with every edge dropped'
