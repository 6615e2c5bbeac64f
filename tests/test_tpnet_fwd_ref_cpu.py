"""``oracle/tpnet_fwd_ref.py`` judged on the CPU, before a device result is judged by it (tests/test_tpnet_blocks_gpu.py):

* in float64 every restatement equals ``tests/tpnet_restate.py`` to 1e-10 on the g17 inputs (``rp_update`` batch by batch, ``rp_features``,
  ``tpnet_tokens`` fed the fixture's pair-MLP output as ``pf``) and reproduces every ``g17_tpnet_update_*`` / ``g17_tpnet_pair_*`` fixture
  within the bars of ``tests/test_tpnet_cpu.py``;
* for every shared case, the BIG ones included, the float32 evaluation of the restatement (messages added in contribution order) stays
  within its own bound: the bounds hold for correct arithmetic (``pytest -rP`` prints the worst ratio per kernel);
* every entry of ``MUTATIONS`` exceeds the bound at the case the table names;
* a row with exactly three contributions that loses the last one exceeds the bound (a hub's bound grows with its count: the
  sensitivity claim does not rest on the hub);
* the exact cases are integers, and the same integers, in float64 and in float32.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import tpnet_restate as tr
from golden_util import load
from oracle import tpnet_fwd_ref as ref
from oracle.tgat_bwd_ref import F64, worst_ratio
from test_tpnet_cpu import ENCODER_CASES, NOISE, PAIR_CASES, UPDATE_CASES, encoder_inputs, fixture_state_dict

F32 = torch.float32
PIN = 1e-10


def _update(c, dtype, mutate):
    new, bounds = ref.update_bounds(c, dtype, mutate)
    return {f'P{i}': (new[i], bounds[i]) for i in range(len(new))}


def _pair(c, dtype, mutate):
    return {'out': ref.pair_bounds(c, dtype, mutate)}


def _tokens(c, dtype, mutate):
    out, bound, lg = ref.token_run(c, dtype, mutate)
    return {'out': (out, bound), 'lg': (lg, torch.zeros_like(lg))}


def _mean(c, dtype, mutate):
    return {'out': ref.mean_bounds(c, dtype, mutate)}


# kind -> (cases, case builder, evaluation -> {output name: (value, bound)})
KINDS = {
    'update': (ref.UPDATE_CASES + ref.UPDATE_EXACT_CASES + [ref.UPDATE_BIG_CASE], ref.update_case, _update),
    'pair': (ref.PAIR_CASES + [ref.PAIR_BIG_CASE], lambda *c: ref.pair_case(*c, items=65539 if c == ref.PAIR_BIG_CASE else None), _pair),
    'tokens': (ref.TOKEN_CASES + [ref.TOKEN_BIG_CASE], ref.token_case, _tokens),
    'mean': (ref.MEAN_CASES + [ref.MEAN_BIG_CASE], ref.mean_case, _mean),
}
ALL = [(kind, case) for kind, spec in KINDS.items() for case in spec[0]]
WORST = {}


@functools.lru_cache(maxsize=None)
def _case(kind, case):
    return KINDS[kind][1](*case)


@functools.lru_cache(maxsize=None)
def _want(kind, case):
    return KINDS[kind][2](_case(kind, case), F64, None)


def _worst(kind, case, dtype, mutate):
    """Worst err / bound of an evaluation against the float64 value and its bound (a non-finite result counts as inf)."""
    got = KINDS[kind][2](_case(kind, case), dtype, mutate)
    worst = 0.0
    for name, (want, bound) in _want(kind, case).items():
        g = got[name][0].double()
        r = worst_ratio(g, want, bound) if bool(torch.isfinite(g).all()) else math.inf
        worst = max(worst, r if r == r else math.inf)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# the restatements against tests/tpnet_restate.py and the reference fixtures, float64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', UPDATE_CASES)
def test_update_is_the_restatement_and_reproduces_the_fixture(name):
    meta, a = load(name)
    cfg = meta['cfg']
    N, L = cfg['num_nodes'], cfg['num_layer']
    p0 = torch.from_numpy(a['p0'])
    tabs = [p0.double()] + [torch.zeros_like(p0, dtype=F64) for _ in range(L)]
    mine, now, now2, worst = list(tabs), cfg['beginning_time'], cfg['beginning_time'], 0.0
    T = torch.from_numpy
    for b in range(a['src'].shape[0]):
        tabs, now = tr.rp_update(tabs, now, a['src'][b], a['dst'][b], a['time'][b], cfg['lam'])
        mine, _, _, now2 = ref.rp_update(mine, now2, T(a['src'][b]), T(a['dst'][b]), T(a['time'][b]), cfg['lam'], N)
        worst = max([worst] + [tr.rel_err(mine[i], tabs[i]) for i in range(L + 1)])
    assert now2 == now == meta['now'] and worst <= PIN
    assert torch.equal(mine[0], p0.double())
    err = max(tr.rel_err(T(a[f'table_{i}']), mine[i]) for i in range(1, L + 1))
    noise = NOISE['fixtures'][name]
    print(f'[tpnet blocks] {name}: oracle vs restatement {worst:.2e}; reference float32 vs oracle {err:.3e} (recorded {noise:.3e})')
    assert err < 1e-5 and abs(err - noise) <= 1e-9 + 1e-3 * noise


@pytest.mark.parametrize('name', PAIR_CASES)
def test_pair_features_are_the_restatement_and_reproduce_the_fixture(name):
    meta, a = load(name)
    cfg = meta['cfg']
    sd = fixture_state_dict(meta, a)
    tabs = [sd[f'random_projections.{i}'] for i in range(cfg['num_layer'] + 1)]
    concat, scale = cfg.get('concat', True), cfg.get('scale', True)
    ia, ib = torch.from_numpy(a['a']).reshape(-1), torch.from_numpy(a['b']).reshape(-1)
    n = ia.numel()
    f, mag = ref.pair_features(tabs, ia, None, n, 1, ib, None, n, n, concat, scale)
    assert tr.rel_err(f, tr.rp_features(tabs, a['a'], a['b'], concat, scale)) <= PIN
    raw, _ = ref.pair_features(tabs, ia, None, n, 1, ib, None, n, n, concat, False)
    assert bool((mag >= raw.abs() * (1 - 1e-12)).all())
    g = lambda k: sd[k].double()
    out = F.linear(F.relu(F.linear(f, g('mlp.0.weight'), g('mlp.0.bias'))), g('mlp.2.weight'), g('mlp.2.bias'))
    err = tr.rel_err(torch.from_numpy(a['out']), out)
    noise = NOISE['fixtures'][name]
    print(f'[tpnet blocks] {name}: reference float32 vs oracle + MLP {err:.3e} (recorded {noise:.3e})')
    assert err < 1e-5 and abs(err - noise) <= 1e-9 + 1e-3 * noise


@pytest.mark.parametrize('name', ENCODER_CASES)
def test_tokens_are_the_restatement(name):
    meta, a = load(name)
    sd = fixture_state_dict(meta, a)
    i = encoder_inputs(a)
    cfg = meta['cfg']
    rp = None if cfg is None else dict(num_layer=cfg['num_layer'], concat=cfg.get('concat', True), scale=cfg.get('scale', True))
    want = tr.tpnet_tokens(sd, rp, **i)
    Q, k, W = want.shape
    B = Q // 2
    pf, od = None, 0
    if rp is not None:
        flat = i['nbr_nids'][:Q].long().reshape(-1)
        blocks = []
        for ends in (i['src'], i['dst']):
            e2 = ends.long().reshape(-1).repeat(2).repeat_interleave(k)
            blocks.append(tr.rp_forward(sd, 'random_projections.', rp['num_layer'], flat, e2, rp['concat'], rp['scale']))
        pf, od = torch.cat(blocks), blocks[0].shape[1]
    dN, dE, dT = i['node_x'].shape[1], i['nbr_edge_x'].shape[2], sd['time_encoder.w.bias'].numel()
    out, bound, lg = ref.tokens(i['node_x'], i['node_x'].shape[0], dN, i['edge_time'], B, i['nbr_nids'].int(), i['nbr_time'], i['nbr_edge_x'], Q, k, dE,
                                None, sd['time_encoder.w.weight'].reshape(-1), sd['time_encoder.w.bias'], dT, pf, od, W + 2)
    assert tr.rel_err(out[:, :W], want.reshape(Q * k, W)) <= PIN and not bool(out[:, W:].any())
    pad = (i['nbr_nids'][:Q] == -1).reshape(-1)
    assert bool((lg[pad] == -1).all()) and bool((lg[~pad] >= 0).all()) and not bool(bound[pad].any())


@pytest.mark.parametrize('case', ref.TOKEN_CASES, ids=str)
def test_token_cases_hold_what_they_promise_and_their_zeros_are_positive(case):
    """The kernel stores 0.f for a structural zero; the device test compares bits, so the restatement must not hand it a -0.0."""
    c = _case('tokens', case)
    out, bound, lg = ref.token_run(c)
    assert not bool(torch.signbit(out[out == 0]).any()) and not bool(torch.signbit(ref.token_run(c, F32)[0][out == 0]).any())
    Q, k = 2 * c['B'], c['k']
    assert bool((lg.view(Q, k) == -1).all(1).any()) and bool((c['nids'][0] >= c['N']).any()) and bool((lg == 0).any())
    assert abs(float(lg.max()) - math.log(2.0 ** (31 if k >= 4 else 24))) < 1e-6, 'the largest gap of GAPS that k admits'
    assert not bool(bound[:, : c['dN']].any()) and not bool(bound[:, c['dN'] + c['dT']:].any())


@pytest.mark.parametrize('Q,k,C', ref.MEAN_CASES)
def test_mean_is_torchs(Q, k, C):
    c = ref.mean_case(Q, k, C)
    v, mag = ref.token_mean(c['z'], k)
    assert tr.rel_err(v, c['z'].double().view(Q, k, C).mean(1)) <= 1e-14 and bool((mag >= v.abs() * (1 - 1e-12)).all())


# ---------------------------------------------------------------------------------------------------------------------------
# the reference alone meets the bounds; the mutations do not
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,case', ALL, ids=str)
def test_float32_evaluation_stays_within_the_bound(kind, case):
    worst = _worst(kind, case, F32, None)
    WORST[kind] = max(WORST.get(kind, 0.0), worst)
    print(f'[tpnet blocks] {kind} {case}: float32 restatement at {worst:.4f}x the bound (worst {kind} so far {WORST[kind]:.4f})')
    assert worst <= 1.0


def test_worst_float32_ratio_per_kernel():
    worst = {kind: max(_worst(kind, case, F32, None) for case in spec[0]) for kind, spec in KINDS.items()}
    print('[tpnet blocks] float32 restatement, worst err / bound per kernel: ' + ', '.join(f'{k} {v:.4f}' for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values())


@pytest.mark.parametrize('name', sorted(ref.MUTATIONS))
def test_every_mutation_exceeds_the_bound_at_its_case(name):
    kind, case = ref.MUTATIONS[name]
    assert case in KINDS[kind][0], 'the named case is a listed one'
    worst = _worst(kind, case, F64, name)
    print(f'[tpnet blocks] {name}: {worst:.3g}x the bound at {kind} {case}')
    assert worst > 1.0


def test_a_row_of_three_contributions_that_loses_its_last_exceeds_the_bound():
    c = ref.three_contribution_case()
    want, bounds = ref.update_bounds(c)
    _, _, count, _ = ref.rp_update(c['tables'], c['now'], c['src'], c['dst'], c['time'], c['lam'], c['N'])
    assert int(count[c['row']]) == 3 and int(c['dst'][-1]) == c['row']
    f32, _ = ref.update_bounds(c, F32)
    lost, _ = ref.update_bounds(c, F64, 'update_lost_last')
    ok, bad = worst_ratio(f32[1].double(), want[1], bounds[1]), worst_ratio(lost[1][c['row']], want[1][c['row']], bounds[1][c['row']])
    print(f'[tpnet blocks] three contributions: float32 at {ok:.4f}x the bound, the last one lost at {bad:.3g}x')
    assert ok <= 1.0 < bad
    others = torch.arange(c['N']) != c['row']
    assert torch.equal(lost[1][others], want[1][others])


@pytest.mark.parametrize('case', ref.UPDATE_EXACT_CASES + [ref.UPDATE_BIG_CASE], ids=str)
def test_exact_cases_are_integers_in_both_precisions(case):
    c = _case('update', case)
    new64, new32 = ref.rp_update(c['tables'], c['now'], c['src'], c['dst'], c['time'], c['lam'], c['N'])[0], \
        ref.rp_update(c['tables'], c['now'], c['src'], c['dst'], c['time'], c['lam'], c['N'], F32)[0]
    for i, (p, q) in enumerate(zip(new64, new32)):
        assert torch.equal(p, p.round()) and float(p.abs().max()) < 2 ** 24 and q.dtype == F32 and torch.equal(q.double(), p), i
    assert any(not torch.equal(new64[i], c['tables'][i].double()) for i in range(1, len(new64)))
