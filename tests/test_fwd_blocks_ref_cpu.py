"""``oracle/fwd_blocks_ref.py`` judged on the CPU, before a device result is judged by it (tests/test_mixer_blocks_gpu.py,
tests/test_dygformer_blocks_gpu.py):

* every restatement agrees with torch in float64 to 1e-12 (``F.layer_norm``, ``F.gelu``, ``scaled_dot_product_attention`` on the packed
  qkv layout) and, composed end to end, with ``tests/graphmixer_restate.py`` and ``tests/dygformer_restate.py``;
* for every shared case the float32 evaluation of the restatement stays within the bound ``n * 2^-24 * magnitude``: the reference
  alone meets the bar (``pytest -rP`` prints the worst err / bound);
* every entry of ``MUTATIONS`` exceeds the bound at one case at least, and at no case where its condition says it cannot show;
* the ``kRefine`` claim of ``csrc/mixer.hip`` -- the corrected mean of K equal float32 values is that value bit for bit -- holds in
  float32 emulation for K in {3, 5, 7, 20, 30} and the values of ``CONSTANTS`` (0.1, 1/3, 1e6 + 0.1, -7.3e-5 among them), while the
  plain mean is off for some of them.  No value was found where the claim fails.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dygformer_restate as dr
import graphmixer_restate as gr
from oracle import fwd_blocks_ref as ref
from oracle.tgat_bwd_ref import EPS, F64, worst_ratio

F32 = torch.float32
PIN = 1e-12


# Time2Vec frequencies 2^-j with a zero phase: dt * tw is exact in float32, so the restatements' float32 argument (one fma, as the kernels
# have it) is the float64 argument of tests/*_restate.py and the composed results agree to rounding in float64
EXACT_TW = lambda T: 2.0 ** -torch.arange(T, dtype=torch.float32)


def _close(a, b, tol=PIN):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1.0)) <= tol


# kind -> (cases, shape names for the MUTATIONS conditions, case builder, evaluation -> {output name: (value, bound)})
def _prologue(c, dtype, mutate):
    return {'out': ref.prologue_bounds(c, dtype, mutate)}


def _token(refine, c, dtype, mutate):
    (z1, y), (b1, by) = ref.token_bounds(c, refine, dtype, mutate)
    return {'z1': (z1, b1), 'y': (y, by)}


def _tail(c, dtype, mutate):
    return {'out': ref.tail_bounds(c, dtype, mutate)}


def _ln_rows(c, dtype, mutate):
    return {'y': ref.ln_rows_bounds(c, dtype, mutate)}


def _mha(c, dtype, mutate):
    return {'out': ref.mha_bounds(c, dtype, mutate)}


def _dyg_prologue(c, dtype, mutate):
    node, edge, time, tmag = ref.dyg_prologue_run(c, dtype, mutate)
    return {'node': (node, torch.zeros_like(node, dtype=F64)), 'edge': (edge, torch.zeros_like(edge, dtype=F64)),
            'time': (time, ref.time_chain() * EPS * tmag.double())}


def _dyg_tail(c, dtype, mutate):
    (mean, out), (bm, bo) = ref.dyg_tail_bounds(c, dtype, mutate)
    return {'mean': (mean, bm), 'out': (out, torch.full_like(out, bo, dtype=F64))}


KINDS = {
    'prologue': (ref.PROLOGUE_CASES, ('S', 'K', 'D', 'T', 'ldo'), ref.prologue_case, _prologue),
    'token': (ref.TOKEN_CASES, ('S', 'K', 'C', 'Ht'), ref.token_case, functools.partial(_token, False)),
    'token_refine': (ref.TOKEN_CASES, ('S', 'K', 'C', 'Ht'), ref.token_case, functools.partial(_token, True)),
    'tail': (ref.TAIL_CASES, ('C', 'F', 'pad', 'split'), ref.tail_case, _tail),
    'ln_rows': (ref.LN_ROWS_CASES, ('R', 'd'), ref.ln_rows_case, _ln_rows),
    'mha': (ref.MHA_CASES, ('B', 'T', 'H', 'dh'), ref.mha_case, _mha),
    'dyg_prologue': (ref.DYG_PROLOGUE_CASES, ('P', 'k', 'widths', 'rows'), ref.dyg_prologue_case, _dyg_prologue),
    'dyg_tail': (ref.DYG_TAIL_CASES, ('P', 'Np', 'D', 'E'), ref.dyg_tail_case, _dyg_tail),
}
ALL = [(kind, case) for kind, spec in KINDS.items() for case in spec[0]]


@functools.lru_cache(maxsize=None)
def _case(kind, case):
    return KINDS[kind][2](*case)


@functools.lru_cache(maxsize=None)
def _want(kind, case):
    return KINDS[kind][3](_case(kind, case), F64, None)


def _worst(kind, case, dtype, mutate):
    """Worst err / bound of an evaluation against the float64 value and its bound (a non-finite result counts as inf)."""
    got = KINDS[kind][3](_case(kind, case), dtype, mutate)
    worst = 0.0
    for name, (want, bound) in _want(kind, case).items():
        g = got[name][0].double()
        r = worst_ratio(g, want, bound) if bool(torch.isfinite(g).all()) else math.inf
        worst = max(worst, r if r == r else math.inf)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# the restatements against torch, float64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R,d', ref.LN_ROWS_CASES)
def test_layernorm_is_torchs(R, d):
    c = ref.ln_rows_case(R, d)
    y, mag = ref.layernorm_rows(c['x'], c['g'], c['b'])
    assert _close(y, F.layer_norm(c['x'].double(), (d,), c['g'].double(), c['b'].double(), ref.LN_EPS))
    assert bool((mag >= y.abs() * (1 - 1e-12)).all())
    const = (c['x'] == c['x'][:, :1]).all(1)
    assert torch.equal(y[const], c['b'].double().expand(R, d)[const]), 'a constant row is exactly beta in float64'


def test_gelu_and_its_derivative_are_torchs():
    a = torch.linspace(-6, 6, 241, dtype=F64).requires_grad_(True)
    F.gelu(a).sum().backward()
    v, d = ref._gelu(a.detach())
    assert _close(v, F.gelu(a.detach())) and _close(d, a.grad.abs())


@pytest.mark.parametrize('B,T,H,dh', ref.MHA_CASES)
def test_mha_is_scaled_dot_product_attention(B, T, H, dh):
    c = ref.mha_case(B, T, H, dh)
    out, mag = ref.mha_small(c['qkv'], H, dh, scale=1.0 / math.sqrt(dh))
    q, k, v = (t.reshape(B, T, H, dh).transpose(1, 2).double() for t in c['qkv'].split(H * dh, dim=-1))
    want = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, H * dh)
    assert _close(out, want, 1e-11)
    assert bool((mag >= out.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('S,K,C,Ht', [(3, 5, 13, 2), (2, 20, 9, 10), (1, 1, 4, 1)])
def test_token_block_composes_to_the_mixer_restatement(S, K, C, Ht):
    c = ref.token_case(S, K, C, Ht)
    g = torch.Generator().manual_seed(5)
    Hc = 2 * C
    cw1, cb1, cw2, cb2 = torch.randn(Hc, C, generator=g), torch.randn(Hc, generator=g), torch.randn(C, Hc, generator=g), torch.randn(C, generator=g)
    sd = {'token_norm.weight': c['tg'], 'token_norm.bias': c['tbeta'], 'token_feedforward.ffn.0.weight': c['w1'], 'token_feedforward.ffn.0.bias': c['b1'],
          'token_feedforward.ffn.3.weight': c['w2'], 'token_feedforward.ffn.3.bias': c['b2'], 'channel_norm.weight': c['cg'], 'channel_norm.bias': c['cb'],
          'channel_feedforward.ffn.0.weight': cw1, 'channel_feedforward.ffn.0.bias': cb1, 'channel_feedforward.ffn.3.weight': cw2,
          'channel_feedforward.ffn.3.bias': cb2}
    want = gr.mixer_forward({k: v.double() for k, v in sd.items()}, '', c['x'].double(), ref.LN_EPS)
    for refine in (False, True):
        z1, y, _, _ = ref.mixer_token(*ref.token_args(c), refine=refine)
        got = z1 + F.linear(F.gelu(F.linear(y, cw1.double(), cb1.double())), cw2.double(), cb2.double())
        # (the special columns' conditioning sets the agreement: 1e4-offset columns through rstd ~ 1)
        assert _close(got, want, 1e-9), refine


def test_graphmixer_blocks_compose_to_the_encoder_restatement():
    S, K, D, T, Fd, E, N = 6, 5, 6, 4, 3, 7, 20
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g)
    pc = ref.prologue_case(S, K, D, T, D + T + 2)
    pc['tw'], pc['tb'] = EXACT_TW(T), torch.zeros(T)
    nids = torch.randint(0, N, (S, K), generator=g, dtype=torch.int32)
    nids[0], nids[1, :3] = -1, -1
    lists = [[], [3], [1, 2, 2], [4, 5, 6, 7], list(range(9)), [0]]
    vals, offs = gr.flatten(lists)
    seeds, node_x = torch.randint(0, N, (S,), generator=g, dtype=torch.int32), r(N, Fd)
    tc = ref.token_case(S, K, D, 2)
    Hc = 3 * D
    sd = {'time_encoder.w.weight': pc['tw'][:, None], 'time_encoder.w.bias': pc['tb'], 'projection_layer.weight': r(D, D + T), 'projection_layer.bias': r(D),
          'output_layer.weight': r(E, D + Fd), 'output_layer.bias': r(E)}
    names = ('token_norm.weight', 'token_norm.bias', 'token_feedforward.ffn.0.weight', 'token_feedforward.ffn.0.bias', 'token_feedforward.ffn.3.weight',
             'token_feedforward.ffn.3.bias', 'channel_norm.weight', 'channel_norm.bias')
    keys = ('tg', 'tbeta', 'w1', 'b1', 'w2', 'b2', 'cg', 'cb')
    sd.update({'mlp_mixers.0.' + n: tc[k] for n, k in zip(names, keys)})
    sd.update({'mlp_mixers.0.channel_feedforward.ffn.0.weight': r(Hc, D), 'mlp_mixers.0.channel_feedforward.ffn.0.bias': r(Hc),
               'mlp_mixers.0.channel_feedforward.ffn.3.weight': r(D, Hc), 'mlp_mixers.0.channel_feedforward.ffn.3.bias': r(D)})
    want = gr.encoder_forward(sd, 1, pc['edge_x'].view(S, K, D), pc['seed_t'], pc['nbr_t'].view(S, K), nids, seeds, lists, node_x)
    d = {k: v.double() for k, v in sd.items()}
    x0, _ = ref.mixer_prologue(pc['edge_x'], pc['seed_t'], pc['nbr_t'], K, D, pc['tw'], pc['tb'], D + T + 2)
    assert not bool(x0[:, D + T:].any())
    z = F.linear(x0[:, :D + T], d['projection_layer.weight'], d['projection_layer.bias']).view(S, K, D)
    z1, y, _, _ = ref.mixer_token(z, *ref.token_args(tc)[1:])
    z = z1 + F.linear(F.gelu(F.linear(y, d['mlp_mixers.0.channel_feedforward.ffn.0.weight'], d['mlp_mixers.0.channel_feedforward.ffn.0.bias'])),
                      d['mlp_mixers.0.channel_feedforward.ffn.3.weight'], d['mlp_mixers.0.channel_feedforward.ffn.3.bias'])
    cat, _ = ref.mixer_tail(z, nids, node_x, torch.from_numpy(vals), torch.from_numpy(offs[:-1]).int(), torch.from_numpy(np.diff(offs)).int(), seeds,
                            D + Fd + 1)
    got = F.linear(cat[:, :D + Fd], d['output_layer.weight'], d['output_layer.bias'])
    assert _close(got, want, 1e-11)


@pytest.mark.parametrize('rows_given', [False, True])
def test_dygformer_blocks_compose_to_the_restatement(rows_given):
    """prologue -> patch projections -> one transformer layer from layernorm_rows and mha_small -> tail, against dygformer_restate."""
    P, k, patch, C, H, E, N = 3, 7, 2, 4, 2, 5, 30
    dN, dE, dT = 3, 4, 6
    S = 2 * P + 3
    g = torch.Generator().manual_seed(13)
    r = lambda *s: torch.randn(*s, generator=g)
    src, dst = (torch.randint(0, N, (P,), generator=g, dtype=torch.int32) for _ in range(2))
    nids = torch.randint(0, 6, (S, k), generator=g, dtype=torch.int32)  # few ids: co-occurrences
    nids[:, :2] = -1
    edge_time = ref.unix_times(P, g)
    nbr_t = edge_time[torch.arange(S) % P][:, None] - torch.randint(0, 41, (S, k), generator=g)
    nbr_x, node_x = r(S, k, dE), r(N, dN)
    nbr_x[nids == -1] = 0  # (the restatement gathers, the reference's sampler wrote zeros there)
    rows = torch.tensor([[5, 0, 7], [2, 8, 1]], dtype=torch.int32) if rows_given else None
    tw, tb = EXACT_TW(dT), torch.zeros(dT)
    D = 4 * C
    L, Np = k + 1, (k + 1) // patch
    sd = {'time_encoder.w.weight': tw[:, None], 'time_encoder.w.bias': tb, 'output_layer.weight': r(E, D), 'output_layer.bias': r(E)}
    co = 'co_occurrence_encoder.neighbor_co_occurrence_encoder.'
    sd.update({co + '0.weight': r(C, 1), co + '0.bias': r(C), co + '2.weight': r(C, C), co + '2.bias': r(C)})
    for name, w in (('node', dN), ('edge', dE), ('time', dT), ('neighbor_co_occurrence', C)):
        sd.update({f'projection_layer.{name}.weight': r(C, patch * w) / w ** 0.5, f'projection_layer.{name}.bias': r(C)})
    t0 = 'transformers.0.'
    sd.update({t0 + 'norm_layers.0.weight': 1 + 0.1 * r(D), t0 + 'norm_layers.0.bias': 0.1 * r(D), t0 + 'norm_layers.1.weight': 1 + 0.1 * r(D),
               t0 + 'norm_layers.1.bias': 0.1 * r(D), t0 + 'multi_head_attention.in_proj_weight': r(3 * D, D) / D ** 0.5,
               t0 + 'multi_head_attention.in_proj_bias': 0.1 * r(3 * D), t0 + 'multi_head_attention.out_proj.weight': r(D, D) / D ** 0.5,
               t0 + 'multi_head_attention.out_proj.bias': 0.1 * r(D), t0 + 'linear_layers.0.weight': r(4 * D, D) / D ** 0.5,
               t0 + 'linear_layers.0.bias': 0.1 * r(4 * D), t0 + 'linear_layers.1.weight': r(D, 4 * D) / D ** 0.5, t0 + 'linear_layers.1.bias': 0.1 * r(D)})
    sel = torch.cat([rows[0], rows[1]]).long() if rows_given else torch.arange(2 * P)
    want_s, want_d = dr.dygformer_forward(sd, patch, 1, H, node_x, src, dst, edge_time, nids[sel], nbr_t[sel], nbr_x[sel])
    d = {k_: v.double() for k_, v in sd.items()}
    node, edge, time, _ = ref.dygformer_prologue(node_x, src, dst, edge_time, nids, nbr_t, nbr_x, S, k, None if rows is None else rows[0],
                                                 None if rows is None else rows[1], tw, tb, dN + 1, dE + 2, dT)
    ids = torch.cat([torch.cat([src, dst])[:, None].long(), nids[sel].long()], 1)  # [2 P, L], sources first
    cs, cd = dr.cooccurrence_counts(ids[:P].numpy(), ids[P:].numpy())
    cofeat = dr.cooccurrence_encode(sd, co, torch.from_numpy(np.stack([cs, cd], 1)))  # [P, 2, L, C]: sequence order q = 2 p + side
    chans = []
    for name, f, w in (('node', node[:, :dN], dN), ('edge', edge[:, :dE], dE), ('time', time[:, :dT], dT), ('neighbor_co_occurrence', cofeat.reshape(2 * P * L, C), C)):
        chans.append(F.linear(f.reshape(2 * P * Np, patch * w), d[f'projection_layer.{name}.weight'], d[f'projection_layer.{name}.bias']))
    x = torch.cat(chans, 1)  # [2 P Np, D]: the 2 Np tokens of pair p in a row
    y, _ = ref.layernorm_rows(x, sd[t0 + 'norm_layers.0.weight'], sd[t0 + 'norm_layers.0.bias'])
    qkv = F.linear(y, d[t0 + 'multi_head_attention.in_proj_weight'], d[t0 + 'multi_head_attention.in_proj_bias'])
    att, _ = ref.mha_small(qkv.view(P, 2 * Np, 3 * D), H, D // H, scale=1.0 / math.sqrt(D // H))
    x1 = x + F.linear(att.reshape(2 * P * Np, D), d[t0 + 'multi_head_attention.out_proj.weight'], d[t0 + 'multi_head_attention.out_proj.bias'])
    y, _ = ref.layernorm_rows(x1, sd[t0 + 'norm_layers.1.weight'], sd[t0 + 'norm_layers.1.bias'])
    x2 = x1 + F.linear(F.gelu(F.linear(y, d[t0 + 'linear_layers.0.weight'], d[t0 + 'linear_layers.0.bias'])), d[t0 + 'linear_layers.1.weight'],
                       d[t0 + 'linear_layers.1.bias'])
    _, _, out = ref.dygformer_tail(x2, P, Np, D + 4, sd['output_layer.weight'], sd['output_layer.bias'])
    assert _close(out[:P], want_s, 1e-10) and _close(out[P:], want_d, 1e-10)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference alone meets the bar; the mutations do not
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,case', ALL, ids=str)
def test_float32_evaluation_stays_within_the_bound(kind, case):
    worst = _worst(kind, case, F32, None)
    print(f'[fwd blocks] {kind} {case}: float32 restatement at {worst:.4f}x the bound')
    assert worst <= 1.0


@pytest.mark.parametrize('name', sorted(ref.MUTATIONS))
def test_every_mutation_exceeds_the_bound_where_it_can_show(name):
    targets, can_show = ref.MUTATIONS[name]
    shown = []
    for kind, (cases, names, _, _) in KINDS.items():
        if kind.replace('_refine', '') not in targets.split('+'):
            continue
        for case in cases:
            worst = _worst(kind, case, F64, name)
            if can_show(**dict(zip(names, case))):
                shown.append((kind, case, worst))
            else:
                assert worst <= 1.0, f'{name} shows at {kind} {case} ({worst:.3g}x) where it is said not to'
    hits = [s for s in shown if s[2] > 1.0]
    print(f'[fwd blocks] {name}: exceeds the bound at {len(hits)} of {len(shown)} cases where it can show')
    assert hits, f'{name} stays within the bound everywhere: {shown}'


# ---------------------------------------------------------------------------------------------------------------------------
# the kRefine claim
# ---------------------------------------------------------------------------------------------------------------------------
CONSTANTS = [0.1, 1.0 / 3.0, 1e6 + 0.1, -7.3e-5, 3.7, 1e-30, 16777215.0, 2.0 ** -126 * 3, 0.7, -123456.789]


@pytest.mark.parametrize('K', [3, 5, 7, 20, 30])
def test_refined_mean_of_equal_values_is_the_value(K):
    off = 0
    for v in CONSTANTS:
        mean, plain = ref.refined_mean_f32(v, K)
        assert mean.tobytes() == np.float32(v).tobytes(), (K, v, float(mean))
        off += plain != np.float32(v)
    print(f'[fwd blocks] K = {K}: the plain float32 mean is off for {off} of {len(CONSTANTS)} constants, the refined one for none')


def test_plain_mean_is_off_somewhere():
    """What the correction is for: without it the mean of K equal values is not always that value."""
    assert any(ref.refined_mean_f32(v, K)[1] != np.float32(v) for v in CONSTANTS for K in (3, 5, 7, 20, 30))
