"""ORACLE (test infrastructure only -- never imported by the product path).

float64 restatements of the forward float kernels of ``csrc/tgn.hip`` (``tgmx_tgn_gru_gate``, ``tgmx_tgn_aggregate``,
``tgmx_tconv_edge_attr``, ``tgmx_tconv_attend``), pure torch on the CPU, in the manner of ``oracle/tgn_bwd_ref.py`` (whose
constants, helpers and case builders are reused, and whose docstring states the magnitude conventions): every function takes the
float32 / integer tensors the kernel gets and returns ``(value, magnitude)``, the value in float64 and, with the same shape, the same
formula with every term replaced by its absolute value.  A worst-case rounding bound for a float32 evaluation is
``n * 2^-24 * magnitude`` with ``n`` from the chain helpers below, counted from the kernels' code and tuned on nothing.
``dtype=torch.float32`` evaluates the same formulas in float32 (plain torch); ``mutate=`` selects a deliberately wrong variant
(``MUTATIONS``).

Magnitudes beyond that docstring: ``|cos|`` counts as 1 (like ``|sin|``); a column that is a plain copy has its own absolute value
(the kernels must reproduce it bit for bit, which the GPU file checks on top of the bound); the softmax weight counts as in
``attend_backward`` (first-order sensitivity to its rounded score plus ``UNDERFLOW_MAG``); the dropout factor keep (0 or
1 / (1 - p)) is an input.  The Time2Vec argument is formed as the kernels form it -- the int64 difference, ONE conversion to float32,
ONE fma rounded once (``_fma32``) -- and is therefore reproduced bit for bit: only the cosine of that float32 argument counts.
"""
from __future__ import annotations

import torch

from .dropout_ref import dropout_scale
from .tgat_bwd_ref import EPS, F64
from .tgn_bwd_ref import (AGGR_CASES, AGGR_ROW, EDGE_BIG_CASE, EDGE_CASES, GRU_BIG_CASE, GRU_CASES, TRANSCENDENTAL_OPS, UNDERFLOW_MAG, UNIX, _fma32,
                          aggr_case, edge_case, edge_targets, gru_case, gru_underflow_floor, time2vec_params)

DROP_SEED = 0x1234ABCD5678


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tgn_gru_gate
# ---------------------------------------------------------------------------------------------------------------------------
def gru_gate(gi, gh, h, dtype=F64, mutate=None):
    """The gate arithmetic of ``TGNMemoryRef._gru`` given gi, gh [R, 3M] (r | z | n) and h [R, M]:

        r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n), out = (1 - z) n + z h

    Magnitudes: r_m = r + r (1 - r) |a_r|_mag, z_m likewise, n_m = |n| + (1 - n^2) (|gi_n| + r_m |gh_n|),
    out_m = (1 + z_m) n_m + z_m |h|.  Returns (out, out_mag)."""
    M = h.shape[1]
    gi, gh, h = (t.to(dtype) for t in (gi, gh, h))
    ar, az = gi[:, :M] + gh[:, :M], gi[:, M:2 * M] + gh[:, M:2 * M]
    ar_m, az_m = gi[:, :M].abs() + gh[:, :M].abs(), gi[:, M:2 * M].abs() + gh[:, M:2 * M].abs()
    r, z = torch.sigmoid(ar), torch.sigmoid(az)
    r_m, z_m = r + r * (1 - r) * ar_m, z + z * (1 - z) * az_m
    gin, ghn = gi[:, 2 * M:], gh[:, 2 * M:]
    if mutate == 'gru_r_on_whole_n':
        n = torch.tanh(r * (gin + ghn))
    else:
        n = torch.tanh(gin + r * ghn)
    n_m = n.abs() + (1 - n * n) * (gin.abs() + r_m * ghn.abs())
    out = z * n + (1 - z) * h if mutate == 'gru_z_swapped' else (1 - z) * n + z * h
    return out, (1 + z_m) * n_m + z_m * h.abs()


def gru_chain() -> int:
    """float32 operations on the longest chain into an element of out, plus 8, counted from tgn_gru_gate_kernel:
    rg = add, expf, add, divide (3 + 4; the negation is exact);  ng = rg * gh_n, add, tanhf (2 + 4);  out = (1 - zg) * ng + zg * h:
    multiply, add (2; 1 - zg and zg * h run beside the chain, zg's own chain is rg's).  15 + 8."""
    return 3 + TRANSCENDENTAL_OPS + 2 + TRANSCENDENTAL_OPS + 2 + 8


def gru_bounds(c):
    """(out, bound): the saturated band's rows get the underflow floor on top (a gate that float32 gives as exactly 0 or 1 where
    float64 keeps 5e-42 of the other operand)."""
    out, mag = gru_gate(c['gi'], c['gh'], c['h'])
    floor = torch.zeros(c['h'].shape[0], 1, dtype=F64)
    floor[c['band']] = gru_underflow_floor(c['gi'], c['gh'], c['h'])
    return out, gru_chain() * EPS * mag + floor


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tgn_aggregate
# ---------------------------------------------------------------------------------------------------------------------------
def aggr_tables(c, negative_row=None):
    """The node-indexed tensors tgmx_tgn_aggregate takes, from an ``aggr_case`` (whose windows and last_update are per ROW): row r is
    node nodes[r]; the other N - R nodes hold a random unix-scale last_update and empty windows at log position 0.
    ``negative_row``: that row's node is given as v - N (the kernel's ``v += N``).  Returns a dict of CPU tensors."""
    N, v = c['N'], c['nodes'].long()
    g = torch.Generator().manual_seed(4242)
    last_update = UNIX + torch.randint(0, 1_000_000, (N,), generator=g)
    last_update[v] = c['lu']
    tab = dict(last_update=last_update, memory=c['memory'], log_other=c['log_other'], log_t=c['log_t'], log_raw=c['log_raw'], tw=c['tw'], tb=c['tb'])
    for name, dt in (('lo_s', torch.int64), ('cnt_s', torch.int32), ('lo_d', torch.int64), ('cnt_d', torch.int32)):
        t = torch.zeros(N, dtype=dt)
        t[v] = c[name]
        tab['st_' + name] = t
    nodes = c['nodes'].clone()
    if negative_row is not None:
        nodes[negative_row] -= N
    tab['nodes'] = nodes
    return tab


def aggr_args(tab, mean):
    return (tab['nodes'], tab['memory'], tab['last_update'], tab['st_lo_s'], tab['st_cnt_s'], tab['st_lo_d'], tab['st_cnt_d'], tab['log_other'],
            tab['log_t'], tab['log_raw'], tab['tw'], tab['tb'], mean)


def aggregate(nodes, memory, last_update, st_lo_s, st_cnt_s, st_lo_d, st_cnt_d, log_other, log_t, log_raw, tw, tb, mean, dtype=F64, mutate=None):
    """aggr [R, 2M + D + T] and new_lu [R] of tgn_aggregate_kernel.  Row r is node v = nodes[r] (v + N when negative); its events are
    the log positions of its source window (lo_s[v] .. + cnt_s[v]) and THEN of its destination window; the message of an event is

        [mem[v] | mem[other] | raw | cos(fma32(float32(t - last_update[v]), tw, tb))]

    LAST takes the event with the largest ``float32(t)``, the first in walk order on ties (``torch.argmax`` semantics); MEAN is the
    sum in walk order divided by the count.  new_lu is the int64 maximum of t, 0 without events; aggr is 0 without events.
    Returns (aggr, new_lu, aggr_mag)."""
    R, N, M, D, T = nodes.numel(), memory.shape[0], memory.shape[1], log_raw.shape[1], tw.numel()
    W = 2 * M + D + T
    aggr, mag = torch.zeros(R, W, dtype=dtype), torch.zeros(R, W, dtype=dtype)
    new_lu = torch.zeros(R, dtype=torch.int64)
    for r in range(R):
        v = int(nodes[r])
        v = v + N if v < 0 else v
        c0, c1 = int(st_cnt_s[v]), int(st_cnt_d[v])
        if mutate == 'ignore_destination_window':
            c1 = 0
        pos = torch.cat([int(st_lo_s[v]) + torch.arange(c0), int(st_lo_d[v]) + torch.arange(c1)])
        if pos.numel() == 0:
            continue
        t = log_t[pos]
        new_lu[r] = t.max()
        if not mean:
            if mutate == 'last_tie_last_wins':
                f = t.float()
                sel = int((f == f.max()).nonzero().max())
            elif mutate == 'last_argmax_int64':
                sel = int(torch.argmax(t))
            else:
                sel = int(torch.argmax(t.float()))
            pos, t = pos[sel:sel + 1], t[sel:sel + 1]
        n = pos.numel()
        lu = last_update[v]
        dt = (t.float() - lu.float()) if mutate == 'dt_float_first' else (t - lu).to(torch.float32)
        enc = torch.cos(_fma32(dt, tw, tb).to(dtype))
        other = log_other[pos].long()
        mem_o = memory[v].expand(n, M) if mutate == 'mem_other_reads_mem_self' else memory[other]
        msgs = torch.cat([memory[v].expand(n, M).to(dtype), mem_o.to(dtype), log_raw[pos].to(dtype), enc], 1)
        mags = torch.cat([msgs[:, :2 * M + D].abs(), torch.ones(n, T, dtype=dtype)], 1)
        if not mean:
            aggr[r], mag[r] = msgs[0], mags[0]
            continue
        cnt = max(c0, 1) if mutate == 'mean_divides_by_source_count' else n
        acc = msgs[0].clone()
        for i in range(1, n):  # in walk order (float32: the kernel's order of additions)
            acc = acc + msgs[i]
        aggr[r], mag[r] = acc / cnt, mags.sum(0) / cnt
    return aggr, new_lu, mag


def aggregate_chain(count, mean: bool, column_kind: str) -> int:
    """float32 operations on the longest chain into an element of aggr, plus 8, counted from tgn_aggregate_kernel /
    tgn_message_cols; ``column_kind`` is 'copy' (mem[v], mem[other], raw) or 'time'.  The argument's conversion and fma are
    reproduced bit for bit by the restatement: not counted.  The multiplication by scale = 1.f is exact: not counted.
    LAST: copy 0 (the GPU file asks for equal bits there), time cos_t2v (4).  MEAN: the same per event, count - 1 additions in
    walk order and the division (count in all).  All + 8."""
    return (TRANSCENDENTAL_OPS if column_kind == 'time' else 0) + (int(count) if mean else 0) + 8


def aggr_bounds(c, mean, tab=None):
    """((aggr, new_lu), bound) for an aggr_case through aggr_tables."""
    tab = aggr_tables(c) if tab is None else tab
    want, new_lu, mag = aggregate(*aggr_args(tab, mean))
    toff = 2 * c['M'] + c['D']
    n = torch.zeros(c['R'], toff + c['T'], dtype=F64)
    for r, (a, b) in enumerate(zip(c['cnt_s'], c['cnt_d'])):
        n[r, :toff] = aggregate_chain(int(a) + int(b), mean, 'copy')
        n[r, toff:] = aggregate_chain(int(a) + int(b), mean, 'time')
    return (want, new_lu), n * EPS * mag


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tconv_edge_attr
# ---------------------------------------------------------------------------------------------------------------------------
def edge_attr(lu_local, src, t, msg, tw, tb, dtype=F64, mutate=None):
    """edge_attr[e] = [cos(fma32(float32(lu_local[src[e]] - t[e]), tw, tb)) | msg[e]] (subtracted in int64, then rounded once).
    ``msg`` [E, D] or None (D = 0).  Returns (value [E, T + D], magnitude)."""
    lu = lu_local[src]
    if mutate == 'dt_float_first':
        dt = lu.float() - t.float()
    elif mutate == 'edge_attr_dt_sign':
        dt = (t - lu).to(torch.float32)
    else:
        dt = (lu - t).to(torch.float32)
    enc = torch.cos(_fma32(dt, tw, tb).to(dtype))
    m = torch.zeros(t.numel(), 0, dtype=dtype) if msg is None else msg.to(dtype)
    return torch.cat([enc, m], 1), torch.cat([torch.ones_like(enc), m.abs()], 1)


def edge_attr_chain() -> int:
    """cos_t2v (4) plus 8 (tconv_edge_attr_kernel; the message columns are copies: equal bits in the GPU file)."""
    return TRANSCENDENTAL_OPS + 8


EDGE_SMALL_LIMIT_CASE = 'small_path_near_its_limit'
EDGE_MIXED_WAVE_CASE = 'one_edge_takes_the_wave_to_the_big_path'
EDGE_FWD_CASES = EDGE_CASES + [EDGE_BIG_CASE, EDGE_SMALL_LIMIT_CASE, EDGE_MIXED_WAVE_CASE]


def edge_fwd_case(case):
    """An ``edge_case`` (with ``msg``), or one of the two forward-only cases that aim at ``cos_t2v``'s per-wave path choice
    (``__all(|x| < 8e6)``):

    * EDGE_SMALL_LIMIT_CASE: E = 96, T = 64, D = 0 (a wave is one edge's 64 columns).  tw runs from 0.5 to 1 and dt from 6.0e6 to
      7.99e6, so EVERY argument lies in [3e6, 8e6): every wave takes cos_t2v_small where x * (2 / pi) is only good to half a unit
      and the one-off correction of k acts.
    * EDGE_MIXED_WAVE_CASE: E = 40, T = 8, D = 0 (a wave is 8 edges).  Every dt is within +-40 except edge 11's 9e6 (tw[0] = 1:
      its first argument is past the limit): wave 1 (edges 8 .. 15) takes cos_t2v_big as a whole, the four others cos_t2v_small."""
    if case == EDGE_SMALL_LIMIT_CASE:
        g = torch.Generator().manual_seed(811)
        E, T = 96, 64
        lu = UNIX + torch.randint(0, 1_000_000, (17,), generator=g)
        src = torch.randint(0, 17, (E,), generator=g)
        diff = torch.randint(6_000_000, 7_990_000, (E,), generator=g)
        tw = torch.linspace(0.5, 1.0, T)
        tb = torch.randn(T, generator=g) * 0.1
        c = dict(lu_local=lu, src=src, t=lu[src] - diff, tw=tw, tb=tb, D=0, T=T, E=E, msg=torch.zeros(E, 0))
        arg = _fma32(diff.float(), tw, tb)
        assert float(arg.min()) >= 3e6 and float(arg.max()) < 8e6
        return c
    if case == EDGE_MIXED_WAVE_CASE:
        g = torch.Generator().manual_seed(812)
        E, T = 40, 8
        lu = UNIX + torch.randint(0, 1_000_000, (17,), generator=g)
        src = torch.randint(0, 17, (E,), generator=g)
        diff = torch.randint(-40, 41, (E,), generator=g)
        diff[11] = 9_000_000
        tw, tb = time2vec_params(T, g)
        arg = _fma32(diff.float(), tw, tb).abs()
        assert float(arg[11].max()) >= 8e6 and float(arg[torch.arange(E) != 11].max()) < 8e6
        return dict(lu_local=lu, src=src, t=lu[src] - diff, tw=tw, tb=tb, D=0, T=T, E=E, msg=torch.zeros(E, 0))
    return edge_case(*case)


def edge_bounds(c):
    want, mag = edge_attr(c['lu_local'], c['src'], c['t'], c['msg'], c['tw'], c['tb'])
    return want, edge_attr_chain() * EPS * mag


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tconv_attend
# ---------------------------------------------------------------------------------------------------------------------------
def attend(q, k, v, eproj, order, src, seg_lo, seg_hi, H, C, scale, out0, keep, dtype=F64, mutate=None):
    """out_i = out0_i + sum_p alpha_p keep_p (v_j + e_p) per head (TransformerConv's attention, the comment above TconvArgs), with
    j = src[e_p], alpha = softmax over the edges into i of s_p = scale q_i . (k_j + e_p); dropout (keep [E, H]: 0 or 1 / (1 - p))
    acts AFTER the normaliser.  A target without edges keeps out0.  Returns (out [U, H*C], magnitude)."""
    U, E = q.shape[0], eproj.shape[0]
    tgt = edge_targets(order, seg_lo, seg_hi, E)
    q, k, v, e, o0, mk = (t.to(dtype) for t in (q, k, v, eproj, out0, keep))
    hc = lambda t: t.view(-1, H, C)
    qe = hc(q)[tgt]
    ke, ke_m = hc(k)[src] + hc(e), hc(k)[src].abs() + hc(e).abs()
    val, val_m = hc(v)[src] + hc(e), hc(v)[src].abs() + hc(e).abs()
    if mutate == 'key_without_edge':
        ke = hc(k)[src]
    if mutate == 'value_without_edge':
        val = hc(v)[src]
    sc = 1.0 if mutate == 'scale_missing' else scale
    s, s_m = sc * (qe * ke).sum(-1), scale * (qe.abs() * ke_m).sum(-1)  # [E, H]
    if mutate == 'score_skips_channel_C-1':
        s = sc * (qe * ke)[..., :C - 1].sum(-1)
    if mutate == 'dropout_head_index_dropped':
        mk = mk[:, :1].expand(E, H)
    idx = tgt[:, None].expand(E, H)
    m = torch.full((U, H), -float('inf'), dtype=dtype).scatter_reduce(0, idx, s, 'amax')
    w = torch.exp(s - m[tgt])
    seg_sum = lambda x: torch.zeros(U, H, dtype=dtype).index_add_(0, tgt, x)[tgt]
    if mutate == 'dropout_inside_normaliser':
        alpha = torch.nan_to_num(w / seg_sum(w * mk), nan=0.0, posinf=0.0)
    else:
        alpha = w / seg_sum(w)
    alpha_m = alpha * (1 + s_m + seg_sum(alpha * s_m)) + UNDERFLOW_MAG
    flat = lambda t: t.reshape(t.shape[0], H * C)
    att = torch.zeros(U, H * C, dtype=dtype).index_add_(0, tgt, flat((alpha * mk)[..., None] * val))
    att_m = torch.zeros(U, H * C, dtype=dtype).index_add_(0, tgt, flat((alpha_m * mk)[..., None] * val_m))
    out = att if mutate == 'skip_not_added' else o0 + att
    return out, o0.abs() + att_m


ATTEND_SHORT = 16  # kTconvShort: up to this many edges the register-resident walks keep a target on ONE wave
ATTEND_WAVES = 4   # beyond, and always on the generic walk: four waves, each over every fourth position


def attend_chain(C: int, L):
    """float32 operations on the longest chain into an element of out, plus 8, counted from tconv_attend_kernel (one figure for its
    three walks: the largest) for a target with L incoming edges (a number or a tensor):

        n = L for L <= 16 (tconv_attend_short: one wave walks them all), else ceil(L / 4) (a wave's share of the positions)
        s: k + e, q * ke, the lane sum (five or six shuffle adds, counted as C: a C-term dot product), * scale                C + 3
        w = expf(s - mn)                                                                                                       + 5
        per edge of the wave: corr = expf(m - mn) (1 + 4: the running maximum may move at every edge), acc * corr, + (2)        + 7 n
        the merge of the four waves: f = expf(m_w - M) (1 + 4), * f, + (2), four times                                         + 28
      that is the normaliser l: C + 7 n + 36.  The sum acc runs the same chain with wd = w * keep, v + e, wd * val (3) more, and
      the result is acc / l (1) added to out (1): both chains enter it.
    2 (C + 7 n + 36) + 5 + 8."""
    L = torch.as_tensor(L)
    n = torch.where(L <= ATTEND_SHORT, L, (L + ATTEND_WAVES - 1) // ATTEND_WAVES)
    return 2 * (C + 7 * n + 36) + 5 + 8


# the issue's table with the 12-edge spread target placed in front of the final empty one
ATTEND_FWD_COUNTS = [0, 1, 2, 3, 4, 5, 16, 17, 64, 65, 255, 256, 257, 300, 1024, 1025, 2049, 12, 0]
ATTEND_FWD_U = len(ATTEND_FWD_COUNTS)
ATTEND_FWD_HUB_TARGET, ATTEND_FWD_HUB_SOURCE, ATTEND_FWD_LOOP = 16, 3, 5
ATTEND_FWD_SPREAD12, ATTEND_FWD_SPREAD300, ATTEND_FWD_WEAK_WAVE = 17, 13, 2
ATTEND_FWD_HEAVY_LAST = [5, 7, 9, 12, 15, 16]  # the targets with 5, 17, 65, 257, 1025, 2049 edges: one past a block, a walk, a trip
# (H, C) -> floats per lane of the walk tconv_short_ok gives with every operand on the 16-byte grid (0 = the generic walk)
ATTEND_FWD_WIDTHS = {(2, 4): 4, (2, 64): 4, (2, 128): 4, (2, 2): 2, (2, 50): 2, (2, 62): 2, (2, 3): 0, (2, 65): 0, (2, 132): 0, (1, 1): 0,
                     (1, 64): 0, (3, 33): 0, (3, 70): 0}
ATTEND_FWD_ALIGN = (2, 8)  # run with eproj 0, 8 and 4 bytes off the 16-byte grid: walks 4, 2 and generic
ATTEND_FWD_DROPOUT = [(2, 64, 0.1), (2, 64, 0.5), (3, 33, 0.1), (3, 33, 0.5)]
ATTEND_FWD_CASES = [(H, C, 0.0) for H, C in ATTEND_FWD_WIDTHS] + [ATTEND_FWD_ALIGN + (0.0,)] + ATTEND_FWD_DROPOUT


def tconv_walk(H, C, *pointers):
    """tconv_short_ok's rule restated: 4 or 2 floats per lane of the register-resident walks, 0 for the generic walk."""
    bits = 0
    for p in pointers:
        bits |= int(p)
    if H != 2:
        return 0
    if C % 4 == 0 and C // 4 <= 32 and bits & 15 == 0:
        return 4
    if C % 2 == 0 and C // 2 <= 32 and bits & 7 == 0:
        return 2
    return 0


def attend_fwd_graph():
    """The segment table all widths share: U = 19 targets with ATTEND_FWD_COUNTS incoming edges (E = 5355), the edge list in
    random order, ``order`` the stable sort by target (no identity).  Source 3 feeds the 2049-edge target throughout; target 5 has
    a self loop.  Returns (tgt, src, order, seg_lo, seg_hi)."""
    g = torch.Generator().manual_seed(20240)
    U = ATTEND_FWD_U
    tgt = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(ATTEND_FWD_COUNTS)])
    E = tgt.numel()
    src = torch.randint(0, U, (E,), generator=g)
    src[tgt == ATTEND_FWD_HUB_TARGET] = ATTEND_FWD_HUB_SOURCE
    src[int((tgt == ATTEND_FWD_LOOP).nonzero()[0])] = ATTEND_FWD_LOOP
    perm = torch.randperm(E, generator=g)
    tgt, src = tgt[perm], src[perm]
    order = torch.sort(tgt, stable=True)[1]
    counts = torch.tensor(ATTEND_FWD_COUNTS)
    seg_hi = counts.cumsum(0)
    return tgt, src, order, seg_hi - counts, seg_hi


def attend_fwd_case(H, C, p, seed=0):
    """q, k, v, out0 [U, H*C] and eproj [E, H*C] (randn; eproj halved) over attend_fwd_graph().  The two spread targets have q = 1 and
    eproj = a / sqrt(C) in every channel, so their scores are a plus noise of order 1:

    * the 12-edge target: a from -60 to 60 over its edges (float32's expf gives exactly 0 for the weak ones);
    * the 300-edge target: a from -60 to 60 over its positions, except the positions p with p % 4 == 2 -- the share of wave 2 of
      the four-wave walks -- whose a runs from -60 to -50: that wave's whole share lies 100 below the others' maximum, its factor
      expf(m_2 - M) in the merge is exactly 0;
    * the targets with 5, 17, 65, 257, 1025 and 2049 edges (ATTEND_FWD_HEAVY_LAST): the LAST position's edge -- the one past a block of
      four, past the one-wave walk, alone in a wave's next trip -- gets eproj += beta sqrt(C) q / max(|q|^2, 1/4) per head with
      beta = ln(L) + 1.5, a score about beta above the others': it carries most of the weight (0.7 at |q|^2 >= 1/4), so a walk that
      loses it is far outside the bound (tests/test_tgn_fwd_ref_cpu.py shows that).

    keep [E, H] = dropout_scale(p, DROP_SEED, stream, (E, H)); p = 0.5: stream is the first one from 0 for which target 1's single
    edge is dropped in head 0 (a (target, head) whose every edge is dropped: it must add exactly 0).  Returns a dict of CPU tensors."""
    tgt, src, order, seg_lo, seg_hi = attend_fwd_graph()
    g = torch.Generator().manual_seed(1000 * seed + 97 * H + 13 * C)
    U, E, HC = ATTEND_FWD_U, tgt.numel(), H * C
    q, k, v, out0 = (torch.randn(U, HC, generator=g) for _ in range(4))
    eproj = torch.randn(E, HC, generator=g) * 0.5
    for t_ in (ATTEND_FWD_SPREAD12, ATTEND_FWD_SPREAD300):
        q[t_] = 1.0
        sp = (tgt == t_).nonzero()[:, 0]  # ascending edge id: the segment's positions
        a = torch.linspace(-60, 60, sp.numel())
        if t_ == ATTEND_FWD_SPREAD300:
            weak = torch.arange(sp.numel()) % ATTEND_WAVES == ATTEND_FWD_WEAK_WAVE
            a[weak] = torch.linspace(-60, -50, int(weak.sum()))
        eproj[sp] = (a / C ** 0.5)[:, None].expand(sp.numel(), HC)
    heavy = []
    for t_ in ATTEND_FWD_HEAVY_LAST:
        last = int((tgt == t_).nonzero()[-1])
        qh = q[t_].view(H, C)
        beta = float(torch.log(torch.tensor(float(ATTEND_FWD_COUNTS[t_])))) + 1.5
        eproj[last] += (beta * C ** 0.5 * qh / (qh * qh).sum(-1, keepdim=True).clamp(min=0.25)).reshape(HC)
        heavy.append(last)
    stream = 6
    if p == 0.5:
        e1 = int((tgt == 1).nonzero()[0])
        stream = next(s for s in range(256) if float(dropout_scale(p, DROP_SEED, s, (E, H))[e1, 0]) == 0.0)
    keep = dropout_scale(p, DROP_SEED, stream, (E, H))
    return dict(q=q, k=k, v=v, eproj=eproj, order=order, src=src, seg_lo=seg_lo, seg_hi=seg_hi, H=H, C=C, scale=float(C) ** -0.5, out0=out0,
                keep=keep, tgt=tgt, U=U, E=E, p=p, stream=stream, heavy=heavy)


def attend_args(c):
    return tuple(c[n] for n in ('q', 'k', 'v', 'eproj', 'order', 'src', 'seg_lo', 'seg_hi', 'H', 'C', 'scale', 'out0', 'keep'))


def attend_bounds(c):
    """(out, bound): the chain length is per target (its own segment)."""
    want, mag = attend(*attend_args(c))
    n = attend_chain(c['C'], c['seg_hi'] - c['seg_lo']).double()[:, None]
    return want, n * EPS * mag


# ---------------------------------------------------------------------------------------------------------------------------
# deliberately wrong variants: name -> (kernels, the condition under which the mutation can show at a case)
# ---------------------------------------------------------------------------------------------------------------------------
MUTATIONS = {
    # LAST with a float32 tie between distinct int64 times (aggr_case rows 11 - 13): the later, larger one wins instead
    'last_tie_last_wins': ('aggregate', lambda mean=0, **_: not mean),
    'last_argmax_int64': ('aggregate', lambda mean=0, **_: not mean),
    # rows with a destination window: their events vanish (LAST: where the maximum sits there; MEAN: always)
    'ignore_destination_window': ('aggregate', lambda **_: True),
    'mean_divides_by_source_count': ('aggregate', lambda mean=0, **_: bool(mean)),  # rows with c1 > 0
    # float(t) - float(lu): off by up to 128 at unix-scale times (every aggr_case / edge_case is one; the two forward-only edge
    # cases too: their lu and t are unix-scale)
    'dt_float_first': ('aggregate+edge_attr', lambda **_: True),
    'mem_other_reads_mem_self': ('aggregate', lambda **_: True),  # columns [M, 2M)
    'edge_attr_dt_sign': ('edge_attr', lambda **_: True),  # cos(-x + tb) != cos(x + tb) because tb != 0
    'gru_r_on_whole_n': ('gru', lambda **_: True),
    'gru_z_swapped': ('gru', lambda **_: True),
    'score_skips_channel_C-1': ('attend', lambda **_: True),  # a lane mask one short (C = 1: every score is 0)
    'key_without_edge': ('attend', lambda **_: True),
    'value_without_edge': ('attend', lambda **_: True),
    'dropout_inside_normaliser': ('attend', lambda p=0.0, **_: p > 0),  # l accumulates the dropped weight
    'dropout_head_index_dropped': ('attend', lambda p=0.0, H=1, **_: p > 0 and H > 1),  # one head has no other index
    'scale_missing': ('attend', lambda C=1, **_: C > 1),  # C = 1: the scale is 1
    'skip_not_added': ('attend', lambda **_: True),
}
