"""ORACLE (test infrastructure only -- never imported by the product path).

float64 restatements of the kernels of ``csrc/tpnet.hip`` one by one, in the manner of ``oracle/fwd_blocks_ref.py``: ``tgmx_tpnet_update``
(``tpnet_stage_kernel`` + ``tpnet_apply_kernel``), ``tgmx_tpnet_pair_features`` (``tpnet_pair_kernel``), ``tgmx_tpnet_tokens``
(``tpnet_tokens_kernel``) and ``tgmx_tpnet_mean`` (``tpnet_mean_kernel``), restated from the contracts in ``include/tgm_amd.h`` -- plain
torch on the host, nothing imported from ``tgm_amd``.  Every function takes the float32 / int32 / int64 tensors the kernel gets and returns
the value in float64 together with its magnitude (the same formula with every term replaced by its absolute value; 0 says "exact": copied
columns, structural zeros, level 0).  A worst-case bound for a float32 evaluation is ``(n + SLACK) * 2^-24 * magnitude`` with ``n`` from
the chain helpers, counted from the kernel code; nothing is tuned on a device result.  ``dtype=torch.float32`` evaluates the same formulas
in float32 with the kernel's roundings in the kernel's places:

* update: ``sc = float32(exp(-lam (next - now) i))`` and ``w = float32(exp(-lam (next - t_e)))`` (the exponentials themselves are taken in
  double, as on the device), a message is ``(P[m][other] * sc_m) * w``, a row is ``P[i][r] * sc_i`` and then gains its messages one by one
  in contribution order (sources j < n, then destinations);
* pair features: float32 products and sums (torch's order, not the kernel's: the bound is order-free), float32 ``log1p``;
* tokens: the time columns are computed in DOUBLE up to the cosine and rounded once, as the kernel has them -- the float32 evaluation
  rounds the float64 value; every other column is a copy;
* mean: float32 sum and division.

Bounds that are not a chain times a magnitude: the scaled pair features get the Gram bound (``log1p`` has slope <= 1 on x >= 0, and the
clamp has slope <= 1) plus ``4 * 2^-24 |log1p(x)|`` -- the 2 ulp OCML documents for float32 ``log1p``; a time column gets one rounding of a
double result, ``2^-24 |cos| + 2^-48 (|w lg| + |b| + 1)`` (the double log, fma and cosine are each good to an ulp or two of 2^-53: 2^-48
leaves a factor 32).

``*_case`` build the inputs the CPU and the GPU tests share; ``MUTATIONS`` lists deliberately wrong variants and the case each is shown at.
"""
from __future__ import annotations

import math

import torch

from .fwd_blocks_ref import GAPS, SLACK
from .tgat_bwd_ref import EPS, F64
from .tgn_bwd_ref import UNIX, time2vec_params

LOG1P_ULPS = 4  # 2 ulp = 4 * 2^-24 relative: OCML's documented accuracy of float32 log1p
EPS64_TIME = 2.0 ** -48


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tpnet_update
# ---------------------------------------------------------------------------------------------------------------------------
def rp_update(tables, now, src, dst, time, lam, num_nodes, dtype=F64, mutate=None):
    """One batch of n edges over the tables P[0 .. L] [num_nodes, dim].  next = time[-1]; level i >= 1 is rescaled by
    exp(-lam (next - now))^i and then gains, for every edge with BOTH endpoints in [0, num_nodes), P_old[i-1][other] decay^(i-1)
    exp(-lam (next - t_e)), read before the batch writes: contribution j < n has target src[j] and other dst[j], contribution n + e has
    target dst[e] and other src[e], and a row's contributions arrive in the order of j.  Level 0 is never written.  ``now``: an int or a
    float.  Returns (new tables, magnitudes |P sc| + sum |msg| (level 0: zeros), count [num_nodes] of contributions per row, next)."""
    N, L1 = int(num_nodes), len(tables)
    src, dst, time = src.long().reshape(-1), dst.long().reshape(-1), time.long().reshape(-1)
    n = src.numel()
    old = [t.to(dtype) for t in tables]
    if n == 0:
        return old, [torch.zeros_like(t, dtype=F64) for t in old], torch.zeros(N, dtype=torch.int64), now
    nxt = int(time[-1])
    dnow = float(nxt) - float(now)
    expo = (lambda i: min(i, 1)) if mutate == 'update_decay_exponent_one' else (lambda i: i)
    sc = [torch.tensor(math.exp(-lam * dnow * expo(i)), dtype=F64).to(dtype) for i in range(L1)]  # one rounding in float32
    base = float(now) if mutate == 'update_now_in_edge_weight' else float(nxt)
    w = torch.exp(-lam * (base - time.double())).to(dtype)  # one rounding in float32
    tgt, oth, w2 = torch.cat([src, dst]), torch.cat([dst, src]), torch.cat([w, w])
    tin, oin = (tgt >= 0) & (tgt < N), (oth >= 0) & (oth < N)
    ok = tin & oin
    if mutate == 'update_half_valid_edges_applied':
        ok, oth = tin, oth % N
    ok = ok.clone()
    if mutate == 'update_no_dst_to_src':
        ok[:n] = False
    if mutate == 'update_lost_j64' and 2 * n > 64:
        ok[64] = False
    if mutate == 'update_lost_last':
        ok[2 * n - 1] = False
    # the contributions of a row in rounds: round r adds every row's r-th contribution, so a row's own order is that of j
    idx = ok.nonzero().reshape(-1)
    order = torch.sort(tgt[idx], stable=True)
    idx, st = idx[order.indices], order.values
    first = torch.searchsorted(st, st)  # the first position of each target's run
    rank = torch.arange(idx.numel()) - first
    count = torch.zeros(N, dtype=torch.int64).index_add_(0, st, torch.ones_like(st))
    scaled = [old[0]] + [old[i] * sc[i] for i in range(1, L1)]
    new, mags = [old[0] * sc[1] if mutate == 'update_level0_rescaled' and L1 > 1 else old[0]], [torch.zeros_like(old[0], dtype=F64)]
    for i in range(1, L1):
        m = i - 1
        source = old[m] if mutate == 'update_message_not_decayed' else (new[m] if mutate == 'update_level_read_after_writes' else scaled[m])
        msg = source[oth.clamp(0, N - 1)] * w2[:, None]  # [2 n, dim]; only the rows of idx are used
        t = scaled[i].clone()
        if mutate == 'update_rows_without_message_not_rescaled':
            t[count == 0] = old[i][count == 0]
        for r in range(int(rank.max()) + 1 if rank.numel() else 0):
            sel = idx[rank == r]
            t[tgt[sel]] = t[tgt[sel]] + msg[sel]
        new.append(t)
        mags.append(scaled[i].double().abs().index_add_(0, tgt[idx], msg[idx].double().abs()))
    return new, mags, count, nxt


def update_chain(count):
    """float32 roundings into an element of a row with ``count`` arriving messages, counted from tpnet_stage_kernel / tpnet_apply_kernel:
    the roundings of sc and of w to float32 (2), the two multiplies of a message ``(P * sc) * w`` (2), the row's own rescale (1), one add
    per message (count).  ``count``: an int or a tensor."""
    return count + 5


def update_bounds(c, dtype=F64, mutate=None):
    """(tables after the batch, one bound per level); level 0's bound is 0: it must keep its bits."""
    new, mags, count, _ = rp_update(c['tables'], c['now'], c['src'], c['dst'], c['time'], c['lam'], c['N'], dtype, mutate)
    n = (update_chain(count) + SLACK).double()[:, None]
    return new, [n * EPS * m for m in mags]


# (n, N, dim, L, flag): one edge; 2 n = 64 (one full chunk of the apply scan) with now == next; 2 n = 66 with a float now; four chunks, the
# dim past two 64-lane trips; eight levels at equal times; dim one short of a trip
UPDATE_CASES = [(1, 2, 1, 1, ''), (32, 40, 16, 2, 'now_is_next'), (33, 40, 65, 2, 'float_now'), (100, 50, 130, 2, ''),
                (40, 30, 64, 7, 'times_equal'), (12, 15, 63, 1, 'float_now')]
UPDATE_EXACT_CASES = [c[:4] + ('exact',) for c in UPDATE_CASES]
# 2 n L = 65 540 stage items and 65 539 apply rows: wave_blocks caps the grid at 16 384 blocks x 4 waves, the second trip is the tail
UPDATE_BIG_CASE = (32770, 65539, 3, 1, 'exact')
UPDATE_BEGIN = 1000


def update_case(n, N, dim, L, flag='', seed=0):
    """Edges with endpoints drawn from the ordinary nodes [1, N - 3); n >= 12 plants (hub = node 0, h = min(36, (n - 6) / 2)):
    edges [0, h) have the hub as source, edges [n - 6 - h, n - 6) have it as destination (n = 100: 72 contributions, j in [0, 36) and
    [158, 194): chunks 0, 2 and 3 of the apply scan; n = 40: j in [0, 17) and [57, 74): across j = 64); edge n - 6 has dst = -1, edge n - 5
    a source of N + 3, edges n - 4 and n - 3 are one edge twice, edge n - 2 is a self loop, edge n - 1 is the only one to name node N - 3
    and names it as its destination (its one contribution is j = 2 n - 1, the last one, past the first chunk once n >= 33).  Node N - 2
    is named by nobody.  Times are sorted, 3 apart on average, from UPDATE_BEGIN; lam = 1e-3 (decay ~ 0.9 .. 0.4 per level).
    Flags: 'now_is_next' (now = time[-1]: decay exactly 1; the unnamed node's rows hold -0.0 and a denormal), 'float_now'
    (now = UPDATE_BEGIN - 0.5), 'times_equal', 'exact' (small-integer tables, lam = 0: every factor is 1, every sum an integer below 2^24)."""
    g = torch.Generator().manual_seed(1000 * seed + 131 * n + 17 * N + 7 * dim + L)
    lo, hi = (1, N - 3) if n >= 12 else (0, N)
    src = torch.randint(lo, hi, (n,), generator=g, dtype=torch.int32)
    dst = torch.randint(lo, hi, (n,), generator=g, dtype=torch.int32)
    plants = {}
    if n >= 12:
        h = min(36, (n - 6) // 2)
        src[:h], dst[n - 6 - h:n - 6] = 0, 0
        dst[n - 6], src[n - 5] = -1, N + 3
        src[n - 3], dst[n - 3] = src[n - 4], dst[n - 4]
        dst[n - 2] = src[n - 2]
        dst[n - 1] = N - 3
        plants = dict(hub=0, dst_only=N - 3, unnamed=N - 2, self_loop=int(src[n - 2]), hub_count=2 * h)
    time = UPDATE_BEGIN + 1 + torch.cumsum(torch.randint(0, 7, (n,), generator=g), 0)
    if flag == 'times_equal':
        time = torch.full((n,), UPDATE_BEGIN + 300)
    now = int(time[-1]) if flag == 'now_is_next' else (UPDATE_BEGIN - 0.5 if flag == 'float_now' else UPDATE_BEGIN)
    if flag == 'exact':
        tables = [torch.randint(-3, 4, (N, dim), generator=g).float() for _ in range(L + 1)]
    else:
        tables = [torch.randn(N, dim, generator=g) * (1.0 if i == 0 else 0.3) for i in range(L + 1)]
    if flag == 'now_is_next' and plants:
        for t in tables[1:]:
            t[plants['unnamed'], 0], t[plants['unnamed'], -1] = -0.0, 1e-41
    return dict(tables=tables, now=now, src=src, dst=dst, time=time, lam=0.0 if flag == 'exact' else 1e-3, n=n, N=N, dim=dim, L=L, flag=flag, **plants)


def three_contribution_case():
    """A row (node 2) with exactly three contributions, the last of them j = 2 n - 1; node 5 is named by nobody."""
    g = torch.Generator().manual_seed(3)
    src, dst = torch.tensor([2, 1, 3, 4], dtype=torch.int32), torch.tensor([0, 2, 1, 2], dtype=torch.int32)
    return dict(tables=[torch.randn(6, 5, generator=g), torch.randn(6, 5, generator=g) * 0.3], now=UPDATE_BEGIN, src=src, dst=dst,
                time=torch.tensor([1001, 1004, 1009, 1010]), lam=1e-3, n=4, N=6, dim=5, L=1, flag='', row=2)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tpnet_pair_features
# ---------------------------------------------------------------------------------------------------------------------------
def pair_features(tables, a, a_rows, a_num_rows, k, b0, b1, bmod, n, concat, scale, dtype=F64, mutate=None):
    """Item t = q k + j pairs node a[(a_rows[q] or q) k + j] (a row index outside [0, a_num_rows) reads as id -1) with b0[q % bmod]; a
    negative id wraps once (-1 is the last row).  With R_x [NL, dim] the rows of node x in the NL tables: concat: the (2 NL)^2 Gram matrix
    of [R_a; R_b], else the NL^2 products R_a R_b^T, row-major.  b1 given: items [n, 2 n) hold the same against b1.  scale:
    log1p(max(x, 0)).  Returns (out [n or 2 n, NR^2], the Gram magnitude sum_c |a_c b_c| of the unscaled entry)."""
    N = tables[0].shape[0]
    t = torch.arange(n)
    q, j = t // k, t % k
    hr = q if a_rows is None else a_rows.long()[q]
    inb = (hr >= 0) & (hr < a_num_rows)
    ida = torch.where(inb, a.reshape(-1).long()[hr.clamp(0, max(a_num_rows - 1, 0)) * k + j], torch.full((), -1, dtype=torch.int64))

    def wrap(i):
        r = torch.where(i < 0, torch.zeros_like(i) if mutate == 'pair_pad_reads_row_0' else i + N, i)
        assert bool(((r >= 0) & (r < N)).all()), 'ids wrap once'
        return r

    outs, mags = [], []
    for blk, b in enumerate([b0] if b1 is None else [b0, b1]):
        if mutate == 'pair_second_block_uses_b0':
            b = b0
        idb = b.long()[q.clamp(max=bmod - 1) if mutate == 'pair_b_index_clamped' else q % bmod]
        ra = torch.stack([T.to(dtype)[wrap(ida)] for T in tables], 1)  # [n, NL, dim]
        rb = torch.stack([T.to(dtype)[wrap(idb)] for T in tables], 1)
        if concat:
            r = torch.cat([ra, rb], 1)
            f, m = r @ r.transpose(1, 2), r.double().abs() @ r.double().abs().transpose(1, 2)
        else:
            f, m = ra @ rb.transpose(1, 2), ra.double().abs() @ rb.double().abs().transpose(1, 2)
            if mutate == 'pair_cross_transposed':
                f = f.transpose(1, 2)
        outs.append(f.reshape(n, -1))
        mags.append(m.reshape(n, -1))
    f, m = torch.cat(outs), torch.cat(mags)
    if scale:
        x = f if mutate == 'pair_clamp_missing' else f.clamp(min=0)
        f = torch.log(x) if mutate == 'pair_log_not_log1p' else torch.log1p(x)
    return f, m


def gram_chain(dim: int, vec: int) -> int:
    """tpnet_pair_kernel<NL, CONCAT, VEC>: a lane runs ceil(dim / (64 VEC)) steps of VEC fmas into an entry, the butterfly adds 6."""
    return -(-dim // (64 * vec)) * vec + 6


def pair_bounds(c, dtype=F64, mutate=None):
    v, mag = pair_features(c['tables'], c['a'], c['a_rows'], c['a_num_rows'], c['k'], c['b0'], c['b1'], c['bmod'], c['n'], c['concat'], c['scale'],
                           dtype, mutate)
    vec = 2 if c['dim'] % 2 == 0 and not c['offset'] else 1  # the launcher: float2 loads need an even dim and 8-byte aligned tables
    bound = (gram_chain(c['dim'], vec) + SLACK) * EPS * mag
    if c['scale']:
        bound = bound + LOG1P_ULPS * EPS * v.double().abs()
    return v, bound


PAIR_DIMS = (1, 2, 63, 64, 65, 128, 130, 300)
PAIR_NODES, PAIR_SEQS = 23, 6


def _pair_cases():
    """(NL, concat, dim, scale, k, rows, b1, short_bmod, ldo_pad, offset): NL x concat x dim exhaustive; the six two-valued axes are bits
    of (dim index + combination index) mod 8 and of their sums, so each value of each meets every (NL, concat) four times; every even
    dim once more with the tables one float into their allocations (the scalar route of an even dim)."""
    cases = []
    for ci, (NL, concat) in enumerate((NL, cc) for NL in (1, 2, 3, 4) for cc in (1, 0)):
        for di, dim in enumerate(PAIR_DIMS):
            d = (di + ci) % 8
            b = (d & 1, (d >> 1) & 1, (d >> 2) & 1)
            cases.append((NL, concat, dim, b[0], (1, 5)[b[1]], b[2], b[0] ^ b[1], b[0] ^ b[2], 4 * (b[1] ^ b[2]), 0))
            if dim % 2 == 0:
                cases.append((NL, concat, dim, b[1], (1, 5)[b[2]], b[0], b[0] ^ b[2], b[1] ^ b[2], 4 * (b[0] ^ b[1]), 1))
    return cases


PAIR_CASES = _pair_cases()
PAIR_BIG_CASE = (1, 1, 2, 0, 1, 0, 0, 0, 0, 0)  # with items=65539: one wave per item, 3 past 16 384 blocks x 4 waves


def pair_case(NL, concat, dim, scale, k, rows, b1, short_bmod, ldo_pad, offset, items=None, seed=0):
    """PAIR_SEQS = 6 sequences of k slots over PAIR_NODES = 23 nodes (``items``: that many sequences over 1000 nodes).  Tables randn /
    dim^(1/4) (Gram entries of order 1, both signs: the clamp works).  The first slots hold the ids 0, N - 1 and -1.  rows: a has two rows
    more, a_rows is a permutation with a -1 and an a_num_rows planted (both read as pads).  short_bmod: b has 4 entries (< 6 sequences)."""
    g = torch.Generator().manual_seed(1000 * seed + 977 * NL + 131 * dim + 64 * concat + 32 * scale + 16 * rows + 8 * b1 + 4 * short_bmod + 2 * offset + k)
    Q, N = (items, 1000) if items else (PAIR_SEQS, PAIR_NODES)
    tables = [torch.randn(N, dim, generator=g) / dim ** 0.25 for _ in range(NL)]
    A = Q + 2 if rows else Q
    a = torch.randint(0, N, (A, k), generator=g, dtype=torch.int32)
    a_rows = None
    if rows:
        a_rows = torch.randperm(A, generator=g)[:Q].to(torch.int32)
        a_rows[1], a_rows[Q - 1] = -1, A
    flat = a.view(-1)
    first = int(a_rows[0]) * k if rows else 0
    plant = torch.tensor([0, N - 1, -1], dtype=torch.int32)[: min(3, k)]
    flat[first:first + plant.numel()] = plant
    if k == 1 and not items:
        last = int(a_rows[2]) if rows else 2
        a[last, 0], a[int(a_rows[3]) if rows else 3, 0] = N - 1, -1
    bmod = 4 if short_bmod else Q
    mk = lambda: torch.randint(0, N, (bmod,), generator=g, dtype=torch.int32)
    b0, bb1 = mk(), (mk() if b1 else None)
    b0[0], b0[1] = -1, N - 1
    NR = 2 * NL if concat else NL
    return dict(tables=tables, a=a, a_rows=a_rows, a_num_rows=A, k=k, b0=b0, b1=bb1, bmod=bmod, n=Q * k, concat=concat, scale=scale, NL=NL, NR=NR,
                dim=dim, N=N, ldo=NR * NR + ldo_pad, offset=offset)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tpnet_tokens
# ---------------------------------------------------------------------------------------------------------------------------
def tokens(node_x, num_nodes, dN, edge_time, B, nbr_nids, nbr_t, nbr_x, S, k, dE, rows, tw, tb, dT, pf, pf_dim, ldo, dtype=F64, mutate=None):
    """Row (q, j), q < 2 B sequences (sources, then destinations) of k slots read from row rows[q] (None: q) of the hop-0 output nbr_*
    [S, k(, dE)]: [node_x[id] (0 on a pad slot and for an id outside [0, num_nodes)) | cos(tw lg + tb) with lg = log(double(edge_time[q
    mod B] - nbr_t + 1)) (0 on a pad slot; an id >= num_nodes still has its time) | nbr_x as given | pf[row, :pf_dim] | pf[2 B k + row,
    :pf_dim] | 0 up to ldo].  A row index outside [0, S) reads as all pads with zero edge features.  Returns (out [2 B k, ldo], bound
    [2 B k, ldo] -- absolute, the one rounding of a double result on the time columns and 0 elsewhere --, lg [2 B k] float64 with -1 on
    pads)."""
    Q, R = 2 * B, 2 * B * k
    q = torch.arange(Q)
    p = q.clamp(max=B - 1) if mutate == 'tokens_dst_time_clamped' else torch.where(q < B, q, q - B)
    hr = q if rows is None else rows.long()
    inb = (hr >= 0) & (hr < S)
    hc = torch.where(inb, hr, torch.zeros_like(hr))
    ids = torch.where(inb[:, None], nbr_nids.long()[hc], torch.full((), -1, dtype=torch.int64))  # [Q, k]
    pad = ids == -1
    has_x = ~pad & (ids >= 0) & (ids < num_nodes)
    gap = edge_time.long()[p][:, None] - nbr_t.long()[hc] + (0 if mutate == 'tokens_gap_without_plus_one' else 1)
    lg = torch.where(pad, torch.zeros((), dtype=F64), torch.log(torch.where(pad, torch.ones_like(gap), gap).double()))
    out, bound = torch.zeros(Q, k, ldo, dtype=dtype), torch.zeros(Q, k, ldo, dtype=F64)
    if dN:
        zero = torch.zeros((), dtype=dtype)  # (a product with the mask would leave -0.0 where the kernel stores 0.f)
        nx = torch.where(has_x[..., None], node_x.to(dtype)[ids.clamp(0, num_nodes - 1)], zero)
        if mutate == 'tokens_pad_node_is_last_row':
            nx = torch.where(pad[..., None], node_x.to(dtype)[num_nodes - 1], nx)
        out[..., :dN] = nx
    if dT:
        wl = tw.double() * lg[..., None]
        v = torch.cos(wl + tb.double())
        live = torch.ones_like(pad) if mutate == 'tokens_time_on_pads' else ~pad
        out[..., dN:dN + dT] = torch.where(live[..., None], v, torch.zeros((), dtype=F64)).to(dtype)  # double up to the cosine, one rounding
        bound[..., dN:dN + dT] = (EPS * v.abs() + EPS64_TIME * (wl.abs() + tb.double().abs() + 1)) * (~pad)[..., None]
    if dE:
        ex = nbr_x.to(dtype)[hc]
        if mutate != 'tokens_row_out_of_range_reads_edge_features':
            ex = torch.where(inb[:, None, None], ex, torch.zeros((), dtype=dtype))
        out[..., dN + dT:dN + dT + dE] = ex
    if pf_dim:
        base = dN + dT + dE
        blk = [pf[:R, :pf_dim].to(dtype).view(Q, k, pf_dim), pf[R:2 * R, :pf_dim].to(dtype).view(Q, k, pf_dim)]
        if mutate == 'tokens_pair_blocks_swapped':
            blk = blk[::-1]
        out[..., base:base + pf_dim], out[..., base + pf_dim:base + 2 * pf_dim] = blk
    return out.view(R, ldo), bound.view(R, ldo), torch.where(pad, torch.full((), -1.0, dtype=F64), lg).view(R)


# (B, k, dN, dT, dE, pfd, ldo, rows): each width alone at 1; small mixed widths with 4 columns of padding (two readings of the same line);
# 63 / 64 / 65 around a 64-lane trip; the example's widths (2 x 36 pair columns)
TOKEN_WIDTHS = [(2, 3, 1, 0, 0, 0, 1), (2, 3, 0, 1, 0, 0, 1), (2, 3, 0, 0, 1, 0, 1), (2, 3, 0, 0, 0, 1, 2), (6, 8, 5, 4, 4, 4, 25), (3, 5, 6, 8, 5, 4, 31),
                (3, 5, 63, 64, 65, 0, 192), (2, 32, 128, 100, 172, 36, 472)]
TOKEN_CASES = [w + (r,) for w in TOKEN_WIDTHS for r in (0, 1)]
TOKEN_BIG_CASE = (4097, 8, 1, 1, 1, 0, 4, 0)  # 2 B k = 65 552 token rows: 16 past 16 384 blocks x 4 waves
TOKEN_NODES = 30


def token_case(B, k, dN, dT, dE, pfd, ldo, rows, seed=0):
    """Edge times unix-scale, ascending (pair 0 holds the smallest); nbr_t = edge_time[0] - gap with the gaps of the first slots of row 0
    GAPS (1, 0, 2^24 + 1, 2^31 - 1), the rest within 40: sequence 0 reads row 0 and sees exactly those, every other gap is >= 0.  Hop-0 row
    1 is all pads, the last slot of every third row is a pad (nbr_t = 0 and nbr_x NOT zero there), the last slot of row 0 holds an
    id >= num_nodes.  rows: S = 2 B + 3 hop-0 rows, rows[0] = 0, rows[1] = -1, rows[2] = 1, rows[3] = S, the rest random."""
    g = torch.Generator().manual_seed(1000 * seed + 977 * B + 131 * k + 17 * dN + 7 * dT + 3 * dE + pfd + 64 * rows)
    N, Q = TOKEN_NODES, 2 * B
    S = Q + 3 if rows else Q
    edge_time = torch.sort(UNIX + torch.randint(0, 1_000_000, (B,), generator=g)).values
    nids = torch.randint(0, N, (S, k), generator=g, dtype=torch.int32)
    gap = torch.randint(0, 41, (S, k), generator=g)
    gap[0, : min(k, len(GAPS))] = torch.tensor(GAPS)[: min(k, len(GAPS))]
    nids[1] = -1
    nids[torch.arange(S) % 3 == 2, k - 1] = -1
    nids[0, k - 1] = N + 5
    nbr_t = edge_time[0] - gap
    nbr_t[nids == -1] = 0
    r = None
    if rows:
        r = torch.randint(0, S, (Q,), generator=g, dtype=torch.int32)
        r[0], r[1], r[2], r[3] = 0, -1, 1, S
    tw, tb = time2vec_params(dT, g) if dT else (None, None)
    ldpf = pfd + 3
    return dict(node_x=torch.randn(N, dN, generator=g) if dN else None, N=N, edge_time=edge_time, nids=nids, nbr_t=nbr_t,
                nbr_x=torch.randn(S, k, dE, generator=g) if dE else None, S=S, rows=r, tw=tw, tb=tb,
                pf=torch.randn(2 * Q * k, ldpf, generator=g) if pfd else None, ldpf=ldpf, B=B, k=k, dN=dN, dT=dT, dE=dE, pfd=pfd, ldo=ldo)


def token_run(c, dtype=F64, mutate=None):
    return tokens(c['node_x'], c['N'], c['dN'], c['edge_time'], c['B'], c['nids'], c['nbr_t'], c['nbr_x'], c['S'], c['k'], c['dE'], c['rows'], c['tw'],
                  c['tb'], c['dT'], c['pf'], c['pfd'], c['ldo'], dtype, mutate)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tpnet_mean
# ---------------------------------------------------------------------------------------------------------------------------
def token_mean(z, k, dtype=F64, mutate=None, nids=None):
    """out [Q, C] = the mean over the k rows q k .. q k + k - 1 of z [Q k, C] (pads included: TPNet's mean is not masked).  Returns
    (out, sum |z| / k).  nids [Q, k]: only for the mutation that masks."""
    Q, C = z.shape[0] // k, z.shape[1]
    zz = z.to(dtype).view(Q, k, C)
    if mutate == 'mean_over_non_pad_tokens':
        live = (nids != -1)[..., None]
        return (zz * live).sum(1) / live.sum(1).clamp(min=1).to(dtype), zz.double().abs().sum(1) / k
    return zz.sum(1) / k, zz.double().abs().sum(1) / k


def mean_chain(k: int) -> int:
    """tpnet_mean_kernel: k adds and the division."""
    return k + 1


MEAN_CASES = [(1, 1, 1), (3, 7, 5), (2, 32, 172), (5, 20, 130)]  # (Q, k, C), z rows 3 floats wider than C
MEAN_BIG_CASE = (65539, 1, 32)  # Q C = 8192 * 256 + 96: the block cap and a second grid-stride trip for the tail


def mean_case(Q, k, C, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 977 * Q + 131 * k + C)
    nids = torch.randint(0, 9, (Q, k), generator=g, dtype=torch.int32)
    nids[:, : k // 2] = -1
    return dict(z=torch.randn(Q * k, C, generator=g) + 0.3, nids=nids, Q=Q, k=k, C=C, ldz=C + 3, ldo=C + 1)


def mean_bounds(c, dtype=F64, mutate=None):
    v, mag = token_mean(c['z'], c['k'], dtype, mutate, c['nids'])
    return v, (mean_chain(c['k']) + SLACK) * EPS * mag


# ---------------------------------------------------------------------------------------------------------------------------
# deliberately wrong variants: name -> (kernel, the listed case it is shown at)
# ---------------------------------------------------------------------------------------------------------------------------
_PAIR = {(c[0], c[1], c[2], c[9]): c for c in PAIR_CASES}
MUTATIONS = {
    'update_level_read_after_writes': ('update', (100, 50, 130, 2, '')),  # level 2 sees level 1 with this batch's messages in it
    'update_decay_exponent_one': ('update', (100, 50, 130, 2, '')),  # level 2 scaled by decay instead of decay^2
    'update_message_not_decayed': ('update', (100, 50, 130, 2, '')),  # the level-1 row behind a level-2 message
    'update_now_in_edge_weight': ('update', (33, 40, 65, 2, 'float_now')),
    'update_no_dst_to_src': ('update', (12, 15, 63, 1, 'float_now')),
    'update_rows_without_message_not_rescaled': ('update', (33, 40, 65, 2, 'float_now')),  # the node nobody names
    'update_level0_rescaled': ('update', (40, 30, 64, 7, 'times_equal')),
    'update_lost_j64': ('update', (33, 40, 65, 2, 'float_now')),  # the self loop's second contribution
    'update_lost_last': ('update', (100, 50, 130, 2, '')),  # the destination-only node's one contribution
    'update_half_valid_edges_applied': ('update', (32, 40, 16, 2, 'now_is_next')),
    'pair_cross_transposed': ('pair', _PAIR[(3, 0, 65, 0)]),
    'pair_clamp_missing': ('pair', next(c for c in PAIR_CASES if c[3] and c[2] >= 63)),
    'pair_log_not_log1p': ('pair', next(c for c in PAIR_CASES if c[3])),
    'pair_pad_reads_row_0': ('pair', _PAIR[(2, 1, 64, 0)]),
    'pair_b_index_clamped': ('pair', next(c for c in PAIR_CASES if c[7])),
    'pair_second_block_uses_b0': ('pair', next(c for c in PAIR_CASES if c[6])),
    'tokens_time_on_pads': ('tokens', TOKEN_CASES[8]),
    'tokens_pad_node_is_last_row': ('tokens', TOKEN_CASES[8]),
    'tokens_gap_without_plus_one': ('tokens', TOKEN_CASES[2]),  # the gap of 0: log(0)
    'tokens_dst_time_clamped': ('tokens', TOKEN_CASES[8]),
    'tokens_pair_blocks_swapped': ('tokens', TOKEN_CASES[6]),
    'tokens_row_out_of_range_reads_edge_features': ('tokens', TOKEN_CASES[9]),
    'mean_over_non_pad_tokens': ('mean', (3, 7, 5)),
}
