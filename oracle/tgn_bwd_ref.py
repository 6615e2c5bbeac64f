"""ORACLE (test infrastructure only -- never imported by the product path).

float64 restatements of the four entry points of ``csrc/tgn_bwd.hip`` (``tgmx_tgn_gru_gate_backward``,
``tgmx_tgn_aggregate_backward``, ``tgmx_tconv_edge_attr_backward``, ``tgmx_tconv_attend_backward``), pure torch on the CPU, in the
manner of ``oracle/tgat_bwd_ref.py``: every function takes the float32 / int64 tensors the kernel gets and returns ``(value,
magnitude)`` pairs, the value in float64 and, with the same shape, the same formula with every term replaced by its absolute value.
A worst-case rounding bound for a float32 evaluation is ``n * 2^-24 * magnitude`` with ``n`` from the chain helpers below.
``dtype=torch.float32`` evaluates the same formulas in float32 (plain torch).

Magnitudes.  ``|sin|`` counts as 1 (like the TGAT module).  A difference counts as the sum of its terms' magnitudes (``1 - z`` as
``1 + z``, ``1 - n^2`` as ``1 + n^2``, ``h - n`` as ``|h| + |n|``).  A sigmoid, a tanh and a softmax weight are NOT inputs here (in
the TGAT module the weights are): their argument is itself a rounded float32 sum, and the function carries that error on.  To first
order ``f(x (1 + d)) = f(x) + f'(x) x d``, so such a value counts as ``|f(x)| + |f'(x)| * magnitude(x)``:

    sigmoid(a):  s + s (1 - s) |a|_mag          tanh(x):  |n| + (1 - n^2) |x|_mag
    softmax:     alpha_p (1 + s_mag_p + sum_p' alpha_p' s_mag_p')      (d alpha_p = alpha_p (ds_p - sum alpha ds))

Underflow.  float32 keeps no relative precision below its smallest normal 2^-126 (the device may flush such a value to 0; ``expf``
of a score 100 below the maximum IS 0).  A softmax weight therefore counts with ``UNDERFLOW_MAG = 2^-126 / 2^-24`` added to its
magnitude (one eps of it is the underflow threshold); the saturated GRU rows get ``gru_underflow_floor``.

The device's ``expf``, ``tanhf`` and the sine polynomial of ``sin_t2v`` are not correctly rounded.  The ROCm math documentation is
not at hand; ASSUMPTION: each is good to 2 ulp (``common.h`` puts the polynomial at about 1e-7 = 1.7 * 2^-24 absolute on a value
of magnitude 1), and each counts as ``TRANSCENDENTAL_OPS = 4`` operations in a chain.  Division is correctly rounded (hipcc's
default): one operation.

``*_case`` build the rows the tests share (CPU and GPU): they live here so that both see the same rows.
"""
from __future__ import annotations

import torch

from .dropout_ref import dropout_scale
from .tgat_bwd_ref import EPS, F64

TRANSCENDENTAL_OPS = 4
FLT_MIN = 2.0 ** -126
UNDERFLOW_MAG = FLT_MIN / EPS  # 2^-102
NAN = float('nan')


def _fma32(dt32, tw, tb):
    """One fma rounded to float32 (tgat_bwd_ref.time_args: exact product in float64, one sum, rounded): [..., T]."""
    return (dt32.double()[..., None] * tw.double() + tb.double()).to(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tgn_gru_gate_backward
# ---------------------------------------------------------------------------------------------------------------------------
def gru_gate_backward(gi, gh, h, dout, dtype=F64, mutate=None):
    """Backward of the gate arithmetic of ``TGNMemoryRef._gru`` w.r.t. gi, gh [R, 3M] (h [R, M] is a buffer row: no gradient):

        r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n), out = (1 - z) n + z h
        dn = g (1 - z), dz = g (h - n), dan = dn (1 - n^2), dar = dan gh_n r (1 - r), daz = dz z (1 - z)
        dgi = [dar | daz | dan],  dgh = [dar | daz | dan r]

    Returns (dgi, dgh, dgi_mag, dgh_mag)."""
    M = h.shape[1]
    gi, gh, h, g = (t.to(dtype) for t in (gi, gh, h, dout))
    ar, az = gi[:, :M] + gh[:, :M], gi[:, M:2 * M] + gh[:, M:2 * M]
    ar_m, az_m = gi[:, :M].abs() + gh[:, :M].abs(), gi[:, M:2 * M].abs() + gh[:, M:2 * M].abs()
    r, z = torch.sigmoid(ar), torch.sigmoid(az)
    r_m, z_m = r + r * (1 - r) * ar_m, z + z * (1 - z) * az_m
    ghn = gh[:, 2 * M:]
    n = torch.tanh(gi[:, 2 * M:] + r * ghn)
    n_m = n.abs() + (1 - n * n) * (gi[:, 2 * M:].abs() + r_m * ghn.abs())
    dn, dn_m = g * (1 - z), g.abs() * (1 + z_m)
    dz, dz_m = g * (h - n), g.abs() * (h.abs() + n_m)
    dan, dan_m = dn * (1 - n * n), dn_m * (1 + n_m * n_m)
    dar, dar_m = dan * ghn * r * (1 - r), dan_m * ghn.abs() * r_m * (1 + r_m)
    daz, daz_m = dz * z * (1 - z), dz_m * z_m * (1 + z_m)
    dghn, dghn_m = (dan, dan_m) if mutate == 'dgh_n_without_r' else (dan * r, dan_m * r_m)
    return (torch.cat([dar, daz, dan], 1), torch.cat([dar, daz, dghn], 1), torch.cat([dar_m, daz_m, dan_m], 1),
            torch.cat([dar_m, daz_m, dghn_m], 1))


def gru_chain() -> int:
    """float32 operations on the longest chain into an element (dar), plus 8, counted from tgn_gru_gate_backward_kernel:
    rg = add, expf, add, divide (3 + 4);  ng = multiply, add, tanhf (2 + 4);  ng * ng, 1 - ..  (2);  dan = dn * ..  (1);
    dar = dan * ghn * rg * (1 - rg)  (3: the subtraction runs beside the chain).  19 + 8."""
    return 3 + TRANSCENDENTAL_OPS + 2 + TRANSCENDENTAL_OPS + 2 + 1 + 3 + 8


def gru_underflow_floor(*inputs) -> float:
    """The absolute floor of the bound on the saturated rows.  Every output is a product of at most two inputs (|g| and |gh_n|,
    or |g| and |h| + 1 -- with A the largest input magnitude, at most A (A + 1)) with factors in [0, 1]: a sigmoid, its
    complement, 1 - n^2.  float32 keeps no relative precision in a factor below its smallest normal 2^-126 (at +-95 ``expf``
    overflows or lands in the denormals: the factor is exactly 0 where float64 has 5e-42), so the output is uncertain by up to
    2^-126 * A * (A + 1)."""
    A = max(float(t.abs().max()) for t in inputs)
    return FLT_MIN * A * (A + 1.0)


GRU_CASES = [(1, 1), (3, 5), (7, 100)]
GRU_BIG_CASE = (41944, 100)  # 4 194 400 elements = 16384 * 256 + 96: the grid stride takes a second trip for exactly the tail
GRU_BAND = (30.0, -30.0, 95.0, -95.0)


def gru_case(R, M, seed=0):
    """gi, gh [R, 3M], h, dout [R, M]: randn.  R >= 3: rows 1 .. min(4, R - 2) are the saturated band -- gate g of column c of
    row r has gi = gh = v / 2 with v = GRU_BAND[(r + c + g) % 4] (the r and z pre-activations are exactly v = +-30, +-95; n's is
    v / 2 or v as r is 0 or 1), and in row R - 1 h is tanh's float64 value rounded to float32: h == n to machine precision, the
    cancellation in dz.  Returns a dict (gi, gh, h, dout, band: the band's row indices, hn_row or None)."""
    g = torch.Generator().manual_seed(seed * 7919 + R * 331 + M)
    gi, gh = torch.randn(R, 3 * M, generator=g), torch.randn(R, 3 * M, generator=g)
    h, dout = torch.randn(R, M, generator=g), torch.randn(R, M, generator=g)
    band = list(range(1, min(4, R - 2) + 1)) if R >= 3 else []
    col = torch.arange(M)
    for r in band:
        for gate in range(3):
            v = torch.tensor(GRU_BAND)[(r + col + gate) % 4] / 2
            gi[r, gate * M:(gate + 1) * M] = v
            gh[r, gate * M:(gate + 1) * M] = v
    hn_row = R - 1 if R >= 3 else None
    if hn_row is not None:
        a, b = gi[hn_row].double(), gh[hn_row].double()
        h[hn_row] = torch.tanh(a[2 * M:] + torch.sigmoid(a[:M] + b[:M]) * b[2 * M:]).float()
    return dict(gi=gi, gh=gh, h=h, dout=dout, band=band, hn_row=hn_row)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tgn_aggregate_backward, tgmx_tconv_edge_attr_backward
# ---------------------------------------------------------------------------------------------------------------------------
def _t2v_terms(dt32, arg32, g, dtype):
    """[-sin(arg) g dt | -sin(arg) g] per event [n, 2T] and the magnitudes [|g| |dt| | |g|]."""
    gs = -torch.sin(arg32.to(dtype)) * g.to(dtype)
    d = dt32.to(dtype)[:, None]
    return torch.cat([gs * d, gs], -1), torch.cat([g.to(dtype).abs() * d.abs(), g.to(dtype).abs().expand_as(gs)], -1)


def aggregate_backward(row_lo_s, row_cnt_s, row_lo_d, row_cnt_d, row_lu, log_t, M, D, tw, tb, mean, d_aggr, dtype=F64, mutate=None):
    """part [R, 2T]: a row's d(tw) | d(tb) contribution from the Time2Vec columns [2M + D, 2M + D + T) of d_aggr (no other column is
    read).  The walk over a row's events is its source window (log positions lo_s .. lo_s + cnt_s) and THEN its destination
    window.  LAST takes the event with the largest ``log_t.float()``, the first one in walk order on ties: ``torch.argmax``
    semantics on the concatenated walk (torch.argmax returns the first maximal index).  MEAN takes every event and divides the sum
    by the count.  dt = float32(int64 t - lu); arg = one fma rounded to float32; the contribution of an event is
    -sin(arg) g dt for tw and -sin(arg) g for tb.  A row without events gives zeros.  Returns (part, part_mag)."""
    R, T = row_lu.numel(), tw.numel()
    toff = 2 * M + D
    part, mag = torch.zeros(R, 2 * T, dtype=dtype), torch.zeros(R, 2 * T, dtype=dtype)
    for r in range(R):
        c0, c1 = int(row_cnt_s[r]), int(row_cnt_d[r])
        if mutate == 'ignore_destination_window':
            c1 = 0
        pos = torch.cat([int(row_lo_s[r]) + torch.arange(c0), int(row_lo_d[r]) + torch.arange(c1)])
        if pos.numel() == 0:
            continue
        t = log_t[pos]
        if not mean:
            if mutate == 'last_tie_last_wins':
                f = t.float()
                sel = int((f == f.max()).nonzero().max())
            elif mutate == 'last_argmax_int64':
                sel = int(torch.argmax(t))
            else:
                sel = int(torch.argmax(t.float()))
            t = t[sel:sel + 1]
        dt = (t.float() - row_lu[r].float()) if mutate == 'dt_float_first' else (t - row_lu[r]).to(torch.float32)
        v, m = _t2v_terms(dt, _fma32(dt, tw, tb), d_aggr[r, toff:toff + T], dtype)
        cnt = (max(c0, 1) if mutate == 'mean_divides_by_source_count' else pos.numel()) if mean else 1
        part[r], mag[r] = v.sum(0) / cnt, m.sum(0) / cnt
    return part, mag


def aggregate_chain(count, mean: bool):
    """float32 operations on the longest chain into an element of part, plus 8, counted from tgn_aggregate_backward_kernel (the
    argument's fma is reproduced bit for bit by the restatement: not counted).  LAST: sin_t2v (4), * gt, * dt (2): 6 + 8.
    MEAN: the same per event, one accumulating fma / add per event (count) and the division (1): 7 + count + 8."""
    return TRANSCENDENTAL_OPS + 2 + 8 + (1 + count) * int(bool(mean))


def edge_attr_backward(lu_local, src, t, tw, tb, d_attr, D, dtype=F64, mutate=None):
    """part [E, 2T] of edge_attr[e, :T] = cos(fma(dt, tw, tb)), dt = float32(lu_local[src[e]] - t[e]) (subtracted in int64, then
    rounded): -sin(arg) g dt | -sin(arg) g with g = d_attr[e, :T] (the D message columns behind are not read).
    Returns (part, part_mag)."""
    T = tw.numel()
    lu = lu_local[src]
    dt = (lu.float() - t.float()) if mutate == 'dt_float_first' else (lu - t).to(torch.float32)
    return _t2v_terms(dt, _fma32(dt, tw, tb), d_attr[:, :T], dtype)


def edge_attr_chain() -> int:
    """sin_t2v (4), * d_attr, * dt (2), plus 8 (tconv_edge_attr_backward_kernel)."""
    return TRANSCENDENTAL_OPS + 2 + 8


T2V_AXES = dict(T=[1, 64, 65, 100], MD=[(1, 0), (100, 172)])
# (mean, T, M, D): every T with both settings at the small message, the wide message at T = 100 and T = 1
AGGR_CASES = [(mean, T, 1, 0) for T in T2V_AXES['T'] for mean in (0, 1)] + [(mean, T, 100, 172) for T in (1, 100) for mean in (0, 1)]
AGGR_ROWS = 23
AGGR_LOG = 4096
AGGR_NODES = 40
UNIX = 1_700_000_000
# row kinds of aggr_case: name -> row
AGGR_ROW = dict(empty=0, one=1, src_only=2, dst_only=3, dst_below_src=4, total64=5, total65=6, total130=7, max_first=8, max_last=9,
                max_127=10, tie_one_lane=11, tie_lanes=12, tie_windows=13, dt_zero=14, dt_2_31=15, dst_only_70=16, empty_last=22)


def time2vec_params(T, g):
    """tw: the reference Time2Vec's frequencies 10^0 .. 10^-9, tb: small random phases."""
    tw = (1.0 / 10 ** torch.linspace(0, 9, T, dtype=F64)).to(torch.float32)
    return tw, torch.randn(T, generator=g) * 0.1


def aggr_case(T, M, D, seed=0):
    """R = 23 rows over a log of 4096 unix-scale times (1.7e9 + up to 1e6: float32 spacing 128; every window sits at its own
    log positions, the rest of the log is random, so a wrong position reads a wrong time).  Rows by kind (AGGR_ROW):

        0 no events; 1 one event; 2 source window only (5); 3 destination window only (6); 4 both (4 + 7), the destination
        window at LOWER log positions; 5, 6, 7 totals of 64 (30 + 34), 65 (33 + 32), 130 (70 + 60); 8, 9, 10 totals of 130 with
        the maximum at walk index 0, 129 and 127 (lane 63, second trip); 11 a float32 tie at walk indices 5 and 69 (one lane's
        two trips), 12 at 10 and 20 (two lanes), 13 at 7 and 43 = 40 + 3 (source and destination window): the tied times are
        X + 3 and X + 50 with X a multiple of 128 -- the LATER one has the larger int64, and row_lu is within 1000 of X so the two
        dt differ as float32; 14 one event with dt == 0; 15 three events with dt = 2^31 - 1 - j (arguments up to 2.1e9 at
        tw[0] = 1); 16 destination window only, 70 events (second trip with c0 == 0); 17 .. 21 random counts 0 .. 20 per
        window; 22 no events (in the last, ragged group of four).

    d_aggr [R, 2M + D + T] holds NaN outside its Time2Vec columns.  The forward kernel's further inputs (oracle/tgn_fwd_ref.py) come
    from a generator of their own, so the tensors above are what they were without them: N = 40 nodes, ``nodes`` [R] distinct node
    ids in random order (row r is node nodes[r]), ``memory`` [N, M], ``log_other`` [4096] in [0, N), ``log_raw`` [4096, D].
    Returns a dict of CPU tensors."""
    g = torch.Generator().manual_seed(1000 * seed + 31 * T + 7 * M + D)
    R = AGGR_ROWS
    log_t = UNIX + torch.randint(0, 1_000_000, (AGGR_LOG,), generator=g)
    counts = {1: (1, 0), 2: (5, 0), 3: (0, 6), 4: (4, 7), 5: (30, 34), 6: (33, 32), 7: (70, 60), 8: (70, 60), 9: (64, 66), 10: (100, 30),
              11: (100, 30), 12: (25, 15), 13: (40, 20), 14: (1, 0), 15: (2, 1), 16: (0, 70)}
    for r in range(17, 22):
        counts[r] = tuple(int(x) for x in torch.randint(0, 21, (2,), generator=g))
    lo = torch.zeros(2, R, dtype=torch.int64)
    cnt = torch.zeros(2, R, dtype=torch.int32)
    cursor = 17  # (not 0: a kernel that forgot the window offset reads other times)
    for r in range(R):
        c0, c1 = counts.get(r, (0, 0))
        for role in ((1, 0) if r == AGGR_ROW['dst_below_src'] else (0, 1)):
            c = (c0, c1)[role]
            lo[role, r], cnt[role, r] = cursor, c
            cursor += c + 3
    assert cursor <= AGGR_LOG
    walk = lambda r: torch.cat([lo[0, r] + torch.arange(int(cnt[0, r])), lo[1, r] + torch.arange(int(cnt[1, r]))])
    lu = torch.zeros(R, dtype=torch.int64)
    for r in range(R):
        p = walk(r)
        lu[r] = (int(log_t[p].min()) if p.numel() else UNIX) - int(torch.randint(0, 5000, (1,), generator=g))
    top = UNIX + 2_000_000
    for r, idx in ((AGGR_ROW['max_first'], 0), (AGGR_ROW['max_last'], 129), (AGGR_ROW['max_127'], 127)):
        log_t[walk(r)[idx]] = top + 777
    X = (top // 128) * 128
    for r, (i, j) in ((AGGR_ROW['tie_one_lane'], (5, 69)), (AGGR_ROW['tie_lanes'], (10, 20)), (AGGR_ROW['tie_windows'], (7, 43))):
        p = walk(r)
        log_t[p[i]], log_t[p[j]] = X + 3, X + 50
        lu[r] = X - 400 - r
    lu[AGGR_ROW['dt_zero']] = log_t[walk(AGGR_ROW['dt_zero'])[0]]
    p = walk(AGGR_ROW['dt_2_31'])
    lu[AGGR_ROW['dt_2_31']] = UNIX - (2 ** 31 - 1 - 1_000_000)
    log_t[p] = lu[AGGR_ROW['dt_2_31']] + 2 ** 31 - 1 - torch.arange(3)
    tw, tb = time2vec_params(T, g)
    W, toff = 2 * M + D + T, 2 * M + D
    d_aggr = torch.full((R, W), NAN)
    d_aggr[:, toff:toff + T] = torch.randn(R, T, generator=g)
    g2 = torch.Generator().manual_seed(77_000_003 + 1000 * seed + 31 * T + 7 * M + D)
    nodes = torch.randperm(AGGR_NODES, generator=g2)[:R].to(torch.int32)
    memory = torch.randn(AGGR_NODES, M, generator=g2)
    log_other = torch.randint(0, AGGR_NODES, (AGGR_LOG,), generator=g2).to(torch.int32)
    log_raw = torch.randn(AGGR_LOG, D, generator=g2)
    return dict(lo_s=lo[0].clone(), cnt_s=cnt[0].clone(), lo_d=lo[1].clone(), cnt_d=cnt[1].clone(), lu=lu, log_t=log_t, tw=tw, tb=tb,
                d_aggr=d_aggr, R=R, T=T, M=M, D=D, walk=walk, N=AGGR_NODES, nodes=nodes, memory=memory, log_other=log_other, log_raw=log_raw)


def aggr_args(c, mean):
    return (c['lo_s'], c['cnt_s'], c['lo_d'], c['cnt_d'], c['lu'], c['log_t'], c['M'], c['D'], c['tw'], c['tb'], mean, c['d_aggr'])


EDGE_CASES = [(1, 1, 0), (5, 8, 3), (37, 100, 172)]
EDGE_BIG_CASE = (41944, 100, 0)  # E * T = 16384 * 256 + 96: the block cap and a second grid-stride trip for the tail


def edge_case(E, T, D, seed=0):
    """lu_local has 1 row (E <= 5) or 17, src repeats rows; lu and t are near 1.7e9 with lu[src] - t within +-40 (float32 spacing
    there is 128: 'float first' is off by up to 128).  E >= 5: edge 0 has dt == 0, edge 1 dt = 2^31 - 3, edge 2 dt = -(2^31 - 7).
    d_attr [E, T + D] holds NaN in its D message columns.  ``msg`` [E, D], the forward kernel's further input, comes from a generator
    of its own (the tensors above are what they were without it)."""
    g = torch.Generator().manual_seed(1000 * seed + 131 * E + 7 * T + D)
    L = 1 if E <= 5 else 17
    lu = UNIX + torch.randint(0, 1_000_000, (L,), generator=g)
    src = torch.randint(0, L, (E,), generator=g)
    diff = torch.randint(-40, 41, (E,), generator=g)
    if E >= 5:
        diff[0], diff[1], diff[2] = 0, 2 ** 31 - 3, -(2 ** 31 - 7)
    t = lu[src] - diff
    tw, tb = time2vec_params(T, g)
    d_attr = torch.full((E, T + D), NAN)
    d_attr[:, :T] = torch.randn(E, T, generator=g)
    msg = torch.randn(E, D, generator=torch.Generator().manual_seed(77_000_003 + 1000 * seed + 131 * E + 7 * T + D))
    return dict(lu_local=lu, src=src, t=t, tw=tw, tb=tb, d_attr=d_attr, D=D, T=T, E=E, msg=msg)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tconv_attend_backward
# ---------------------------------------------------------------------------------------------------------------------------
def edge_targets(order, seg_lo, seg_hi, E):
    """tgt [E]: the target whose segment order[seg_lo : seg_hi] lists the edge (every edge has exactly one)."""
    tgt = torch.full((E,), -1, dtype=torch.int64)
    for i in range(seg_lo.numel()):
        tgt[order[int(seg_lo[i]):int(seg_hi[i])]] = i
    assert bool((tgt >= 0).all())
    return tgt


def attend_backward(q, k, v, eproj, order, src, seg_lo, seg_hi, H, C, scale, dout, keep, dtype=F64, mutate=None):
    """Backward of out_i = sum_p alpha_p mk_p val_p (TransformerConv's attention, the comment above TconvBwdArgs), per head:

        ke_p = k[j] + e_p, val_p = v[j] + e_p (j = src[e_p]),  s_p = scale q_i . ke_p,  alpha = softmax over the edges into i
        dal_p = dout_i . val_p,  delta = sum_p alpha_p mk_p dal_p,  ds_p = alpha_p (dal_p mk_p - delta) scale
        (the softmax backward acts on the pre-dropout coefficients alpha; mk = keep [E, H] is the dropout mask times 1 / (1 - p))
        dq_i = sum_p ds_p ke_p,  dk_j += ds_p q_i,  dv_j += alpha_p mk_p dout_i,  de_p = ds_p q_i + alpha_p mk_p dout_i

    A target without incoming edges gives dq = 0.  Returns a dict dq, dk, dv [U, H*C], de [E, H*C] and dq_mag .. de_mag."""
    U, E = q.shape[0], eproj.shape[0]
    tgt = edge_targets(order, seg_lo, seg_hi, E)
    q, k, v, e, go, mk = (t.to(dtype) for t in (q, k, v, eproj, dout, keep))
    hc = lambda t: t.view(-1, H, C)
    qe, ge = hc(q)[tgt], hc(go)[tgt]
    ke, ke_m = hc(k)[src] + hc(e), hc(k)[src].abs() + hc(e).abs()
    val, val_m = hc(v)[src] + hc(e), hc(v)[src].abs() + hc(e).abs()
    s, s_m = scale * (qe * ke).sum(-1), scale * (qe.abs() * ke_m).sum(-1)  # [E, H]
    if mutate == 'score_skips_channel_C-1':
        s = scale * (qe * ke)[..., :C - 1].sum(-1)
    idx = tgt[:, None].expand(E, H)
    m = torch.full((U, H), -float('inf'), dtype=dtype).scatter_reduce(0, idx, s, 'amax')
    w = torch.exp(s - m[tgt])
    alpha = w / torch.zeros(U, H, dtype=dtype).index_add_(0, tgt, w)[tgt]
    alpha_m = alpha * (1 + s_m + torch.zeros(U, H, dtype=dtype).index_add_(0, tgt, alpha * s_m)[tgt]) + UNDERFLOW_MAG
    if mutate == 'dropout_head_index_dropped':
        mk = mk[:, :1].expand(E, H)
    dal, dal_m = (ge * val).sum(-1), (ge.abs() * val_m).sum(-1)
    delta = torch.zeros(U, H, dtype=dtype).index_add_(0, tgt, alpha * mk * dal)[tgt]
    delta_m = torch.zeros(U, H, dtype=dtype).index_add_(0, tgt, alpha_m * mk * dal_m)[tgt]
    mk_dal = torch.ones_like(mk) if mutate == 'dropout_on_value_path_only' else mk
    if mutate == 'ds_without_delta':
        delta = torch.zeros_like(delta)
    ds, ds_m = alpha * (dal * mk_dal - delta) * scale, alpha_m * (dal_m * mk_dal + delta_m) * scale
    ad, ad_m = alpha * mk, alpha_m * mk
    flat = lambda t: t.reshape(t.shape[0], H * C)
    z = lambda n: torch.zeros(n, H * C, dtype=dtype)
    dq, dq_m = z(U).index_add_(0, tgt, flat(ds[..., None] * ke)), z(U).index_add_(0, tgt, flat(ds_m[..., None] * ke_m))
    dk, dk_m = z(U).index_add_(0, src, flat(ds[..., None] * qe)), z(U).index_add_(0, src, flat(ds_m[..., None] * qe.abs()))
    dv, dv_m = z(U).index_add_(0, src, flat(ad[..., None] * ge)), z(U).index_add_(0, src, flat(ad_m[..., None] * ge.abs()))
    de = flat(ds[..., None] * qe) if mutate == 'de_without_alpha_dout' else flat(ds[..., None] * qe + ad[..., None] * ge)
    de_m = flat(ds_m[..., None] * qe.abs() + ad_m[..., None] * ge.abs())
    return dict(dq=dq, dk=dk, dv=dv, de=de, dq_mag=dq_m, dk_mag=dk_m, dv_mag=dv_m, de_mag=de_m)


def attend_chain(C: int, L, outdeg=0):
    """float32 operations on the longest chain into an element, plus 8, counted from tconv_attend_backward_kernel for a target
    with L incoming edges (L, outdeg: numbers or tensors):

        s: k + e, q * ke, the wave sum (6 shuffle adds, counted as C: a C-term dot product), * scale                       C + 3
        l: s - mn, expf (1 + 4), then L times (l * corr + w)                                                          C + 2L + 8
        delta: acc like l with w * mk * val (2 more), acc / l, go * .., the wave sum (C)                             2C + 2L + 12
        ds = alpha * (dal * mk - delta) * scale                                                                       2C + 2L + 15
        dq: one fma per edge (L);  de: ds * qi + ad * go (2);  dk, dv: ds * qi (1) and the atomic sum over outdeg
    One figure for all four: 2C + 3L + 16 + outdeg + 8."""
    return 2 * C + 3 * L + 16 + outdeg + 8


def attend_chains(c):
    """Per-row chain lengths for an attend_case: dq [U, 1] (its own segment), de [E, 1] (its target's segment), dk = dv [U, 1]
    (the longest segment among the targets the row feeds, plus its out-degree: the atomic sum)."""
    U, C = c['U'], c['C']
    L = (c['seg_hi'] - c['seg_lo'])
    Le = L[c['tgt']]
    outdeg = torch.zeros(U, dtype=torch.int64).index_add_(0, c['src'], torch.ones_like(c['src']))
    Lk = torch.zeros(U, dtype=torch.int64).scatter_reduce(0, c['src'], Le, 'amax')
    n = lambda L_, o=0: (attend_chain(C, L_, o)).double()[:, None]
    return dict(dq=n(L), de=n(Le), dk=n(Lk, outdeg), dv=n(Lk, outdeg))


ATTEND_AXES = dict(C=[1, 8, 33, 64], H=[1, 2, 3], p=[0.0, 0.1, 0.5])
ATTEND_CASES = [(1, 1, 0.0), (2, 8, 0.1), (3, 33, 0.5), (2, 64, 0.5), (1, 64, 0.1), (3, 8, 0.0)]  # (H, C, p)
ATTEND_U = 11
ATTEND_COUNTS = [0, 1, 2, 64, 65, 300, 12, 0, 5, 3, 0]  # incoming edges per target
ATTEND_HUB_TARGET, ATTEND_HUB_SOURCE, ATTEND_SPREAD_TARGET, ATTEND_LOOP = 5, 7, 6, 9
DROP_SEED = 0x1234ABCD5678


def attend_case(H, C, p, seed=0):
    """U = 11 targets with ATTEND_COUNTS incoming edges (E = 452; targets 0, 7 and 10 have none: an ``hi <= lo`` row in every
    group of four).  Source 7 feeds target 5 all 300 times and targets 3, 4, 8 besides (a long atomic chain into dk / dv row
    7); target 9 has a self loop; the edge list is in random order and ``order`` (the stable sort by target) is no identity.
    Target 6: q = 1 and eproj = a / sqrt(C) in every channel with a from -60 to 60 over its 12 edges -- the scores spread by
    more than 100 and float32's expf gives exactly 0 for the weak ones.  keep [E, H] = dropout_scale(p, DROP_SEED, stream,
    (E, H)); p = 0.5: stream is the first one from 0 for which target 1's single edge is dropped in head 0 (a (target, head)
    whose every edge is dropped).  Returns a dict of CPU tensors."""
    g = torch.Generator().manual_seed(1000 * seed + 97 * H + 13 * C)
    U, HC = ATTEND_U, H * C
    tgt = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(ATTEND_COUNTS)])
    E = tgt.numel()
    src = torch.randint(0, U, (E,), generator=g)
    src[tgt == ATTEND_HUB_TARGET] = ATTEND_HUB_SOURCE
    for t_ in (3, 4, 8):
        src[int((tgt == t_).nonzero()[0])] = ATTEND_HUB_SOURCE
    src[int((tgt == ATTEND_LOOP).nonzero()[0])] = ATTEND_LOOP
    perm = torch.randperm(E, generator=g)
    tgt, src = tgt[perm], src[perm]
    order = torch.sort(tgt, stable=True)[1]
    counts = torch.tensor(ATTEND_COUNTS)
    seg_hi = counts.cumsum(0)
    seg_lo = seg_hi - counts
    q, k, v = (torch.randn(U, HC, generator=g) for _ in range(3))
    eproj, dout = torch.randn(E, HC, generator=g) * 0.5, torch.randn(U, HC, generator=g)
    q[ATTEND_SPREAD_TARGET] = 1.0
    sp = (tgt == ATTEND_SPREAD_TARGET).nonzero()[:, 0]
    eproj[sp] = (torch.linspace(-60, 60, sp.numel()) / C ** 0.5)[:, None].expand(sp.numel(), HC)
    stream = 6
    if p == 0.5:
        e1 = int((tgt == 1).nonzero()[0])
        stream = next(s for s in range(256) if float(dropout_scale(p, DROP_SEED, s, (E, H))[e1, 0]) == 0.0)
    keep = dropout_scale(p, DROP_SEED, stream, (E, H))
    return dict(q=q, k=k, v=v, eproj=eproj, order=order, src=src, seg_lo=seg_lo, seg_hi=seg_hi, H=H, C=C, scale=float(C) ** -0.5, dout=dout,
                keep=keep, tgt=tgt, U=U, E=E, p=p, stream=stream)


def attend_args(c):
    return tuple(c[n] for n in ('q', 'k', 'v', 'eproj', 'order', 'src', 'seg_lo', 'seg_hi', 'H', 'C', 'scale', 'dout', 'keep'))


# ---------------------------------------------------------------------------------------------------------------------------
# the bounds n * 2^-24 * magnitude, per case: one place for the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
def gru_bounds(c):
    """((dgi, dgh), (bound_dgi, bound_dgh)): the saturated band's rows get the underflow floor on top."""
    dgi, dgh, mi, mh = gru_gate_backward(c['gi'], c['gh'], c['h'], c['dout'])
    floor = torch.zeros(c['h'].shape[0], 1, dtype=F64)
    floor[c['band']] = gru_underflow_floor(c['gi'], c['gh'], c['h'], c['dout'])
    n = gru_chain() * EPS
    return (dgi, dgh), (n * mi + floor, n * mh + floor)


def aggr_bounds(c, mean):
    want, mag = aggregate_backward(*aggr_args(c, mean))
    n = torch.tensor([aggregate_chain(int(a) + int(b), mean) for a, b in zip(c['cnt_s'], c['cnt_d'])], dtype=F64)[:, None]
    return want, n * EPS * mag


def edge_bounds(c):
    want, mag = edge_attr_backward(c['lu_local'], c['src'], c['t'], c['tw'], c['tb'], c['d_attr'], c['D'])
    return want, edge_attr_chain() * EPS * mag


def attend_bounds(c):
    """(dict of dq, dk, dv, de, dict of their bounds)."""
    want, n = attend_backward(*attend_args(c)), attend_chains(c)
    return want, {name: n[name] * EPS * want[name + '_mag'] for name in ('dq', 'dk', 'dv', 'de')}


# ---------------------------------------------------------------------------------------------------------------------------
# deliberately wrong variants: name -> (function, the condition under which the mutation can show at a case)
# ---------------------------------------------------------------------------------------------------------------------------
MUTATIONS = {
    # LAST with a float32 tie between distinct int64 times (aggr_case rows 11 - 13): the later, larger one wins instead
    'last_tie_last_wins': ('aggregate', lambda mean=0, **_: not mean),
    'last_argmax_int64': ('aggregate', lambda mean=0, **_: not mean),
    # rows with a destination window: their events vanish (LAST: where the maximum sits there; MEAN: always)
    'ignore_destination_window': ('aggregate', lambda **_: True),
    'mean_divides_by_source_count': ('aggregate', lambda mean=0, **_: bool(mean)),  # rows with c1 > 0
    # float(t) - float(lu): off by up to 128 at unix-scale times (every aggr_case / edge_case is one)
    'dt_float_first': ('aggregate+edge_attr', lambda **_: True),
    'dgh_n_without_r': ('gru', lambda **_: True),
    'ds_without_delta': ('attend', lambda **_: True),  # any target with two or more edges
    'dropout_on_value_path_only': ('attend', lambda p=0.0, **_: p > 0),  # keep is all ones without dropout
    'de_without_alpha_dout': ('attend', lambda **_: True),
    'score_skips_channel_C-1': ('attend', lambda **_: True),  # a lane mask one short (C = 1: every score is 0)
    'dropout_head_index_dropped': ('attend', lambda p=0.0, H=1, **_: p > 0 and H > 1),  # one head has no other index
}
