"""ORACLE (test infrastructure only -- never imported by the product path).

float64 restatements of the seven forward entry points that GraphMixer and DyGFormer inference is made of (``csrc/mixer.hip``,
``csrc/dygformer.hip``, ``csrc/dense.hip``): ``tgmx_mixer_prologue``, ``tgmx_mixer_token`` (and its TPNet twin
``tgmx_tpnet_token_mix``), ``tgmx_mixer_tail``, ``tgmx_layernorm_rows``, ``tgmx_mha_small``, ``tgmx_dygformer_prologue``,
``tgmx_dygformer_tail`` -- pure torch on the CPU, in the manner of ``oracle/tgn_bwd_ref.py``.  Every function takes the float32 / int32 /
int64 tensors the kernel gets and returns ``(value, magnitude)`` pairs: the value in float64 and, with the same shape, the same formula
with every term replaced by its absolute value.  A worst-case rounding bound for a float32 evaluation is ``n * 2^-24 * magnitude`` with
``n`` from the chain helpers below, counted from the kernel code; nothing is tuned on a device result.  ``dtype=torch.float32`` evaluates
the same formulas in float32 (plain torch).  A magnitude of 0 says "exact": gathered features, structural zeros.

Time encodings.  ``dt = float32(int64 seed_t - int64 nbr_t)``, ``arg`` = one fma rounded to float32 (reproduced bit for bit, not counted),
the value is float64 ``cos(arg)`` with magnitude 1.  ASSUMPTION (the project's standing one, ``oracle/tgn_bwd_ref.py``): the device's
``cosf`` / ``erff`` / ``expf`` are good to 2 ulp, and each counts as ``TRANSCENDENTAL_OPS = 4`` operations in a chain.

LayerNorm (``_layernorm``: the token LayerNorm over K, the channel LayerNorm over C, ``layernorm_rows``).  Its outputs are not inputs
of a rounding chain: ``y = (x - mean) rstd g + b`` amplifies the error of ``x - mean`` by ``rstd <= 1 / sqrt(eps)`` (316).  With Z the
magnitude of x (|x| for an exact input, more where x itself carries error: the channel LayerNorm of z1) and first-order sensitivities
``dy = g rstd (dx - mean(dx) - xhat mean(xhat dx))``:

    |y|_mag = |g| rstd (Z + mean(Z) (1 + so) + |xhat| mean(|xhat| Z)) + |b|

``mean(Z)`` is what the subtraction can lose to the mean's rounding; the last term is rstd's own sensitivity (it also covers the
variance's rounding: mean(xhat^2) <= 1).  ``so = |xhat| rstd n 2^-24 mean(Z) / 2`` is the one second-order term that ``1 / sqrt(eps)``
can make visible: an error D in the mean adds D^2 to the variance.  A constant row or column is exactly ``b`` in float64, but a plain
float32 kernel may be off by ``rstd K 2^-24 |x|``: the magnitude says so (``rstd mean(Z)`` stays).  K = 1 gives ``b`` on the device too
(the sum of one value divided by 1 is exact); the bound does not use that.

``tgmx_tpnet_token_mix`` (``kRefine``) claims more: on a column of K equal values the corrected mean is that value bit for bit, so the
normalised column is exactly ``tbeta``.  ``mixer_token(refine=True)`` restates that claim: such a column's LayerNorm magnitude is
``|tbeta|`` alone, with no ``1 / sqrt(eps)`` term; on every other column the refined kernel gets the plain bound with a longer chain.

Softmax (``mha_small``): ``alpha (1 + s_mag + sum alpha s_mag) + UNDERFLOW_MAG``, the formula of ``oracle/tgn_bwd_ref.py``.  The GEMM
inside ``tgmx_dygformer_tail`` is judged by ``gemm_bar(D)``, the project's own bar.

``*_case`` build the rows the tests share (CPU and GPU); ``MUTATIONS`` lists deliberately wrong variants and where each can show.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from .tgat_bwd_ref import EPS, F64, gemm_bar
from .tgn_bwd_ref import TRANSCENDENTAL_OPS, UNDERFLOW_MAG, UNIX, _fma32, time2vec_params

SLACK = 8  # the project's "plus 8" on every chain
LN_EPS = 1e-5
GAPS = (1, 0, 2 ** 24 + 1, 2 ** 31 - 1)  # seed_t - nbr_t of the first slots of every time case
AWKWARD = (0.1, 1.0 / 3.0, -7.3e-5, 3.7)  # constant columns / rows of the device cases (test_fwd_blocks_ref_cpu.py tries more)


def _dt(seed_t, nbr_t, mutate=None):
    return (seed_t.float() - nbr_t.float()) if mutate == 'dt_float_first' else (seed_t - nbr_t).to(torch.float32)


def time_enc(dt32, tw, tb, dtype=F64):
    """cos(fma(dt, tw, tb)) [..., T] and its magnitude 1."""
    v = torch.cos(_fma32(dt32, tw, tb).to(dtype))
    return v, torch.ones_like(v)


def time_chain() -> int:
    """mixer_prologue_kernel / dyg_prologue_kernel: the fma is reproduced bit for bit, cosf (4), plus 8."""
    return TRANSCENDENTAL_OPS + SLACK


def unix_times(n, g):
    """n unix-scale int64 seed times (float32 spacing 128 there)."""
    return UNIX + torch.randint(0, 1_000_000, (n,), generator=g)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_mixer_prologue
# ---------------------------------------------------------------------------------------------------------------------------
def mixer_prologue(edge_x, seed_t, nbr_t, K, D, tw, tb, ldo, dtype=F64, mutate=None):
    """out [S K, ldo] = [edge_x | cos(fma(float32(seed_t[r / K] - nbr_t[r]), tw, tb)) | 0]: edge_x [S K, D] (None with D = 0), seed_t
    [S], nbr_t [S K].  The kernel writes every column up to ldo.  Returns (out, out_mag): the copied and the zero columns have
    magnitude 0 (exact)."""
    R, T = nbr_t.numel(), tw.numel()
    out, mag = torch.zeros(R, ldo, dtype=dtype), torch.zeros(R, ldo, dtype=dtype)
    if D:
        out[:, :D] = edge_x.to(dtype)
    out[:, D:D + T], mag[:, D:D + T] = time_enc(_dt(seed_t.repeat_interleave(K), nbr_t.reshape(-1), mutate), tw, tb, dtype)
    return out, mag


PROLOGUE_CASES = [(1, 1, 0, 1, 1), (3, 5, 13, 7, 20), (2, 3, 4, 5, 16), (7, 20, 172, 100, 272)]  # (S, K, D, T, ldo)
PROLOGUE_BIG_CASE = (65539, 4, 3, 5, 8)  # S K ldo = 8192 * 256 + 96: the block cap and a second grid-stride trip for the tail


def prologue_case(S, K, D, T, ldo, seed=0):
    """seed_t unix-scale; the gaps of the first slots are GAPS (1, 0, 2^24 + 1, 2^31 - 1), slot 4 is a pad (nbr_t = 0: the gap is the
    seed time itself), the rest within 40 of the seed time ('float first' is off by up to 128 there)."""
    g = torch.Generator().manual_seed(1000 * seed + 131 * S + 17 * K + 7 * D + T)
    seed_t = unix_times(S, g)
    gap = torch.randint(0, 41, (S * K,), generator=g)
    gap[: len(GAPS)] = torch.tensor(GAPS)[: S * K]
    nbr_t = seed_t.repeat_interleave(K) - gap
    if S * K > len(GAPS):
        nbr_t[len(GAPS)] = 0
    tw, tb = time2vec_params(T, g)
    return dict(edge_x=torch.randn(S * K, D, generator=g) if D else None, seed_t=seed_t, nbr_t=nbr_t, tw=tw, tb=tb, S=S, K=K, D=D, T=T, ldo=ldo)


def prologue_bounds(c, dtype=F64, mutate=None):
    want, mag = mixer_prologue(c['edge_x'], c['seed_t'], c['nbr_t'], c['K'], c['D'], c['tw'], c['tb'], c['ldo'], dtype, mutate)
    return want, time_chain() * EPS * mag.double()


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm, shared by tgmx_mixer_token and tgmx_layernorm_rows
# ---------------------------------------------------------------------------------------------------------------------------
def _layernorm(x, Z, g, b, eps, n, mutate=None, refine=False, exact_const=False):
    """LayerNorm over the last dimension (biased variance) of x with magnitude Z; g, b broadcast against it.  ``n``: the chain length the
    caller will multiply the magnitude with (the second-order term needs it).  ``refine``: one correction step on the mean, as
    mixer_token_kernel<true> has it.  ``exact_const``: a constant row gets the magnitude |b| (the kRefine claim).  Returns (y, y_mag)."""
    K = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    if refine:
        mean = mean + (x - mean).mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    if mutate == 'ln_unbiased_variance':
        var = var * (K / max(K - 1, 1))
    rstd = 1.0 / torch.sqrt(var + (0.0 if mutate == 'ln_without_eps' else eps))
    xhat = d * rstd
    y = xhat * g + b
    shift = Z.mean(-1, keepdim=True)
    so = 0.5 * xhat.abs() * rstd * (n * EPS) * shift
    mag = g.abs() * rstd * (Z + shift * (1 + so) + xhat.abs() * (xhat.abs() * Z).mean(-1, keepdim=True)) + b.abs()
    if exact_const:
        mag = torch.where((x == x[..., :1]).all(-1, keepdim=True), b.abs().expand_as(mag), mag)
    return y, mag


def wave_ln_chain(C: int) -> int:
    """One wave per row (pass 2 of mixer_token_kernel, layernorm_rows_kernel), L = ceil(C / 64) columns per lane: the mean is L adds, 6
    shuffle adds and a division (L + 7); x - mean (1); the variance L fmas, 6 shuffle adds, a division and ``+ eps`` (L + 8); sqrtf
    and the reciprocal (2); ``* rstd * g + b`` (3).  2 L + 21."""
    return 2 * ((C + 63) // 64) + 21


def token_chain(K: int, Ht: int, refine: bool = False) -> int:
    """float32 operations into an element of z1, counted from pass 1 of mixer_token_kernel, plus 8: the column mean is K adds and a
    division (K + 1); kRefine: K subtractions and adds, a division, an add more (2 K + 2); x - mean (1); the variance K fmas, a
    division, ``+ eps`` (K + 2); sqrtf and the reciprocal (2); ``* rstd * tg + tbeta`` (3); the first Linear K fmas and ``+ b1`` (K + 1);
    gelu_erf a multiply, erff, ``1 +``, ``0.5 v``, a multiply (4 + 4); the second Linear Ht fmas, ``+ b2``, ``+=`` (Ht + 2).
    3 K + Ht + 20 (+ 2 K + 2) + 8.  Ht = 0 runs neither Linear nor the GELU; the same figure is an upper bound."""
    return 3 * K + Ht + 16 + TRANSCENDENTAL_OPS + (2 * K + 2) * int(bool(refine)) + SLACK


def _gelu(a, mutate=None):
    """(gelu(a), |gelu'(a)|): exact erf; gelu'(a) = Phi(a) + a phi(a)."""
    d = 0.5 * (1 + torch.erf(a * 0.7071067811865476)) + a * torch.exp(-0.5 * a * a) * 0.3989422804014327
    return F.gelu(a, approximate='tanh' if mutate == 'gelu_tanh_approx' else 'none'), d.abs()


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_mixer_token / tgmx_tpnet_token_mix
# ---------------------------------------------------------------------------------------------------------------------------
def mixer_token(x, tg, tbeta, w1, b1, w2, b2, cg, cb, eps=LN_EPS, refine=False, dtype=F64, mutate=None):
    """x [S, K, C]; tg, tbeta, b2 [K]; w1 [Ht, K], b1 [Ht], w2 [K, Ht] (None with Ht = 0); cg, cb [C].

        z1 = x + (W2 gelu(W1 LN_K(x) + b1) + b2) along the K tokens of every channel,  y = LN_C(z1)

    Returns (z1, y, z1_mag, y_mag) [S, K, C]."""
    S, K, C = x.shape
    Ht = 0 if w1 is None else w1.shape[0]
    n_all = token_chain(K, Ht, refine) + wave_ln_chain(C)
    p = lambda t: None if t is None else t.to(dtype)
    xx, tg, tbeta, w1, b1, w2, b2, cg, cb = (p(t) for t in (x, tg, tbeta, w1, b1, w2, b2, cg, cb))
    col = xx.transpose(1, 2)  # [S, C, K]
    xn, xn_mag = _layernorm(col, col.abs(), tg, tbeta, eps, n_all, mutate, refine=refine, exact_const=refine)
    if Ht:
        a, a_mag = xn @ w1.t() + b1, xn_mag @ w1.abs().t() + b1.abs()
        h, dh = _gelu(a, mutate)
        h_mag = h.abs() + dh * a_mag
        o, o_mag = h @ w2.t(), h_mag @ w2.abs().t()
    else:
        o, o_mag = torch.zeros_like(col), torch.zeros_like(col)
    upd, upd_mag = (o + b2).transpose(1, 2), (o_mag + b2.abs()).transpose(1, 2)
    if mutate == 'token_skips_channel_128':
        upd = upd.clone()
        upd[:, :, 128:129] = 0
    z1, z1_mag = xx + upd, xx.abs() + upd_mag
    y, y_mag = _layernorm(z1, z1_mag, cg, cb, eps, n_all, mutate)
    if mutate == 'token_skips_last_token_when_K_odd' and K % 2:
        z1, y = z1.clone(), y.clone()
        z1[:, K - 1], y[:, K - 1] = 0, 0
    return z1, y, z1_mag, y_mag


# (S, K, C, Ht): C on both sides of a 64-lane trip and of the 128-channel chunk, K = 1 (variance 0), odd and even K around the two
# waves of pass 2, Ht = 0 (w1 = NULL), 1, K / 2 and 39 > K; the last one fills the 64 KiB of LDS to 16 380 floats
TOKEN_CASES = [(1, 1, 1, 0), (1, 1, 65, 1), (1, 2, 63, 1), (3, 2, 128, 1), (1, 5, 1, 2), (3, 5, 65, 2), (1, 5, 257, 0), (3, 20, 127, 10),
               (1, 20, 128, 10), (3, 20, 129, 10), (1, 20, 257, 10), (3, 30, 63, 15), (1, 30, 129, 39), (2, 20, 627, 10)]
TOKEN_UNSUPPORTED_CASE = (2, 20, 628, 10)  # 4 * (20 * 628 + 30 * 128) = 65 600 bytes


def token_lds_floats(K, C, Ht):
    return K * C + (K + Ht) * 128


def token_case(S, K, C, Ht, seed=0):
    """x randn.  The LAST seed's channels c = 1, 3, 5 (mod 7) are special columns: K equal awkward values (AWKWARD in turn); offset 1e4
    with spread 1; spread 0.01 around 0 (the variance is of eps's size: LayerNorm without eps shows there).  Every other seed is
    randn throughout.  Parameters: LayerNorm weights 1 +- 0.1, biases 0.1 randn, Linear weights randn / sqrt(fan_in)."""
    g = torch.Generator().manual_seed(1000 * seed + 977 * S + 131 * K + 7 * C + Ht)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(S, K, C)
    ch = torch.arange(C)
    for i, c in enumerate(ch[ch % 7 == 1].tolist()):
        x[S - 1, :, c] = AWKWARD[i % len(AWKWARD)]
    x[S - 1][:, ch % 7 == 3] += 1e4
    x[S - 1][:, ch % 7 == 5] *= 0.01
    return dict(x=x, tg=1 + 0.1 * r(K), tbeta=0.1 * r(K), w1=r(Ht, K) / K ** 0.5 if Ht else None, b1=0.1 * r(Ht) if Ht else None,
                w2=r(K, Ht) / Ht ** 0.5 if Ht else None, b2=0.1 * r(K), cg=1 + 0.1 * r(C), cb=0.1 * r(C), S=S, K=K, C=C, Ht=Ht,
                const_cols=(ch % 7 == 1))


def token_args(c):
    return tuple(c[n] for n in ('x', 'tg', 'tbeta', 'w1', 'b1', 'w2', 'b2', 'cg', 'cb'))


def token_bounds(c, refine=False, dtype=F64, mutate=None):
    """((z1, y), (bound_z1, bound_y)); refine: the constant columns carry the tighter claim."""
    z1, y, m1, my = mixer_token(*token_args(c), refine=refine, dtype=dtype, mutate=mutate)
    n = token_chain(c['K'], c['Ht'], refine)
    return (z1, y), (n * EPS * m1.double(), (n + wave_ln_chain(c['C'])) * EPS * my.double())


def refined_mean_f32(v, K):
    """mixer_token_kernel<true>'s column mean of K copies of float32(v), operation by operation in float32: (mean, plain mean)."""
    v = np.float32(v)
    s = np.float32(0)
    for _ in range(K):
        s = np.float32(s + v)
    mean0 = np.float32(s / np.float32(K))
    rest = np.float32(0)
    for _ in range(K):
        rest = np.float32(rest + np.float32(v - mean0))
    return np.float32(mean0 + np.float32(rest / np.float32(K))), mean0


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_mixer_tail
# ---------------------------------------------------------------------------------------------------------------------------
def mixer_tail(z, nbr_nids, node_x, tg_nbr, tg_lo, tg_cnt, seeds, ldo, dtype=F64, mutate=None):
    """out [S, ldo] = [mean of z [S, K, C] over the slots with nbr_nids != -1 (0 without one) | mean of node_x over the seed's time-gap
    run tg_nbr[lo : lo + cnt] (0 when cnt == 0) + node_x[seed] | 0].  Returns (out, out_mag); the magnitude is 0 (exact) for a link
    mean without a valid slot, for the node part of a seed with cnt == 0 and for the columns past C + F."""
    S, K, C = z.shape
    Fd = node_x.shape[1]
    valid = (nbr_nids != -1)[:, :, None]
    zz = z.to(dtype) if mutate == 'tail_sums_pad_rows' else torch.where(valid, z.to(dtype), torch.zeros((), dtype=dtype))
    den = torch.full((S, 1), float(K), dtype=dtype) if mutate == 'tail_counts_pads_in_denominator' else valid.sum(1).clamp(min=1).to(dtype)
    out, mag = torch.zeros(S, ldo, dtype=dtype), torch.zeros(S, ldo, dtype=dtype)
    out[:, :C], mag[:, :C] = zz.sum(1) / den, zz.abs().sum(1) / den
    nx = node_x.to(dtype)
    for i in range(S):
        cnt = int(tg_cnt[i])
        own = nx[int(seeds[i])]
        use = cnt - cnt % 4 if mutate == 'timegap_drops_entries_past_multiple_of_4' else cnt
        if cnt == 0:
            out[i, C:C + Fd] = own
            continue
        rows = nx[tg_nbr[int(tg_lo[i]):int(tg_lo[i]) + use].long()]
        div = K if mutate == 'timegap_divides_by_K' else cnt
        out[i, C:C + Fd], mag[i, C:C + Fd] = rows.sum(0) / div + own, rows.abs().sum(0) / div + own.abs()
    return out, mag


def tail_chains(c):
    """[S, ldo] chain lengths, counted from mixer_tail_kernel, plus 8: the link mean is K adds and a division (K + 1); the node part is
    ceil(cnt / 4) adds per wave (kTailWaves = 4), 3 adds across the waves, a division and ``+ node_x[seed]`` (ceil(cnt / 4) + 5)."""
    n = torch.full((c['S'], c['ldo']), float(c['K'] + 1 + SLACK), dtype=F64)
    n[:, c['C']:] = ((c['tg_cnt'].double() / 4).ceil() + 5 + SLACK)[:, None]
    return n


TAIL_SEEDS, TAIL_K, TAIL_NODES = 9, 5, 50
TAIL_CNT = [0, 1, 3, 4, 5, 300, 1000, 2, 7]  # tg_cnt per seed
TAIL_VALID = [0, 1, 5, 3, 2, 5, 0, 4, 1]     # valid slots per seed (the pads in front, as the sampler leaves them)
# (C, F, ldo - C - F, (n0, n1)): the 256-thread stride over C, the 64-lane chunks of F, the tail columns, the seed groups
TAIL_CASES = [(1, 1, 0, (9, 0)), (255, 64, 7, (0, 0)), (256, 65, 0, (3, 2)), (257, 100, 7, (9, 0)), (1, 100, 7, (0, 0)), (257, 1, 0, (3, 2)),
              (256, 64, 7, (4, 5)), (255, 65, 0, (0, 9))]


def tail_case(C, Fd, pad, split, seed=0):
    """S = 9 seeds, K = 5 slots.  Pad slots hold id -1 and a z row of 1e30 (it must not reach the mean).  The time-gap runs sit at
    their own offsets in tg_nbr with three foreign entries between them.  seeds is cut into the groups (n0, n1, S - n0 - n1)."""
    g = torch.Generator().manual_seed(1000 * seed + 131 * C + 7 * Fd + pad)
    S, K, N = TAIL_SEEDS, TAIL_K, TAIL_NODES
    z = torch.randn(S, K, C, generator=g)
    nids = torch.randint(0, N, (S, K), generator=g, dtype=torch.int32)
    for i, v in enumerate(TAIL_VALID):
        nids[i, : K - v] = -1
        z[i, : K - v] = 1e30
    cnt = torch.tensor(TAIL_CNT, dtype=torch.int32)
    lo = torch.zeros(S, dtype=torch.int32)
    cursor = 5
    for i in range(S):
        lo[i] = cursor
        cursor += int(cnt[i]) + 3
    tg_nbr = torch.randint(0, N, (cursor,), generator=g, dtype=torch.int32)
    seeds = torch.randint(0, N, (S,), generator=g, dtype=torch.int32)
    return dict(z=z, nids=nids, node_x=torch.randn(N, Fd, generator=g), tg_nbr=tg_nbr, tg_lo=lo, tg_cnt=cnt, seeds=seeds, S=S, K=K, C=C, F=Fd,
                ldo=C + Fd + pad, split=split)


def tail_bounds(c, dtype=F64, mutate=None):
    want, mag = mixer_tail(c['z'], c['nids'], c['node_x'], c['tg_nbr'], c['tg_lo'], c['tg_cnt'], c['seeds'], c['ldo'], dtype, mutate)
    return want, tail_chains(c) * EPS * mag.double()


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_layernorm_rows
# ---------------------------------------------------------------------------------------------------------------------------
def layernorm_rows(x, g, b, eps=LN_EPS, dtype=F64, mutate=None):
    """y [R, d] = LayerNorm over the d columns.  Returns (y, y_mag)."""
    xx = x.to(dtype)
    return _layernorm(xx, xx.abs(), g.to(dtype), b.to(dtype), eps, wave_ln_chain(x.shape[1]) + SLACK, mutate)


LN_ROWS_CASES = [(1, 1), (2, 63), (5, 64), (37, 65), (5, 200), (37, 512), (2, 512), (1, 200), (5, 1)]  # (R, d)


def ln_rows_case(R, d, seed=0):
    """Rows r = 1, 2, 3 (mod 5): constant (AWKWARD in turn); offset 1e4 with spread 1; spread 0.01 around 0.  The rest randn."""
    gen = torch.Generator().manual_seed(1000 * seed + 131 * R + d)
    x = torch.randn(R, d, generator=gen)
    for r in range(R):
        if r % 5 == 1:
            x[r] = AWKWARD[(r // 5) % len(AWKWARD)]
        elif r % 5 == 2:
            x[r] += 1e4
        elif r % 5 == 3:
            x[r] *= 0.01
    return dict(x=x, g=1 + 0.1 * torch.randn(d, generator=gen), b=0.1 * torch.randn(d, generator=gen), R=R, d=d)


def ln_rows_bounds(c, dtype=F64, mutate=None):
    want, mag = layernorm_rows(c['x'], c['g'], c['b'], dtype=dtype, mutate=mutate)
    return want, (wave_ln_chain(c['d']) + SLACK) * EPS * mag.double()


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_mha_small
# ---------------------------------------------------------------------------------------------------------------------------
def mha_scale(dh: int) -> float:
    """1.f / sqrtf((float)dh) as the launcher computes it, in float32."""
    return float(np.float32(1.0) / np.sqrt(np.float32(dh)))


def mha_small(qkv, H, dh, scale=None, dtype=F64, mutate=None):
    """qkv [B, T, 3 H dh] packed [q | k | v], head h in columns [h dh, (h + 1) dh) of each: out [B, T, H dh] = softmax(scale q k^T) v per
    (sequence, head).  Returns (out, out_mag)."""
    B, T = qkv.shape[:2]
    D = H * dh
    scale = mha_scale(dh) if scale is None else scale
    if mutate == 'mha_scale_missing':
        scale = 1.0
    heads = lambda t: t.reshape(B, T, H, dh).transpose(1, 2).to(dtype)  # [B, H, T, dh]
    q, k, v = (heads(qkv[..., i * D:(i + 1) * D]) for i in range(3))
    if mutate == 'mha_head_offset_dropped':
        q, k, v = (t[:, :1].expand(B, H, T, dh) for t in (q, k, v))
    if mutate == 'mha_scores_include_pad_columns':
        padrows = torch.zeros(B, H, (-T) % 16, dh, dtype=dtype)
        k, v = torch.cat([k, padrows], 2), torch.cat([v, padrows], 2)
    s, s_mag = scale * (q @ k.transpose(-1, -2)), scale * (q.abs() @ k.abs().transpose(-1, -2))
    alpha = torch.softmax(s, -1)
    alpha_mag = alpha * (1 + s_mag + (alpha * s_mag).sum(-1, keepdim=True)) + UNDERFLOW_MAG
    back = lambda t: t.transpose(1, 2).reshape(B, T, D)
    return back(alpha @ v), back(alpha_mag @ v.abs())


def mha_chain(T: int, dh: int) -> int:
    """Counted from mha_small_kernel, plus 8: the score's MFMA chain over the head dimension (dh), ``* scale`` (1), ``- m`` and expf
    (1 + 4), the row sum over the ceil(T / 16) score tiles of a lane and 4 shuffle adds, the division (1), the MFMA chain over the T
    keys of P V (T)."""
    return dh + 1 + 1 + TRANSCENDENTAL_OPS + (T + 15) // 16 + 4 + 1 + T + SLACK


# (B, T, H, dh): one token; T on both sides of a 16-row score tile; more than four tiles; past 64 KiB of LDS; the whole envelope
MHA_CASES = [(1, 1, 1, 1), (2, 15, 1, 3), (2, 16, 2, 4), (2, 17, 3, 5), (3, 64, 2, 32), (2, 65, 1, 128), (2, 100, 2, 100), (2, 128, 1, 128),
             (1, 128, 3, 33)]
MHA_UNSUPPORTED_CASES = [(1, 129, 1, 4), (1, 4, 1, 129)]


def mha_case(B, T, H, dh, seed=0):
    """qkv randn.  T >= 2: the query of token 1 of sequence 0 is all zeros (every score equal: the weights are 1 / T); the key of
    token T - 1 of the last sequence is lined up with the query of its token 0 for a score of 200 in every head (the other weights of
    that row underflow in float32)."""
    g = torch.Generator().manual_seed(1000 * seed + 977 * B + 131 * T + 7 * H + dh)
    D = H * dh
    qkv = torch.randn(B, T, 3 * D, generator=g)
    if T >= 2:
        qkv[0, 1, :D] = 0
        q0 = qkv[B - 1, 0, :D].view(H, dh).double()
        qkv[B - 1, T - 1, D:2 * D] = (q0 * (200.0 / mha_scale(dh)) / (q0 * q0).sum(-1, keepdim=True)).reshape(D).float()
    return dict(qkv=qkv, B=B, T=T, H=H, dh=dh)


def mha_bounds(c, dtype=F64, mutate=None):
    want, mag = mha_small(c['qkv'], c['H'], c['dh'], dtype=dtype, mutate=mutate)
    return want, mha_chain(c['T'], c['dh']) * EPS * mag.double()


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_dygformer_prologue
# ---------------------------------------------------------------------------------------------------------------------------
def dygformer_prologue(node_x, src, dst, edge_time, nbr_nids, nbr_t, nbr_x, S, k, src_rows, dst_rows, tw, tb, ldn, lde, ldt, dtype=F64, mutate=None):
    """Sequence q = 2 p + side (0 = the pair's source, 1 = its destination), slot j of it at row q L + j, L = k + 1.  Slot 0 is the seed
    itself, slot j > 0 the sampler's slot j - 1 of row src_rows[p] / dst_rows[p] (None: rows p and P + p); a row outside [0, S) makes
    the whole sequence pads.  node [2 P L, ldn]: node_x[id] for 0 <= id < num_nodes, else 0.  edge [2 P L, lde]: nbr_x of the slot as
    the sampler wrote it (slot 0 and pad sequences: 0).  time [2 P L, ldt]: cos(fma(dt, tw, tb)) with dt = 0 for slot 0 and
    float32(edge_time[p] - nbr_t[slot]) else, 0 where id == -1 (an id >= num_nodes still gets its time encoding).  Columns past
    dN / dE / dT are 0.  Returns (node, edge, time, time_mag): node and edge are exact."""
    P, N, dN = src.numel(), node_x.shape[0], node_x.shape[1]
    dE, dT, L = (nbr_x.shape[2] if nbr_x is not None else 0), tw.numel(), k + 1
    q = torch.arange(2 * P)
    p, side = q >> 1, (q & 1).bool()
    seed = torch.where(side, dst[p], src[p]).long()
    row = torch.where(side, P + p, p) if src_rows is None else torch.where(side, dst_rows[p], src_rows[p]).long()
    ok = (row >= 0) & (row < S)
    rowc = row.clamp(0, max(S - 1, 0))
    ids = torch.full((2 * P, L), -1, dtype=torch.int64)
    ids[:, 0] = seed
    edge = torch.zeros(2 * P, L, lde, dtype=dtype)
    dt = torch.zeros(2 * P, L, dtype=torch.float32)
    if k and S:
        ids[:, 1:] = torch.where(ok[:, None], nbr_nids[rowc].long(), torch.full((), -1, dtype=torch.int64))
        edge[:, 1:, :dE] = torch.where(ok[:, None, None], nbr_x[rowc].to(dtype), torch.zeros((), dtype=dtype))
        dt[:, 1:] = torch.where(ok[:, None], _dt(edge_time[p][:, None], nbr_t[rowc], mutate), torch.zeros(()))
    inside = (ids >= 0) & ((ids < N) if mutate != 'dyg_node_feature_for_id_out_of_range' else torch.ones_like(ids, dtype=torch.bool))
    node = torch.zeros(2 * P, L, ldn, dtype=dtype)
    node[..., :dN] = node_x.to(dtype)[ids.clamp(0, N - 1)] * inside[..., None]
    has = (ids != -1) if mutate != 'dyg_time_for_pad_id' else torch.ones_like(ids, dtype=torch.bool)
    time, tmag = torch.zeros(2 * P, L, ldt, dtype=dtype), torch.zeros(2 * P, L, ldt, dtype=dtype)
    v, m = time_enc(dt, tw, tb, dtype)
    time[..., :dT], tmag[..., :dT] = v * has[..., None], m * has[..., None]
    flat = lambda t: t.reshape(2 * P * L, -1)
    return flat(node), flat(edge), flat(time), flat(tmag)


DYG_WIDTHS = [(1, 1, 1, 4, 4, 4), (6, 5, 8, 8, 8, 8), (128, 172, 100, 128, 172, 100)]  # (dN, dE, dT, ldn, lde, ldt)
# (P, k, widths, rows given): P = 3, k = 7 with identity rows and with row indices; k = 0 with NULL neighbour pointers
DYG_PROLOGUE_CASES = [(3, 7, w, rows) for w in DYG_WIDTHS for rows in (False, True)] + [(3, 0, DYG_WIDTHS[1], False)]
DYG_PROLOGUE_BIG_CASE = (87384, 1, (4, 4, 4, 4, 4, 4), False)  # 2 P L W = 16384 * 256 + 128: the block cap and a second trip
DYG_NODES = 40


def dyg_prologue_case(P, k, widths, rows_given, seed=0):
    """Unix-scale edge times; the first slots' gaps are GAPS, the rest within 40 (of the time of pair ``row % P``: identity rows measure
    from their own pair, given rows may belong to another one, a gap of up to 1e6 more).  Small cases (P <= 8): slot k - 2 of every row
    and the whole last row hold id -1 (pad slots: nbr_t = 0, and nbr_x NOT zero there: the edge channel copies what the sampler wrote),
    two slots hold ids >= num_nodes; rows given: S = 5 sampler rows, src_rows = [4, -1, 2], dst_rows = [0, S, 3] (a row index of -1
    and one of S: all pads).  k = 0: no neighbour tensors at all."""
    dN, dE, dT, ldn, lde, ldt = widths
    g = torch.Generator().manual_seed(1000 * seed + 131 * P + 17 * k + 7 * dN + int(rows_given))
    N = DYG_NODES
    S = 5 if rows_given else 2 * P
    src, dst = (torch.randint(0, N, (P,), generator=g, dtype=torch.int32) for _ in range(2))
    edge_time = unix_times(P, g)
    c = dict(node_x=torch.randn(N, dN, generator=g), src=src, dst=dst, edge_time=edge_time, nids=None, nbr_t=None, nbr_x=None, S=S, k=k,
             src_rows=None, dst_rows=None, P=P, widths=widths, N=N)
    c['tw'], c['tb'] = time2vec_params(dT, g)
    if rows_given:
        c['src_rows'], c['dst_rows'] = torch.tensor([4, -1, 2], dtype=torch.int32), torch.tensor([0, S, 3], dtype=torch.int32)
    if k:
        nids = torch.randint(0, N, (S, k), generator=g, dtype=torch.int32)
        gap = torch.randint(0, 41, (S, k), generator=g)
        nbr_x = torch.randn(S, k, dE, generator=g)
        if P <= 8:
            gap.view(-1)[: len(GAPS)] = torch.tensor(GAPS)
            nids[:, k - 2] = -1
            nids[S - 1, :] = -1
            nids[1, k - 1], nids[2, 1] = N, N + 1000
        owner = torch.arange(S) % P  # the pair whose time a row's gaps are measured from (identity rows: p and P + p)
        nbr_t = edge_time[owner][:, None] - gap
        nbr_t[nids == -1] = 0
        c.update(nids=nids, nbr_t=nbr_t, nbr_x=nbr_x)
    return c


def dyg_prologue_run(c, dtype=F64, mutate=None):
    w = c['widths']
    return dygformer_prologue(c['node_x'], c['src'], c['dst'], c['edge_time'], c['nids'], c['nbr_t'], c['nbr_x'], c['S'], c['k'], c['src_rows'],
                              c['dst_rows'], c['tw'], c['tb'], w[3], w[4], w[5], dtype, mutate)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_dygformer_tail
# ---------------------------------------------------------------------------------------------------------------------------
def dygformer_tail(x, P, Np, ldm, out_w, out_b, dtype=F64, mutate=None):
    """x [2 P Np, D], rows (2 p + side) Np + t.  mean [2 P, ldm]: row side P + p (sources first) = the mean over the Np tokens, columns
    [D, ldm) zero.  out [2 P, E] = mean out_w^T + out_b.  Returns (mean, mean_mag, out)."""
    D = x.shape[1]
    xs = x.to(dtype).view(P, 2, Np, D)
    m, a = xs.sum(2) / Np, xs.abs().sum(2) / Np  # [P, 2, D]
    order = (lambda t: t.reshape(2 * P, D)) if mutate == 'dyg_mean_row_order' else (lambda t: t.transpose(0, 1).reshape(2 * P, D))
    mean, mag = torch.zeros(2 * P, ldm, dtype=dtype), torch.zeros(2 * P, ldm, dtype=dtype)
    mean[:, :D], mag[:, :D] = order(m), order(a)
    return mean, mag, mean[:, :D] @ out_w.to(dtype).t() + out_b.to(dtype)


def dyg_mean_chain(Np: int) -> int:
    """dyg_mean_kernel: Np adds and the division."""
    return Np + 1


DYG_TAIL_CASES = [(1, 1, 1, 1), (5, 3, 63, 7), (1, 32, 64, 172), (5, 1, 65, 1), (5, 3, 200, 7), (1, 32, 257, 172), (5, 32, 257, 7)]  # (P, Np, D, E)


def dyg_tail_case(P, Np, D, E, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 977 * P + 131 * Np + 7 * D + E)
    return dict(x=torch.randn(2 * P * Np, D, generator=g) + 0.3, out_w=torch.randn(E, D, generator=g), out_b=torch.randn(E, generator=g), P=P,
                Np=Np, D=D, E=E, ldx=D + 3, ldm=D + 5)


def dyg_tail_bounds(c, dtype=F64, mutate=None):
    """(mean, out), (bound_mean, gemm_bar(D))."""
    mean, mag, out = dygformer_tail(c['x'], c['P'], c['Np'], c['ldm'], c['out_w'], c['out_b'], dtype, mutate)
    return (mean, out), (dyg_mean_chain(c['Np']) * EPS * mag.double(), gemm_bar(c['D']))


# ---------------------------------------------------------------------------------------------------------------------------
# deliberately wrong variants: name -> (the entry points it applies to, the condition on a case's shape under which it can show)
# ---------------------------------------------------------------------------------------------------------------------------
MUTATIONS = {
    # float(seed_t) - float(nbr_t): off by up to 128 at unix-scale times (every time case is one); k = 0 has no neighbour times
    'dt_float_first': ('prologue+dyg_prologue', lambda k=1, **_: k > 0),
    # the small-spread and the constant columns / rows (0 * inf without eps); one column of one value: every LayerNorm is K = 1
    'ln_without_eps': ('token+ln_rows', lambda **_: True),
    'ln_unbiased_variance': ('token+ln_rows', lambda K=1, C=1, d=1, **_: max(K, C, d) > 1),
    'gelu_tanh_approx': ('token', lambda Ht=0, **_: Ht > 0),
    'token_skips_channel_128': ('token', lambda C=1, **_: C > 128),  # the first channel of the second 128-chunk keeps x
    'token_skips_last_token_when_K_odd': ('token', lambda K=2, **_: K % 2 == 1),  # the two-wave pass
    'tail_counts_pads_in_denominator': ('tail', lambda **_: True),  # seeds with 0 < valid < K
    'tail_sums_pad_rows': ('tail', lambda **_: True),  # the 1e30 rows
    'timegap_drops_entries_past_multiple_of_4': ('tail', lambda **_: True),  # cnt = 1, 3, 5, 2, 7
    'timegap_divides_by_K': ('tail', lambda **_: True),  # cnt != K
    'mha_scores_include_pad_columns': ('mha', lambda T=16, **_: T % 16 != 0),
    'mha_scale_missing': ('mha', lambda dh=1, T=1, **_: dh > 1 and T > 1),
    'mha_head_offset_dropped': ('mha', lambda H=1, **_: H > 1),
    'dyg_mean_row_order': ('dyg_tail', lambda P=1, **_: P > 1),  # pair-major instead of sources first
    'dyg_time_for_pad_id': ('dyg_prologue', lambda k=0, **_: k > 0),  # slot ids of -1
    'dyg_node_feature_for_id_out_of_range': ('dyg_prologue', lambda k=0, P=9, **_: k > 0 and P <= 8),  # ids >= num_nodes: the small cases
}
