"""ORACLE (test infrastructure only -- never imported by the product path).

float64 restatements of the six public building blocks of ``csrc/tgat_bwd.hip`` (``tgmx_sgemm_tn``, ``tgmx_colsum``,
``tgmx_relu_mask``, ``tgmx_add_cols``, ``tgmx_ln_backward``, ``tgmx_tgat_attn_backward``), pure torch on the CPU.  Every function
takes the float32 tensors the kernel gets and returns ``(value, magnitude)`` pairs: the value in float64 and, with the same shape, the
same formula with every term replaced by its absolute value.  A worst-case rounding bound for a float32 evaluation of the formula is
``n * 2^-24 * magnitude`` with ``n`` the length of the longest chain of float32 operations into the element (``ln_chain`` /
``attn_chain`` below); the tests build their bars from it.  ``dtype=torch.float32`` evaluates the same formulas in float32 (plain
torch): the tests use it to show that the bars leave room for an honest float32 implementation.

``attn_case`` builds the row kinds the attention tests share (CPU and GPU): it lives here so that both see the same rows.
"""
from __future__ import annotations

import math

import torch

F64 = torch.float64
EPS = 2.0 ** -24  # unit round-off of float32


def sgemm_tn(A, B, dtype=F64):
    """C[..., m, n] = sum_r A[..., r, m] B[..., r, n]."""
    a, b = A.to(dtype), B.to(dtype)
    return a.transpose(-1, -2) @ b, a.abs().transpose(-1, -2) @ b.abs()


def colsum(x, dtype=F64):
    """out[c] = sum_r x[r, c]."""
    v = x.to(dtype)
    return v.sum(0), v.abs().sum(0)


def relu_mask(g, h, dtype=F64):
    """g[r, c] where h[r, c] > 0, else 0  (-0.0 and 0.0 are not > 0)."""
    v = torch.where(h > 0, g.to(dtype), torch.zeros((), dtype=dtype))
    return v, v.abs()


def add_cols(dst, src, accumulate, dtype=F64):
    """dst + src (accumulate) or src."""
    d, s = dst.to(dtype), src.to(dtype)
    return (d + s, d.abs() + s.abs()) if accumulate else (s, s.abs())


def ln_backward(dout, y, res, gamma, eps, dtype=F64):
    """Backward of LayerNorm(y + res) * gamma + beta w.r.t. u = y + res, and dgx = dout * xhat (its column sum is d gamma).
    Returns (du, dgx, |du|-magnitude, |dgx|-magnitude)."""
    dout, y, res, gamma = (t.to(dtype) for t in (dout, y, res, gamma))
    u = y + res
    mean = u.mean(-1, keepdim=True)
    t = u - mean
    rstd = 1.0 / torch.sqrt((t * t).mean(-1, keepdim=True) + eps)
    xhat = t * rstd
    gd = gamma * dout
    du = rstd * (gd - gd.mean(-1, keepdim=True) - xhat * (gd * xhat).mean(-1, keepdim=True))
    dgx = dout * xhat
    au = y.abs() + res.abs()
    xmag = (au + au.mean(-1, keepdim=True)) * rstd  # |u| + |mean|: what the subtraction u - mean can lose
    gm = gd.abs()
    du_mag = rstd * (gm + gm.mean(-1, keepdim=True) + xmag * (gm * xmag).mean(-1, keepdim=True))
    return du, dgx, du_mag, dout.abs() * xmag


def ln_chain(O: int) -> int:
    """float32 operations on the longest chain into an element of du, plus 8: two sums over the O columns."""
    return 2 * O + 16


def attn_chain(C: int, H: int, k: int, dtime: bool = False) -> int:
    """The dot product over the C columns, the softmax-backward sum and the slot / head sums, plus 8; dtime sums k slots more."""
    return C + H * k + 8 + (k if dtime else 0)


def time_args(seed_t, nbr_t, tw, tb):
    """dt = float32(seed_t - nbr_t) [R, k] and arg = one fma rounded to float32 [R, k, T].  (dt * tw is exact in float64; the sum is
    rounded to float64 and then to float32 -- this differs from the single rounding of an fma only when the float64 sum is an exact
    float32 tie, once in ~2^29 elements.)"""
    dt = (seed_t[:, None] - nbr_t).to(torch.float32)
    arg = (dt.double()[:, :, None] * tw.double() + tb.double()).to(torch.float32)
    return dt, arg


def attn_backward(qf, probs, dzbar, nbrf, ex, seed_t, nbr_t, tw, tb, scale, keep, no_valid, dnbr0=None, dtype=F64, mutate=None):
    """Backward of the folded masked-softmax attention row (tgmx_tgat_attn_reduce), by hand:

        z[s] = [nbrf[s] | ex[s] | cos(arg[s])],  A' = probs * keep,  dA = (dzbar . z[s]) * keep
        ds = probs * (dA - sum_s probs dA); rows flagged no_valid: ds = 0 (the reference's masked_fill(-1e10) on every slot)
        dqf[h] = scale * sum_s ds[h, s] z[s],  dzs[s] = sum_h (A'[h, s] dzbar[h] + scale * ds[h, s] qf[h])
        dnbr = dnbr0 + dzs[:, :d],  dtime[:, :T] = sum_s -sin(arg) dzs[s, time] dt[s],  dtime[:, T:] = sum_s -sin(arg) dzs[s, time]

    qf, dzbar [R, H, C]; probs, keep [R, H, k]; nbrf [R, k, d]; ex [R, k, D] (D may be 0); no_valid [R] bool; dnbr0 [R, k, d] or None.
    Returns a dict with dqf, dnbr, dtime and dqf_mag, dnbr_mag, dtime_mag (|cos| and |sin| count as 1 in the magnitudes).
    ``mutate``: one deliberately wrong variant (the sensitivity tests), see MUTATIONS."""
    R, k, d = nbrf.shape
    D, T, H = ex.shape[2], tw.shape[0], qf.shape[1]
    C = d + D + T
    dt, arg = time_args(seed_t, nbr_t, tw, tb)
    if mutate == 'dt_from_neighbouring_slot':
        dt = dt.roll(1, dims=1)
        arg = (dt.double()[:, :, None] * tw.double() + tb.double()).to(torch.float32)
    if mutate == 'other_heads_probs':
        probs = probs.flip(1)
    qf, probs, dzbar, nbrf, ex, keep = (t.to(dtype) for t in (qf, probs, dzbar, nbrf, ex, keep))
    argc, dtc = arg.to(dtype), dt.to(dtype)
    z = torch.cat([nbrf, ex, torch.cos(argc)], -1)  # [R, k, C]
    zmag = torch.cat([nbrf.abs(), ex.abs(), torch.ones_like(argc)], -1)
    zs, zsmag = z, zmag
    if mutate == 'skip_column_C-1':
        zs, zsmag = z.clone(), zmag.clone()
        zs[..., C - 1] = 0
    keep_dA = torch.ones_like(keep) if mutate == 'omit_keep_on_dA' else keep
    dA = torch.einsum('rhc,rkc->rhk', dzbar, zs) * keep_dA
    dA_mag = torch.einsum('rhc,rkc->rhk', dzbar.abs(), zsmag) * keep_dA
    ds = probs * (dA - (probs * dA).sum(-1, keepdim=True))
    ds_mag = probs * (dA_mag + (probs * dA_mag).sum(-1, keepdim=True))
    ds = torch.where(no_valid[:, None, None], torch.zeros_like(ds), ds)
    ds_mag = torch.where(no_valid[:, None, None], torch.zeros_like(ds), ds_mag)
    Ap = probs * keep
    if mutate == 'drop_last_slot_of_one_row':  # the fully valid row (attn_case: row k)
        ds, Ap = ds.clone(), Ap.clone()
        ds[min(k, R - 1), :, k - 1] = 0
        Ap[min(k, R - 1), :, k - 1] = 0
    dqf = scale * torch.einsum('rhk,rkc->rhc', ds, zs)
    dqf_mag = scale * torch.einsum('rhk,rkc->rhc', ds_mag, zsmag)
    dzs = torch.einsum('rhk,rhc->rkc', Ap, dzbar) + scale * torch.einsum('rhk,rhc->rkc', ds, qf)
    dzs_mag = torch.einsum('rhk,rhc->rkc', Ap, dzbar.abs()) + scale * torch.einsum('rhk,rhc->rkc', ds_mag, qf.abs())
    dn0 = torch.zeros_like(nbrf) if dnbr0 is None else dnbr0.to(dtype)
    dnbr = dzs[..., :d].clone() if mutate == 'no_accumulate_into_dnbr' else dn0 + dzs[..., :d]
    g = -torch.sin(argc) * dzs[..., d + D:]
    gmag = dzs_mag[..., d + D:]
    dtime = torch.cat([(g * dtc[:, :, None]).sum(1), g.sum(1)], -1)
    dtime_mag = torch.cat([(gmag * dtc.abs()[:, :, None]).sum(1), gmag.sum(1)], -1)
    return dict(dqf=dqf, dnbr=dnbr, dtime=dtime, dqf_mag=dqf_mag, dnbr_mag=dn0.abs() + dzs_mag[..., :d], dtime_mag=dtime_mag)


# name -> the condition under which the mutation can change anything at all.  (k = 1: the softmax of a single slot is the constant 1,
# so ds = 0 whatever dA is, and every head's weight is 1: a mutation that only reaches the outputs through dA or the weights is none.)
MUTATIONS = {
    'drop_last_slot_of_one_row': lambda H, k, drop: True,
    'other_heads_probs': lambda H, k, drop: H > 1 and k > 1,  # one head has no other
    'omit_keep_on_dA': lambda H, k, drop: drop and k > 1,     # keep is all ones without dropout
    'dt_from_neighbouring_slot': lambda H, k, drop: k > 1,    # one slot has no neighbour
    'skip_column_C-1': lambda H, k, drop: k > 1,
    'no_accumulate_into_dnbr': lambda H, k, drop: True,
}

# (R, M, N, batch): the split / tile edges of tgmx_sgemm_tn;  (R, C): those of tgmx_colsum;  LayerNorm widths and row counts
SGEMM_TN_CASES = [(0, 5, 7, 1), (1, 1, 1, 1), (7, 33, 65, 1), (65, 32, 64, 1), (300, 128, 64, 1), (300, 129, 64, 1), (1345, 320, 640, 1),
                  (33000, 8, 12, 1), (12600, 172, 344, 1), (600, 86, 273, 2), (600, 86, 172, 2)]
COLSUM_CASES = [(0, 3), (1, 1), (63, 5), (64, 256), (65, 257), (16400, 7), (12600, 200)]
LN_WIDTHS = [1, 2, 5, 64, 65, 172, 300]
LN_ROWS = [1, 2, 5, 37]


def randn_or_int(shape, integer, g):
    """float32 inputs: randn, or integers in [-4, 4] (every partial sum of the cases above stays below 2^24: float32 sums are exact)."""
    if integer:
        return torch.randint(-4, 5, shape, generator=g).to(torch.float32)
    return torch.randn(shape, generator=g)


def ln_case(R, O, seed=0):
    """dout, y, res, gamma for LayerNorm backward; y + res has a row standard deviation of at least 0.1 (O = 1: it has none)."""
    g = torch.Generator().manual_seed(seed * 7919 + R * 331 + O)
    for _ in range(100):  # (redrawn until every row is wide enough: a fixed seed, so the same tensors every time)
        dout, y, gamma = torch.randn(R, O, generator=g), torch.randn(R, O, generator=g), 1.0 + 0.5 * torch.randn(O, generator=g)
        res = torch.randn(R, O, generator=g) + 3.0 * torch.randn(R, 1, generator=g)  # a row offset: the mean is not small
        if O == 1 or float((y + res).double().std(-1, unbiased=False).min()) >= 0.1:
            return dout, y, res, gamma
    raise AssertionError(f'ln_case({R}, {O}): no draw with row std >= 0.1')


# (H, k, d, D, T): the dispatch routes of launch_attn_backward (tests/test_tgat_bwd_blocks_gpu.py says which condition sends each there)
ATTN_SHAPES = [
    (1, 5, 1, 4, 8), (1, 20, 3, 8, 128), (2, 10, 8, 12, 16), (2, 13, 4, 16, 70), (2, 20, 1, 172, 100), (2, 20, 172, 172, 100),
    (2, 4, 1, 6, 10), (2, 6, 5, 0, 9), (2, 20, 4, 8, 130), (2, 20, 66, 8, 16), (2, 20, 130, 12, 16), (2, 20, 200, 8, 16), (2, 20, 201, 8, 16),
    (4, 16, 8, 12, 16), (8, 8, 8, 4, 12), (4, 1, 5, 3, 3), (1, 64, 4, 8, 6), (2, 32, 3, 4, 7),
]


def attn_case(H, k, d, D, T, seed=0):
    """R = k + 8 rows of float32 inputs for the attention backward, one per row kind:

        rows 0 .. k-1   left-padded, 1 .. k valid slots (row k-1 is fully valid): every span body
        row  k          fully valid
        row  k+1        an interior hole (slot k // 2 masked; k < 3: slot 0)
        row  k+2        all-zero dzbar (the early exit)
        row  k+3        no valid slot, identical slot features (the sampler's all-pad row)
        row  k+4        no valid slot, differing slot features
        rows k+5, k+6   dt up to 2^30 with tw[0] = 1: Time2Vec arguments past 8e6 (the double reduction path), below 2.1e9
        row  k+7        a random mask with at least one valid slot

    probs is the float64 softmax of random scores under masked_fill(-1e10), rounded to float32: masked slots exactly 0, rows without
    a valid slot uniform.  Returns a dict of CPU tensors (qf, probs, dzbar, nbrf, ex, seed_t, nbr_t, tw, tb, scale, mask, no_valid)."""
    g = torch.Generator().manual_seed(1000 * seed + 97 * H + 13 * k + 7 * d + 3 * D + T)
    R, C = k + 8, d + D + T
    slot = torch.arange(k)
    mask = torch.ones(R, k, dtype=torch.bool)
    for r in range(k):
        mask[r] = slot >= k - 1 - r
    mask[k + 1, k // 2 if k >= 3 else 0] = False
    mask[k + 3] = False
    mask[k + 4] = False
    mask[k + 7] = torch.rand(k, generator=g) < 0.5
    mask[k + 7, int(torch.randint(0, k, (1,), generator=g))] = True
    no_valid = ~mask.any(1)
    scores = torch.randn(R, H, k, generator=g, dtype=F64).masked_fill(~mask[:, None, :], -1e10)
    probs = torch.softmax(scores, -1).to(torch.float32)
    qf = torch.randn(R, H, C, generator=g) * 0.5
    dzbar = torch.randn(R, H, C, generator=g)
    dzbar[k + 2] = 0.0
    nbrf = torch.randn(R, k, d, generator=g)
    ex = torch.rand(R, k, D, generator=g)
    seed_t = torch.randint(1_000_000, 2_600_000, (R,), generator=g)
    nbr_t = seed_t[:, None] - torch.randint(1, 900_000, (R, k), generator=g)
    pad = ~mask
    pad[k + 4] = False  # the differing all-pad row keeps its random features and times
    pad[k + 1] = False  # so does the hole (an explicit mask over a real slot)
    pad[k + 7] = False
    nbrf[k + 3] = nbrf[k + 3, 0]
    nbrf[pad & ~no_valid[:, None]] = 0.0
    ex[pad] = 0.0
    nbr_t[pad] = 0
    for i, r in enumerate((k + 5, k + 6)):
        seed_t[r] = (1 << 30) + 12345 * (i + 1)
        nbr_t[r] = torch.where(mask[r], torch.randint(0, 1 << 29, (k,), generator=g), torch.zeros(k, dtype=torch.int64))
        nbr_t[r, k - 1] = 3 + i  # dt just below 2^30 + ...: the largest argument
    tw = (1.0 / 10 ** torch.linspace(0, 9, T, dtype=F64)).to(torch.float32)
    tb = torch.randn(T, generator=g) * 0.1
    return dict(qf=qf, probs=probs, dzbar=dzbar, nbrf=nbrf, ex=ex, seed_t=seed_t, nbr_t=nbr_t, tw=tw, tb=tb,
                scale=float(C) ** -0.5, mask=mask, no_valid=no_valid, R=R, C=C)


def attn_forward_autograd(qf, dzbar, nbrf, ex, seed_t, nbr_t, tw, tb, scale, keep, mask):
    """float64 autograd through a plain forward: scores = scale * qf . z, masked_fill(-1e10), softmax, dropout as a given keep mask, zbar = A' z; loss = sum(zbar * dzbar).
    Returns (probs, dict of gradients w.r.t. qf, nbrf, tw, tb): what attn_backward must reproduce (dtime summed over the rows)."""
    qf, nbrf, tw, tb = (t.double().clone().requires_grad_(True) for t in (qf, nbrf, tw, tb))
    dt = (seed_t[:, None] - nbr_t).to(torch.float32).double()
    z = torch.cat([nbrf, ex.double(), torch.cos(dt[:, :, None] * tw + tb)], -1)
    s = (scale * torch.einsum('rhc,rkc->rhk', qf, z)).masked_fill(~mask[:, None, :], -1e10)
    A = torch.softmax(s, -1)
    zbar = torch.einsum('rhk,rkc->rhc', A * keep.double(), z)
    (zbar * dzbar.double()).sum().backward()
    return A.detach(), dict(dqf=qf.grad, dnbr=nbrf.grad, dtw=tw.grad, dtb=tb.grad)


def worst_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (0 / 0 counts as 0, x / 0 as inf)."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0


def gemm_bar(R: int) -> float:
    """The project's bar for exact-fp32 GEMMs on randn inputs (tests/test_gemm_gpu.py), with the reduction length R."""
    return 2e-5 * math.sqrt(max(R, 1))
