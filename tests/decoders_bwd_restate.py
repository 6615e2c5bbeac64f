"""The gradients of the three decoder heads written out by hand, on the CPU in float64, step by step as ``tgmx_decoder_backward`` composes
them (include/tgm_amd.h) -- the formulas, not autograd -- each with a per-element bound on what a float32 device result may differ by.

The bound is a running one.  A float32 sum of n terms, in ANY order, fused or not, differs from the exact sum by at most
``gamma(n) sum |terms|``, ``gamma(n) = n u / (1 - n u)``, ``u = 2^-24``; where an operand already carries an error ``E`` the product rule adds
``|A| E_B + E_A |B| + E_A E_B``.  So every quantity here is a pair (value, bound), starting from the inputs and parameters (exact: they are
float32 numbers) through the device's own forward (whose saved activations the backward reads) to every gradient.  A ReLU mask is read
from the saved activation: where ``|h| <= E_h`` the device's mask may differ from the exact one and the bound is the whole unmasked value.

``n`` is the chain length of the kernel that forms the sum, counted from its code where that is shorter than the number of terms:

* ``tgmx_decoder_tail_bwd`` dW / db: a wave's rows of its block (``ceil(rpb / 4)``), three wave adds, the blocks in ascending order;
* ``tgmx_sgemm_tn``: the rows of a split (two per MFMA step, ``rows_per_split`` roundings at most), then the splits in ascending order;
* ``tgmx_colsum``: the rows of a split, then the splits;
* ``tgmx_decoder_scatter``: a row's pairs in ascending order (at most 64), four quarters and their three adds beyond, 1024-entry chunks of
  four quarters each and the chunks in ascending order past 2048;
* the dX and forward GEMMs (``tgmx_sgemm_nt``, ``tgmx_decoder_pair_gemm``, the row dots) pick their K order by shape: the number of terms,
  which bounds every order, plus the bias and the final adds.

Nothing here is tuned on a device result.  The forward is ``decoders_restate``'s.
"""
from __future__ import annotations

import glob
import json
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

import decoders_restate as dr

U = 2.0**-24
F64 = torch.float64
# name -> (kind, constructor arguments, merge, rows): tests/decoders_restate.py's CASES of the same names
GRAD_CASES = {k: dr.CASES[k] for k in ('link_concat_100_100', 'link_sum_128', 'link_concat_deep', 'node_100')}
EXPECTED_GRAD_FIXTURES = sorted(GRAD_CASES)
LONG_ROW, VERY_LONG, CHUNK = 64, 2048, 1024  # spmm.h's kSpmmLongRow, kSpmmVeryLong, kSpmmChunk


def gamma(n) -> float:
    return n * U / (1.0 - n * U)


# ---- chain lengths, from the kernels' launch code ---------------------------------------------------------------------------------------------
def tail_bwd_rpb(R: int) -> int:
    rpb = -(-R // 256)
    return max(4, -(-rpb // 4) * 4)


def tail_bwd_chain(R: int) -> int:
    rpb = tail_bwd_rpb(R)
    return -(-rpb // 4) + 3 + -(-R // rpb)


def sgemm_tn_chain(R: int, M: int, N: int) -> int:
    tiles = -(-M // 32) * -(-N // 64)
    s = max(1, min(-(-2048 // tiles), -(-R // 64), 512))
    rps = -(-(-(-R // s)) // 8) * 8
    return rps + s


def colsum_chain(R: int) -> int:
    s = max(1, min(256, -(-R // 64)))
    return -(-R // s) + s


def scatter_chain(count: int, total: int) -> int:
    """A table row of ``count`` pairs among ``total`` CSR entries (2R at most: very long rows leave the first launch only then)."""
    if count <= LONG_ROW:
        return max(count, 1)
    if count <= VERY_LONG or total <= VERY_LONG:
        return -(-count // 4) + 4
    return CHUNK // 4 + 4 + count // CHUNK + 2


# ---- (value, bound) arithmetic ------------------------------------------------------------------------------------------------------------------
def _e(E, like: Tensor) -> Tensor:
    return torch.zeros_like(like) if E is None else E


def mm(A: Tensor, EA, B: Tensor, EB, n) -> Tuple[Tensor, Tensor]:
    """A @ B summed over n-long float32 chains, the operands off by EA / EB at most."""
    EA, EB = _e(EA, A), _e(EB, B)
    E = A.abs() @ EB + EA @ B.abs() + EA @ EB + gamma(n) * ((A.abs() + EA) @ (B.abs() + EB))
    return A @ B, E


def relu_saved(pre: Tensor, Epre: Tensor) -> Tuple[Tensor, Tensor]:
    """relu(pre) as the device saves it: exactly 0 where pre is negative beyond its bound"""
    return torch.relu(pre), torch.where(pre < -Epre, torch.zeros_like(Epre), Epre)


def masked(g: Tensor, Eg: Tensor, pre: Tensor, Epre: Tensor) -> Tuple[Tensor, Tensor]:
    """g where the saved activation relu(pre) > 0, else 0; where the device's pre may have the other sign (|pre| <= its bound) the mask
    may differ and the bound is the whole value."""
    on = pre > 0
    unsure = pre.abs() <= Epre
    return torch.where(on, g, torch.zeros_like(g)), torch.where(unsure, g.abs() + Eg, torch.where(on, Eg, torch.zeros_like(Eg)))


def _layers(sd: Dict[str, Tensor], first: int):
    n = len([k for k in sd if k.startswith('model.') and k.endswith('.weight')])
    return [(f'model.{2 * i}', sd[f'model.{2 * i}.weight'].to(F64), sd[f'model.{2 * i}.bias'].to(F64)) for i in range(first, n)]


def head_grads(sd: Dict[str, Tensor], kind: str, op: Optional[str], inputs: Dict[str, Tensor], dout: Tensor,
               idx: Optional[Tuple[Tensor, Tensor]] = None) -> Dict[str, Tuple[Tensor, Tensor]]:  # fmt: skip
    """name -> (gradient in float64, bound on a float32 device result) for every parameter (``state_dict`` keys) and every input
    ('z_src', 'z_dst' | 'z').  ``idx`` = (ia, ib): the table form over ``inputs['z']`` (pairs with an index outside the table take no part).
    ``dout``: the upstream gradient [R, out_dim] (or [R])."""
    sd = {k: v.detach() for k, v in sd.items()}
    g: Dict[str, Tuple[Tensor, Tensor]] = {}
    table = idx is not None
    # ---- the forward, as the device runs it: (activation, bound) of every saved tensor ----
    if kind == 'node':
        x = inputs['z'].to(F64)
        x = x.reshape(-1, x.shape[-1])
        h, Eh, relu, pre, Epre = x, torch.zeros_like(x), False, None, None
        layers = _layers(sd, 0)
    else:
        if table:
            z = inputs['z'].to(F64)
            ia, ib = (t.reshape(-1).long() for t in idx)
            keep = (ia >= 0) & (ia < z.shape[0]) & (ib >= 0) & (ib < z.shape[0])
            ia, ib = ia[keep], ib[keep]
            a, b = z[ia], z[ib]
        else:
            a, b = inputs['z_src'].to(F64), inputs['z_dst'].to(F64)
        D = a.shape[1]
        if op == 'concat':
            W0, b0 = sd['model.0.weight'].to(F64), sd['model.0.bias'].to(F64)
            Wa, Wb, bias, relu = W0[:, :D], W0[:, D:], b0, True
            layers = _layers(sd, 1)
        else:
            Wa, Wb = sd['merge.lin_src.weight'].to(F64), sd['merge.lin_dst.weight'].to(F64)
            bias, relu = sd['merge.lin_src.bias'].to(F64) + sd['merge.lin_dst.bias'].to(F64), False
            layers = _layers(sd, 0)
        n0 = 2 * D + 3  # both operands' K terms, the bias (LearnableSumMerge: the sum of two), the halves' add of the table form
        pre = a @ Wa.t() + b @ Wb.t() + bias
        Epre = gamma(n0) * (a.abs() @ Wa.abs().t() + b.abs() @ Wb.abs().t() + bias.abs())
        h, Eh = relu_saved(pre, Epre) if relu else (pre, Epre)
    dout = dout.to(F64).reshape(-1, layers[-1][1].shape[0])
    R_all = dout.shape[0]
    if table:
        dout = dout[keep]
    saved = []  # per layer: (its input, the input's bound, whether the input went through a ReLU, what went into that ReLU and its bound)
    for i, (name, W, bv) in enumerate(layers):
        saved.append((h, Eh, relu, pre, Epre))
        if i < len(layers) - 1:
            pre, Epre = mm(h, Eh, W.t(), None, W.shape[1] + 1)
            pre, Epre = pre + bv, Epre + gamma(W.shape[1] + 1) * bv.abs()
            (h, Eh), relu = relu_saved(pre, Epre), True
    # ---- the backward, from the back ----
    R = dout.shape[0]
    dY, EdY = dout, torch.zeros_like(dout)
    first = kind == 'node'
    for i in range(len(layers) - 1, -1, -1):
        name, W, bv = layers[i]
        X, EX, x_relu, pre, Epre = saved[i]
        out_dim, in_dim = W.shape
        tail = i == len(layers) - 1 and out_dim <= 16 and out_dim * in_dim * 4 <= 48 * 1024
        n_w = tail_bwd_chain(R) if tail else sgemm_tn_chain(R, out_dim, in_dim)
        n_b = tail_bwd_chain(R) if tail else colsum_chain(R)
        g[f'{name}.weight'] = mm(dY.t(), EdY.t(), X, EX, n_w)
        ones = torch.ones(R, 1, dtype=F64)
        db, Edb = mm(dY.t(), EdY.t(), ones, None, n_b)
        g[f'{name}.bias'] = (db.reshape(-1), Edb.reshape(-1))
        dX, EdX = mm(dY, EdY, W, None, out_dim + 1)
        if x_relu:
            dX, EdX = masked(dX, EdX, pre, Epre)
        dY, EdY = dX, EdX
    if first:
        g['z'] = (dY.reshape(inputs['z'].shape), EdY.reshape(inputs['z'].shape))
        return g
    # ---- the merge stage: dY is dh0 [R, H] ----
    H = dY.shape[1]
    ones = torch.ones(R, 1, dtype=F64)
    db0, Edb0 = mm(dY.t(), EdY.t(), ones, None, colsum_chain(R))
    db0, Edb0 = db0.reshape(-1), Edb0.reshape(-1)
    if table:
        NP = z.shape[0]
        halves = []
        for ix in (ia, ib):
            counts = torch.bincount(ix, minlength=NP)
            n_row = torch.tensor([scatter_chain(int(c), 2 * R_all) for c in counts], dtype=F64)
            dP = torch.zeros(NP, H, dtype=F64).index_add_(0, ix, dY)
            mag = torch.zeros(NP, H, dtype=F64).index_add_(0, ix, dY.abs() + EdY)
            EdP = torch.zeros(NP, H, dtype=F64).index_add_(0, ix, EdY) + (n_row * U / (1 - n_row * U)).unsqueeze(1) * mag
            halves.append((dP, EdP))
        (dPa, EPa), (dPb, EPb) = halves
        n_w = sgemm_tn_chain(NP, H, D)
        dWa, dWb = mm(dPa.t(), EPa.t(), z, None, n_w), mm(dPb.t(), EPb.t(), z, None, n_w)
        dz, Edz = mm(torch.cat((dPa, dPb), 1), torch.cat((EPa, EPb), 1), torch.cat((Wa, Wb), 0), None, 2 * H + 1)
        g['z'] = (dz, Edz)
    else:
        n_w = sgemm_tn_chain(R, H, D)
        dWa, dWb = mm(dY.t(), EdY.t(), a, None, n_w), mm(dY.t(), EdY.t(), b, None, n_w)
        g['z_src'], g['z_dst'] = mm(dY, EdY, Wa, None, H + 1), mm(dY, EdY, Wb, None, H + 1)
    if op == 'concat':
        g['model.0.weight'] = (torch.cat((dWa[0], dWb[0]), 1), torch.cat((dWa[1], dWb[1]), 1))
        g['model.0.bias'] = (db0, Edb0)
    else:
        g['merge.lin_src.weight'], g['merge.lin_dst.weight'] = dWa, dWb
        g['merge.lin_src.bias'] = g['merge.lin_dst.bias'] = (db0, Edb0)
    return g


def worst_ratio(got: Tensor, ref: Tensor, bound: Tensor) -> float:
    """max |got - ref| / bound over the elements (0 / 0 counts as 0: an exact zero must be met exactly)"""
    got = got.detach().cpu().to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    if err.numel() == 0:
        return 0.0
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    return float(ratio.max())


# ---- the recorded gradients (tests/golden/make_golden_decoder_grads.py) ------------------------------------------------------------------------
def grad_fixture_names():
    return sorted(os.path.basename(p)[len('g30_decoder_grad_') : -len('.npz')] for p in glob.glob(os.path.join(dr.GOLDEN, 'g30_decoder_grad_*.npz')))


def load_grad_fixture(name: str):
    """(meta, state_dict, inputs, upstream gradient, the reference's gradients: name -> float32 tensor)"""
    with np.load(os.path.join(dr.GOLDEN, f'g30_decoder_grad_{name}.npz')) as f:
        meta = json.loads(bytes(f['meta']).decode())
        sd = {k[2:]: torch.from_numpy(f[k]) for k in meta['keys']}
        inputs = {k: torch.from_numpy(f[k]) for k in ('z_src', 'z_dst', 'z') if k in f.files}
        grads = {k[2:]: torch.from_numpy(f[k]) for k in f.files if k.startswith('g.')}
        return meta, sd, inputs, torch.from_numpy(f['dout']), grads
