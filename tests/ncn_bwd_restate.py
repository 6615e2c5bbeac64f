"""The gradients of NCNPredictor written out by hand, on the CPU in float64, step by step as ``tgmx_ncn_backward`` composes them
(include/tgm_amd.h) -- the formulas, not autograd -- each with a per-element bound on what a float32 device result may differ by.

The bound is ``decoders_bwd_restate``'s running one: a float32 sum of n terms, in any order, fused or not, differs from the exact sum by
at most ``gamma(n) sum |terms|``; where an operand already carries an error the product rule adds ``|A| E_B + E_A |B| + E_A E_B``; a ReLU
mask read from a saved ``h`` with ``|h| <= E_h`` may differ from the exact one and the bound is then the whole unmasked value.  Every quantity
is a (value, bound) pair from the inputs (exact float32 numbers) through the device's own forward to every gradient.

Chain lengths, counted from the launch code:

* the forward's ``xs`` (csrc/ncn.hip): one rounding for ``x_i x_j``; a k = 4 block is ``fl(fl(m W) x)``; the common-neighbour sum is one fma
  per distinct common neighbour in ascending id, its weight ``fl(fl(A_i A_j) W)`` (the count product is an exact small integer);
* ``W = expf(-(gap / 10000))`` on the float32 gap the reference forms: the division is correctly rounded and is the reference's own float32
  number, ``expf`` is taken as accurate to 2 ulp: ``E_W = 4 u W``;
* the two Linear layers and ``dxs``: the number of terms plus the bias, which bounds every K order of ``tgmx_sgemm_nt``;
* ``dW2`` / ``db2``: ``tgmx_decoder_tail_bwd``'s chain where the tail route applies, else ``tgmx_sgemm_tn`` / ``tgmx_colsum``; ``dW1`` / ``db1``:
  ``tgmx_sgemm_tn`` / ``tgmx_colsum`` (``decoders_bwd_restate``'s counts);
* ``dx`` (csrc/ncn_bwd.hip): a node's row is ONE chain of fmas, a rounding per term -- the pairs of term (1) in ascending r (a k = 4 pair adds
  a second term), those of term (2), then term (3) in ascending (tar_i, r): ``T`` terms, chain ``T``.  A row of more than ``LONG_ROW``
  adjacency entries (and only when 2 E exceeds it) sums term (3) per ``CHUNK`` entries of the entry array and adds the chunk sums in ascending
  chunk order onto terms (1) + (2): no term passes through more than ``T + chunks`` roundings, which is the chain used here.

Nothing here is tuned on a device result.  The forward is ``ncn_restate``'s arithmetic, written again with its bounds.

``variant`` selects a deliberately WRONG backward the tests must tell from the right one: ``'no_last'`` (term (3) without the 'last' rule),
``'no_self_double'`` (a pair with i = j contributes through term (2) only), ``'single_mult'`` (A[n, i] counted once in term (3)),
``'wrong_w'`` (the k = 4 blocks weighted with W[r, .] of the other target).
"""
from __future__ import annotations

import glob
import json
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

import ncn_restate as nr
from decoders_bwd_restate import F64, U, colsum_chain, gamma, masked, mm, relu_saved, sgemm_tn_chain, tail_bwd_chain, worst_ratio  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LONG_ROW, CHUNK = 512, 256  # csrc/ncn_bwd.hip's kNcnBwdLongRow, kNcnBwdChunk
E_EXPF = 4 * U  # expf within 2 ulp
VARIANTS = ('no_last', 'no_self_double', 'single_mult', 'wrong_w')
PARAMS = ('xsmlp.0.weight', 'xsmlp.0.bias', 'xsmlp.2.weight', 'xsmlp.2.bias')


def active_pairs(ti: Tensor, tj: Tensor, ok: Tensor, dup: str) -> Tensor:
    """[B] bool: the forward's rule -- in range, and under 'last' the last in-range position of its target on both sides."""
    if dup == 'all':
        return ok.clone()
    li, lj = {}, {}
    for r in range(ti.numel()):
        if ok[r]:
            li[int(ti[r])], lj[int(tj[r])] = r, r
    return torch.tensor([bool(ok[r]) and li[int(ti[r])] == r and lj[int(tj[r])] == r for r in range(ti.numel())], dtype=torch.bool)


def _prod(a: Tensor, Ea: Tensor, b: Tensor, Eb: Tensor) -> Tuple[Tensor, Tensor]:
    """fl(a b) of two carried quantities"""
    v = a * b
    E = a.abs() * Eb + Ea * b.abs() + Ea * Eb
    return v, E + U * (v.abs() + E)


def _mlp(sd, x, A, ci, cj, xi, xj, actf, m, W, EW, Wi, EWi, Wj, EWj, k, dout, g, dout_abs_err=0.0) -> Tuple[Tensor, Tensor]:
    """the forward as the device runs it and the MLP's backward: fills g with the parameters' gradients, returns (dxs, bound)"""
    (B, C), N = xi.shape, x.shape[0]
    Z = torch.zeros((B, C), dtype=F64)
    w1, b1 = sd['xsmlp.0.weight'].detach().cpu().to(F64), sd['xsmlp.0.bias'].detach().cpu().to(F64)
    w2, b2 = sd['xsmlp.2.weight'].detach().cpu().to(F64), sd['xsmlp.2.bias'].detach().cpu().to(F64)
    H, O, K = w1.shape[0], w2.shape[0], k * C
    # ---- the forward, as the device runs it ----
    blocks = [_prod(xi, Z, xj, Z)]
    Ai, Aj = A[ci] * actf, A[cj] * actf  # [B, N]
    if k == 4:
        for Wt, EWt, xt in ((Wi, EWi, xi), (Wj, EWj, xj)):
            c, Ec = _prod(m, torch.zeros_like(m), Wt, EWt)
            blocks.append(_prod(c.expand(B, C), Ec.expand(B, C), xt, Z))
    coef, Ecoef = _prod(Ai * Aj, torch.zeros_like(W), W, EW)  # [B, N]
    n_cn = ((Ai * Aj) > 0).sum(dim=1, keepdim=True).clamp(min=1).to(F64)
    blocks.append(mm(coef, Ecoef, x, None, n_cn))
    xs, Exs = torch.cat([b[0] for b in blocks], 1), torch.cat([b[1] for b in blocks], 1)
    pre, Epre = mm(xs, Exs, w1.t(), None, K + 1)
    pre, Epre = pre + b1, Epre + gamma(K + 1) * b1.abs()
    h, Eh = relu_saved(pre, Epre)
    # ---- the MLP's backward ----
    dY = torch.as_tensor(dout).detach().cpu().to(F64).reshape(B, O)
    EdY = torch.full_like(dY, dout_abs_err)
    tail = O <= 16 and O * H * 4 <= 48 * 1024
    ones = torch.ones(B, 1, dtype=F64)
    g['xsmlp.2.weight'] = mm(dY.t(), EdY.t(), h, Eh, tail_bwd_chain(B) if tail else sgemm_tn_chain(B, O, H))
    db2 = mm(dY.t(), EdY.t(), ones, None, tail_bwd_chain(B) if tail else colsum_chain(B))
    g['xsmlp.2.bias'] = (db2[0].reshape(-1), db2[1].reshape(-1))
    dpre, Edpre = masked(*mm(dY, EdY, w2, None, O + 1), pre, Epre)
    g['xsmlp.0.weight'] = mm(dpre.t(), Edpre.t(), xs, Exs, sgemm_tn_chain(B, H, K))
    db1 = mm(dpre.t(), Edpre.t(), ones, None, colsum_chain(B))
    g['xsmlp.0.bias'] = (db1[0].reshape(-1), db1[1].reshape(-1))
    dxs, Edxs = mm(dpre, Edpre, w1, None, H + 1)
    g['_h'] = (h, Eh)
    return dxs, Edxs


def grads(sd: Dict[str, Tensor], x, edge_index, tar_ei, k: int, dout, last_update=None, edge_time=None, duplicate_targets: str = 'last',
          variant: Optional[str] = None, dxs=None, dout_abs_err: float = 0.0) -> Dict[str, Tuple[Tensor, Tensor]]:  # fmt: skip
    """name -> (gradient in float64, bound on a float32 device result) for 'x' and the four ``xsmlp`` parameters.  With ``dxs`` [B, k C]
    (exact float32 numbers) only the dx stage is restated (``tgmx_ncn_dx``): ``sd`` and ``dout`` are not read, the result holds 'x' alone.
    ``dout_abs_err``: what every element of the device's upstream gradient may differ from ``dout`` by (0: ``dout`` is what the device got)."""
    assert variant is None or variant in VARIANTS
    x = torch.as_tensor(x).detach().cpu().to(F64)
    N, C = x.shape
    tar = torch.as_tensor(tar_ei).detach().cpu().long()
    ti, tj = tar[0], tar[1]
    B = ti.numel()
    ok = (ti >= 0) & (ti < N) & (tj >= 0) & (tj < N)
    ei = torch.as_tensor(edge_index).detach().cpu().long()
    E_all = ei.shape[1]
    ei = ei[:, ((ei >= 0) & (ei < N)).all(dim=0)]
    A = nr.dense_adjacency(N, ei)
    act = active_pairs(ti, tj, ok, duplicate_targets)
    ci, cj = ti.clamp(0, N - 1), tj.clamp(0, N - 1)
    okf, actf = ok.to(F64)[:, None], act.to(F64)[:, None]
    W = nr.decay_weights(last_update, edge_time).reshape(B, N) if last_update is not None else torch.ones((B, N), dtype=F64)
    EW = E_EXPF * W if last_update is not None else torch.zeros_like(W)
    xi, xj = x[ci] * okf, x[cj] * okf
    ar = torch.arange(B)
    m = (A[ci, cj] * act.to(F64))[:, None]  # A[i, j] of the active pairs
    Wi, EWi, Wj, EWj = W[ar, ci][:, None], EW[ar, ci][:, None], W[ar, cj][:, None], EW[ar, cj][:, None]
    g: Dict[str, Tuple[Tensor, Tensor]] = {}
    if dxs is not None:  # the dx stage alone: dxs is an exact float32 input
        dxs = torch.as_tensor(dxs).detach().cpu().to(F64).reshape(B, k * C)
        Edxs = torch.zeros_like(dxs)
    else:
        dxs, Edxs = _mlp(sd, x, A, ci, cj, xi, xj, actf, m, W, EW, Wi, EWi, Wj, EWj, k, dout, g, dout_abs_err)
    # ---- dx: every term as (value, bound of its operands), scattered to its node; then one chain per node ----
    g0, Eg0 = dxs[:, :C], Edxs[:, :C]
    gcn, Egcn = dxs[:, (k - 1) * C : k * C], Edxs[:, (k - 1) * C : k * C]
    val, opd, mag = (torch.zeros((N, C), dtype=F64) for _ in range(3))
    terms = torch.zeros(N, dtype=F64)

    def scatter(idx: Tensor, keep: Tensor, v: Tensor, Ev: Tensor) -> None:
        """the terms v (carrying Ev) of the pairs in ``keep`` go to the nodes idx"""
        kf = keep.to(F64)[:, None]
        val.index_add_(0, idx, v * kf)
        opd.index_add_(0, idx, Ev * kf)
        mag.index_add_(0, idx, (v.abs() + Ev) * kf)
        terms.index_add_(0, idx, keep.to(F64))

    side1 = ok & ~((ti == tj) if variant == 'no_self_double' else torch.zeros(B, dtype=torch.bool))
    scatter(ci, side1, g0 * xj, Eg0 * xj.abs())  # (1)
    scatter(cj, ok, g0 * xi, Eg0 * xi.abs())  # (2)
    if k == 4:
        has = act & (m[:, 0] > 0)
        for idx, Wt, EWt, blk in ((ci, Wj if variant == 'wrong_w' else Wi, EWi, 1), (cj, Wi if variant == 'wrong_w' else Wj, EWj, 2)):
            c, Ec = _prod(m, torch.zeros_like(m), Wt, EWt)
            gs, Egs = dxs[:, blk * C : (blk + 1) * C], Edxs[:, blk * C : (blk + 1) * C]
            scatter(idx, has, c * gs, c.abs() * Egs + Ec * gs.abs() + Ec * Egs)
    # (3): node n from pair r with weight A[n, i] A[n, j] W[r, n]
    act3 = ok if variant == 'no_last' else act
    Ai3 = A[ci] * act3.to(F64)[:, None]
    if variant == 'single_mult':
        Ai3 = (Ai3 > 0).to(F64)
    cnt3 = Ai3 * A[cj] * act3.to(F64)[:, None]
    c3, Ec3 = _prod(cnt3, torch.zeros_like(W), W, EW)
    val += c3.t() @ gcn
    opd += c3.t().abs() @ Egcn + Ec3.t() @ gcn.abs() + Ec3.t() @ Egcn
    mag += (c3.abs() + Ec3).t() @ (gcn.abs() + Egcn)
    terms += (cnt3 > 0).sum(dim=0).to(F64)
    deg = A.sum(dim=1)
    chunks = torch.zeros(N, dtype=F64)
    if 2 * E_all > LONG_ROW:  # (the kernel's rule is on the host's 2 E, dropped edges included)
        start = torch.cumsum(deg, 0) - deg
        span = torch.floor((start + deg - 1) / CHUNK) - torch.floor(start / CHUNK) + 1
        chunks = torch.where(deg > LONG_ROW, span, chunks)
    chain = (terms + chunks).clamp(min=1)[:, None]
    g['x'] = (val, opd + gamma(chain) * mag)
    return g


def ambiguous_relu_fraction(g: Dict[str, Tuple[Tensor, Tensor]]) -> float:
    """the share of h whose mask the device may read differently: |h64| <= E_h where the exact pre-activation is within its bound of zero"""
    h, Eh = g['_h']
    return float(((h <= Eh) & (Eh > 0)).double().mean()) if h.numel() else 0.0


def autograd_grads(sd, x, edge_index, tar_ei, k, dout, last_update=None, edge_time=None, duplicate_targets='last', dtype=F64) -> Dict[str, Tensor]:
    """float64 (or ``dtype``) autograd of ``ncn_restate.forward``.  That restatement takes in-range ids only, so an edge with an endpoint outside [0, N)
    is left out, and a pair with a target outside goes through a zero ``xs`` row (out = W2 relu(b1) + b2) and takes no part in the
    'last' rule -- what the device's forward does."""
    x64 = torch.as_tensor(x).detach().cpu().to(dtype).requires_grad_()
    N = x64.shape[0]
    p = {n: sd[n].detach().cpu().to(dtype).requires_grad_() for n in PARAMS}
    tar = torch.as_tensor(tar_ei).detach().cpu().long()
    ei = torch.as_tensor(edge_index).detach().cpu().long()
    ei = ei[:, ((ei >= 0) & (ei < N)).all(dim=0)]
    ok = ((tar >= 0) & (tar < N)).all(dim=0)
    O = p['xsmlp.2.weight'].shape[0]
    dY = torch.as_tensor(dout).detach().cpu().to(dtype).reshape(tar.shape[1], O)
    et = None if edge_time is None else torch.as_tensor(edge_time).reshape(-1)[ok]
    out = nr.forward(p, x64, ei, tar[:, ok], k, last_update, et, duplicate_targets, dtype=dtype).reshape(-1, O)
    loss = (out * dY[ok]).sum() + ((torch.relu(p['xsmlp.0.bias']) @ p['xsmlp.2.weight'].t() + p['xsmlp.2.bias']) * dY[~ok]).sum()
    loss.backward()
    res = {n: (v.grad if v.grad is not None else torch.zeros_like(v)) for n, v in p.items()}
    res['x'] = x64.grad if x64.grad is not None else torch.zeros_like(x64)
    return res


# ---- the recorded gradients (tests/golden/make_golden_ncn_grads.py) -----------------------------------------------------------------------------
EXPECTED_GRAD_FIXTURES = ['k2_decay', 'k2_plain', 'k4_decay', 'k4_plain', 'onevsmany', 'selfloop']


def grad_fixture_names():
    return sorted(os.path.basename(p)[len('g31_ncn_grad_') : -len('.npz')] for p in glob.glob(os.path.join(GOLDEN, 'g31_ncn_grad_*.npz')))


def load_grad_fixture(name: str):
    """(meta, state_dict, inputs: x / edge_index / tar_ei / last_update / edge_time, upstream gradient, the reference's float32 gradients)"""
    with np.load(os.path.join(GOLDEN, f'g31_ncn_grad_{name}.npz')) as f:
        meta = json.loads(bytes(f['meta']).decode())
        sd = {k[2:]: torch.from_numpy(f[k]) for k in meta['keys']}
        inputs = {k: (torch.from_numpy(f[k]) if k in f.files else None) for k in ('x', 'edge_index', 'tar_ei', 'last_update', 'edge_time')}
        grads_ = {k[2:]: torch.from_numpy(f[k]) for k in f.files if k.startswith('g.')}
        return meta, sd, inputs, torch.from_numpy(f['dout']), grads_
