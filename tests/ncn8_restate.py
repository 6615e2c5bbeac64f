"""NCNPredictor at k = 8 (two-hop common neighbours) restated densely in float64, in the words of ncn_restate.py, whose helpers it uses; the
CPU and GPU tests and the fixture generator share it.

    A, R_i, I_i, W   as in ncn_restate.py;  keep_i[r]: r is the LAST position of tar_i[r] in tar_i ('all': every r);  both = keep_i keep_j
    A2 = A A,  K3 = A2 A
    S_i[r]    A2[tar_i[r]] keep_i[r]
    u[r]      -A[tar_i[r], tar_j[r]] both[r]
    c01 = I_i o R_j    c10 = R_i o I_j    c11 = R_i o R_j
    sp  = c11 A                                                                        ("special_2_2")
    c12 = R_i o S_j + R_i o R_i u
    c21 = S_i o R_j + R_j o R_j u
    c22 = S_i o S_j + ([R_i > 0] K3[tar_i, tar_i] keep_i + [R_j > 0] K3[tar_j, tar_j] keep_j - c11) u + sp
    c12, c21, c22: columns tar_i[r] and tar_j[r] of row r are set to 0; then c22 = max(c22, 0)
    cn_emb    [(c01 o W) x | (c10 o W) x | (c11 o W) x | (c12 o W) x | (c21 o W) x | (c22 o W) x | sp x]     (sp: no decay, no masking)
    xs        [x[tar_i] * x[tar_j] | cn_emb]  (8 C wide);  out = Linear(relu(Linear(xs))).view(-1)  (the discarded relu as at k = 2 / 4)

``drop`` leaves one step out ('masks', 'clamp', 'u'): the tests show with it that the step matters in a fixture.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

import ncn_restate as nr

BLOCKS = ('c01', 'c10', 'c11', 'c12', 'c21', 'c22', 'sp')


def coefficients(num_nodes: int, edge_index, tar_ei, duplicate_targets: str = 'last', dtype=torch.float64, drop: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """The seven [B, N] coefficient matrices (before W), and what they were made of: A, K3 diagonals, u, R / S rows, c22 before the column
    masks and the clamp (``c22_raw``), c12 / c21 before the masks (``c12_raw`` / ``c21_raw``).  Only the targets' rows of A A are formed
    (A A and A A A are [N, N]; K3[t, t] = sum over m of (A A)[t, m] A[t, m], A being symmetric)."""
    N = num_nodes
    tar = nr._t(tar_ei, torch.int64)
    ti, tj = tar[0], tar[1]
    B = ti.numel()
    ar = torch.arange(B)
    A = nr.dense_adjacency(N, edge_index, dtype)
    ki, kj = nr.kept_rows(ti, duplicate_targets).to(dtype)[:, None], nr.kept_rows(tj, duplicate_targets).to(dtype)[:, None]
    both = ki * kj
    Ii, Ij = torch.zeros((B, N), dtype=dtype), torch.zeros((B, N), dtype=dtype)
    Ii[ar, ti], Ij[ar, tj] = 1.0, 1.0
    Ri, Rj, Ii, Ij = A[ti] * ki, A[tj] * kj, Ii * ki, Ij * kj
    Si, Sj = Ri @ A, Rj @ A
    u = -A[ti, tj][:, None] * both
    if drop == 'u':
        u = torch.zeros_like(u)
    c01, c10, c11 = Ii * Rj, Ri * Ij, Ri * Rj
    sp = c11 @ A
    c12 = Ri * Sj + Ri * Ri * u
    c21 = Si * Rj + Rj * Rj * u
    k3i, k3j = (Si * Ri).sum(dim=1, keepdim=True), (Sj * Rj).sum(dim=1, keepdim=True)  # K3[tar_i, tar_i] keep_i, K3[tar_j, tar_j] keep_j
    c22 = Si * Sj + ((Ri > 0).to(dtype) * k3i + (Rj > 0).to(dtype) * k3j - c11) * u + sp
    raw = dict(c12_raw=c12.clone(), c21_raw=c21.clone(), c22_raw=c22.clone())
    if drop != 'masks':
        for c in (c12, c21, c22):
            c[ar, ti] = 0
            c[ar, tj] = 0
    if drop != 'clamp':
        c22 = c22.clamp(min=0)
    return dict(c01=c01, c10=c10, c11=c11, c12=c12, c21=c21, c22=c22, sp=sp, A=A, k3i=k3i, k3j=k3j, u=u, Ri=Ri, Rj=Rj, Si=Si, Sj=Sj, **raw)


def cn_emb(x, edge_index, tar_ei, last_update=None, edge_time=None, duplicate_targets: str = 'last', dtype=torch.float64,
           drop: Optional[str] = None) -> torch.Tensor:
    x = nr._t(x, dtype)
    co = coefficients(x.shape[0], edge_index, tar_ei, duplicate_targets, dtype, drop)
    W = 1.0 if last_update is None else nr.decay_weights(last_update, edge_time, dtype)
    return torch.cat([(co[b] * W) @ x for b in BLOCKS[:-1]] + [co['sp'] @ x], dim=-1)


def forward(sd: Dict[str, torch.Tensor], x, edge_index, tar_ei, last_update=None, edge_time=None, duplicate_targets: str = 'last',
            dtype=torch.float64) -> torch.Tensor:
    x = nr._t(x, dtype)
    tar = nr._t(tar_ei, torch.int64)
    xs = torch.cat([x[tar[0]] * x[tar[1]], cn_emb(x, edge_index, tar, last_update, edge_time, duplicate_targets, dtype)], dim=-1)
    w = lambda n: sd[n].to(dtype) if not sd[n].requires_grad else sd[n]
    h = F.linear(xs, w('xsmlp.0.weight'), w('xsmlp.0.bias')).relu()
    return F.linear(h, w('xsmlp.2.weight'), w('xsmlp.2.bias')).reshape(-1)
