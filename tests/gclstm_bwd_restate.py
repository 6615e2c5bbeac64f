"""The backward of the GCLSTM cell restated in float64 (or float32 on request), pure torch on the CPU, in the manner of
``oracle/tgn_bwd_ref.py``: every function returns ``(value, magnitude)`` pairs -- the value and, with the same shape, the same formula with
every term replaced by its absolute value.  A worst-case rounding bound for a float32 evaluation is ``n * 2^-24 * magnitude`` with ``n``
from the chain helpers below (counted from ``csrc/cheb_bwd.hip``).  ``mutate=`` names a deliberately wrong variant (``MUTATIONS``).

Magnitudes follow the oracle's rules: a difference counts as the sum of its terms' magnitudes (``1 - I`` as ``1 + I``, ``1 - T^2`` as
``1 + T^2``).  The gate pre-activations ARE inputs here (the forward saved them as float32), so a sigmoid or tanh of one counts as its own
value; ``tanh(C')`` is a function of a rounded sum and counts as ``|tanh| + (1 - tanh^2) * magnitude(C')``.

Nothing here imports the product or the reference; the forward comes from ``gclstm_restate.py``.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

import gclstm_restate as gr
from oracle.tgat_bwd_ref import EPS, F64
from oracle.tgn_bwd_ref import FLT_MIN, TRANSCENDENTAL_OPS

GATE_CASES = [(1, 1), (5, 3), (7, 100)]
GATE_BIG_CASE = (41944, 100)  # 4 194 400 elements = 16384 * 256 + 96: the second grid-stride trip carries exactly the tail
GATE_BAND = (30.0, -30.0, 95.0, -95.0)

# deliberately wrong variants: name -> (the part they live in, the condition under which they can show)
MUTATIONS = {
    'dCprev_without_F': ('gate', lambda **_: True),
    'one_minus_T': ('gate', lambda **_: True),  # 1 - T for 1 - T^2
    'clenshaw_without_b_k2': ('clenshaw', lambda K=1, **_: K >= 3),
    'L_for_LT': ('clenshaw', lambda K=1, **_: K >= 2),  # the forward's operator instead of its transpose
}


# ---- the gates ------------------------------------------------------------------------------------------------------------------------------
def gate_backward(pre: Tensor, Cprev: Tensor, dH: Optional[Tensor], dC: Optional[Tensor], dtype=F64, mutate=None):
    """pre [N, 4C] (gates i, f, c, o), Cprev [N, C]; dH / dC [N, C] or None (zero):

        I, F, O = s(pre_i), s(pre_f), s(pre_o), T = tanh(pre_c), C' = F Cprev + I T, tc = tanh(C')
        dCn = dC + dH O (1 - tc^2);  dpre = [dCn T I(1-I) | dCn Cprev F(1-F) | dCn I (1-T^2) | dH tc O(1-O)];  dCprev = dCn F

    Returns (dpre, dCprev, dpre_mag, dCprev_mag)."""
    C = Cprev.shape[1]
    pre, cp = pre.to(dtype), Cprev.to(dtype)
    gh = torch.zeros_like(cp) if dH is None else dH.to(dtype)
    gc = torch.zeros_like(cp) if dC is None else dC.to(dtype)
    I, F, O = torch.sigmoid(pre[:, :C]), torch.sigmoid(pre[:, C:2 * C]), torch.sigmoid(pre[:, 3 * C:])
    T = torch.tanh(pre[:, 2 * C:3 * C])
    cn, cn_m = F * cp + I * T, F * cp.abs() + I * T.abs()
    tc = torch.tanh(cn)
    tc_m = tc.abs() + (1 - tc * tc) * cn_m
    dcn, dcn_m = gc + gh * O * (1 - tc * tc), gc.abs() + gh.abs() * O * (1 + tc_m * tc_m)
    dT, dT_m = ((1 - T), (1 + T.abs())) if mutate == 'one_minus_T' else ((1 - T * T), (1 + T * T))
    dpre = torch.cat([dcn * T * I * (1 - I), dcn * cp * F * (1 - F), dcn * I * dT, gh * tc * O * (1 - O)], 1)
    dpre_m = torch.cat([dcn_m * T.abs() * I * (1 + I), dcn_m * cp.abs() * F * (1 + F), dcn_m * I * dT_m, gh.abs() * tc_m * O * (1 + O)], 1)
    dcp, dcp_m = (dcn, dcn_m) if mutate == 'dCprev_without_F' else (dcn * F, dcn_m * F)
    return dpre, dcp, dpre_m, dcp_m


def gate_chain() -> int:
    """float32 operations on the longest chain into an element (dpre_i / dpre_f), plus 8, counted from gclstm_gate_backward_kernel:
    a sigmoid = expf, add, divide (4 + 2; the negation is exact);  cn = F * cp + I * T (2);  tanhf (4);  tc * tc, 1 - .. (2);
    gh * O * (..) (2);  gc + .. (1);  dcn * T * I * (1 - I) (3: the subtraction runs beside the chain).  20 + 8."""
    return TRANSCENDENTAL_OPS + 2 + 2 + TRANSCENDENTAL_OPS + 2 + 2 + 1 + 3 + 8


def gate_underflow_floor(*inputs) -> float:
    """The absolute floor of the bound on the saturated rows (``gru_underflow_floor``'s kind).  Every output is (|dC'| + |dH'|) times |Cprev|
    or 1, times factors in [0, 1] -- with A the largest input magnitude, at most 2 A (A + 1).  float32 keeps no relative precision in a
    factor below its smallest normal 2^-126 (at +-95 ``expf`` overflows or lands in the denormals: the sigmoid is exactly 0 or 1 where
    float64 has 5e-42), so the output is uncertain by up to 2^-126 * 2 A (A + 1)."""
    A = max(float(t.abs().max()) for t in inputs if t is not None)
    return FLT_MIN * 2.0 * A * (A + 1.0)


def gate_case(N: int, C: int, seed: int = 0, saturate_all: bool = False) -> Dict[str, object]:
    """pre [N, 4C], Cprev, dH, dC [N, C]: randn.  N >= 3: rows 1 .. min(4, N - 2) are the saturated band -- gate g of column c of row r
    has the pre-activation GATE_BAND[(r + c + g) % 4], exactly +-30 or +-95.  ``saturate_all``: every row is (the one-row cases)."""
    g = torch.Generator().manual_seed(seed * 7919 + N * 331 + C)
    pre = torch.randn(N, 4 * C, generator=g)
    Cprev, dH, dC = (torch.randn(N, C, generator=g) for _ in range(3))
    band = list(range(N)) if saturate_all else (list(range(1, min(4, N - 2) + 1)) if N >= 3 else [])
    col = torch.arange(C)
    for r in band:
        for gate in range(4):
            pre[r, gate * C:(gate + 1) * C] = torch.tensor(GATE_BAND)[(r + col + gate) % 4]
    return dict(pre=pre, Cprev=Cprev, dH=dH, dC=dC, band=band)


def gate_bounds(c, dH=True, dC=True):
    """((dpre, dCprev), (bound_dpre, bound_dCprev)): the band's rows get the underflow floor on top."""
    gh, gc = (c['dH'] if dH else None), (c['dC'] if dC else None)
    dpre, dcp, mp, mc = gate_backward(c['pre'], c['Cprev'], gh, gc)
    floor = torch.zeros(c['Cprev'].shape[0], 1, dtype=F64)
    floor[c['band']] = gate_underflow_floor(c['pre'], c['Cprev'], gh, gc)
    n = gate_chain() * EPS
    return (dpre, dcp), (n * mp + floor, n * mc + floor)


# ---- the reverse recurrence -------------------------------------------------------------------------------------------------------------------
def propagate_t(lap, t: Tensor, mag: bool = False) -> Tensor:
    """L_hat^T t (``gclstm_restate.propagate`` with the entry's endpoints swapped); ``mag``: with |m| and |d|."""
    row, col, m, d = lap
    if mag:
        m, d = m.abs(), d.abs()
    out = d.unsqueeze(1) * t
    if row.numel():
        out = out.index_add(0, row, m.unsqueeze(1) * t[col])
    return out


def _propagate_mag(lap, t: Tensor) -> Tensor:
    row, col, m, d = lap
    return gr.propagate((row, col, m.abs(), d.abs()), t)


def clenshaw(lap, g: Tensor, K: int, dtype=F64, mutate=None) -> Tuple[Tensor, Tensor]:
    """g [N, K C]: the gradient at Tx_k in the columns [k C, (k + 1) C).  b_K = b_{K+1} = 0, b_k = g_k + 2 L^T b_{k+1} - b_{k+2}
    (k = K - 1 .. 1), dH = g_0 + L^T b_1 - b_2.  ``lap`` = (row, col, m, d) of ``gclstm_restate.scaled_laplacian``.  Returns (dH, dH_mag)."""
    lap = tuple(t if i < 2 else t.to(dtype) for i, t in enumerate(lap))
    g = g.to(dtype)
    C = g.shape[1] // K
    gk = [g[:, k * C:(k + 1) * C] for k in range(K)]
    fwd = mutate == 'L_for_LT'
    app = (lambda t: gr.propagate(lap, t)) if fwd else (lambda t: propagate_t(lap, t))
    app_m = (lambda t: _propagate_mag(lap, t)) if fwd else (lambda t: propagate_t(lap, t, mag=True))
    zero = torch.zeros_like(gk[0])
    b1, b2, m1, m2 = zero, zero, zero, zero  # b_{k+1}, b_{k+2} and their magnitudes
    for k in range(K - 1, 0, -1):
        b, m = gk[k] + 2.0 * app(b1), gk[k].abs() + 2.0 * app_m(m1) + m2
        if mutate != 'clenshaw_without_b_k2':
            b = b - b2
        b1, b2, m1, m2 = b, b1, m, m1
    dH = gk[0] + app(b1)
    if mutate != 'clenshaw_without_b_k2':
        dH = dH - b2
    return dH, gk[0].abs() + app_m(m1) + m2


def out_degrees(lap, N: int) -> Tensor:
    """entries per row of L_hat^T: the kept edges leaving each node"""
    return torch.bincount(lap[0], minlength=N)


def clenshaw_chain(K: int, row_len, longest: int):
    """float32 operations on the longest chain into an element of dH, plus 8, counted from spmm.h / Cheb2Epi: a propagation adds a row's
    entries one fma each (L), the diagonal fma (1), alpha (1) and the two addends (2).  The last step runs over the element's own row
    (``row_len``, a number or a tensor), each of the K - 2 before it over rows of at most ``longest`` entries."""
    return (row_len + 4) + max(K - 2, 0) * (longest + 4) + 8


# ---- the whole cell -----------------------------------------------------------------------------------------------------------------------------
def forward_saved(sd, x, edge_index, edge_weight, H, C, lambda_max, normalization, rounded: bool = False):
    """What the forward keeps for the backward, float64: op = [x | Tx_0 .. Tx_{K-1}], pre [N, 4C], C, the Laplacian's entries.
    ``rounded``: every saved activation goes through float32, as the device keeps it."""
    sd = {k: torch.as_tensor(v).to(F64) for k, v in sd.items()}
    x = torch.as_tensor(x).to(F64)
    N, Co = x.shape[0], sd['W_i'].shape[1]
    K = sum(1 for k in sd if k.startswith('conv_i.lins.'))
    H = torch.zeros(N, Co, dtype=F64) if H is None else torch.as_tensor(H).to(F64)
    C = torch.zeros(N, Co, dtype=F64) if C is None else torch.as_tensor(C).to(F64)
    lap = gr.scaled_laplacian(edge_index, edge_weight, N, normalization, lambda_max, F64)
    tx = gr.cheb_basis(lap, H, K)
    pre = []
    for g in gr.GATES:
        conv = sum(tx[k] @ sd[f'conv_{g}.lins.{k}.weight'].t() for k in range(K))
        if f'conv_{g}.bias' in sd:
            conv = conv + sd[f'conv_{g}.bias']
        pre.append(x @ sd[f'W_{g}'] + conv + sd[f'b_{g}'])
    op, pre = torch.cat([x] + tx, 1), torch.cat(pre, 1)
    if rounded:
        op, pre, C = op.float().double(), pre.float().double(), C.float().double()
        lap = (lap[0], lap[1], lap[2].float().double(), lap[3].float().double())
    return dict(op=op, pre=pre, C=C, lap=lap, K=K, cin=x.shape[1], Co=Co, N=N)


def cell_backward(sd, saved, dH: Optional[Tensor], dC: Optional[Tensor], dtype=F64, mutate=None) -> Dict[str, Tuple[Tensor, Tensor]]:
    """The launch list of ``tgmx_gclstm_backward`` as formulas: name -> (gradient, magnitude) for every key of ``sd`` and for
    ``node_x``, ``H``, ``C``."""
    K, cin, Co = saved['K'], saved['cin'], saved['Co']
    op = saved['op'].to(dtype)
    dpre, dcp, dpre_m, dcp_m = gate_backward(saved['pre'], saved['C'], dH, dC, dtype, mutate)
    out = {'C': (dcp, dcp_m)}
    x, tx = op[:, :cin], [op[:, cin + k * Co: cin + (k + 1) * Co] for k in range(K)]
    g_x, g_xm = torch.zeros_like(x), torch.zeros_like(x)
    g_tx, g_txm = [torch.zeros_like(tx[0]) for _ in range(K)], [torch.zeros_like(tx[0]) for _ in range(K)]
    for i, g in enumerate(gr.GATES):
        d, dm = dpre[:, i * Co:(i + 1) * Co], dpre_m[:, i * Co:(i + 1) * Co]
        W = sd[f'W_{g}'].to(dtype)
        out[f'W_{g}'] = (x.t() @ d, x.abs().t() @ dm)
        out[f'b_{g}'] = (d.sum(0, keepdim=True), dm.sum(0, keepdim=True))
        if f'conv_{g}.bias' in sd:
            out[f'conv_{g}.bias'] = (d.sum(0), dm.sum(0))
        g_x, g_xm = g_x + d @ W.t(), g_xm + dm @ W.abs().t()
        for k in range(K):
            L = sd[f'conv_{g}.lins.{k}.weight'].to(dtype)
            out[f'conv_{g}.lins.{k}.weight'] = (d.t() @ tx[k], dm.t() @ tx[k].abs())
            g_tx[k], g_txm[k] = g_tx[k] + d @ L, g_txm[k] + dm @ L.abs()
    out['node_x'] = (g_x, g_xm)
    dHp, _ = clenshaw(saved['lap'], torch.cat(g_tx, 1), K, dtype, mutate)
    _, dHm = clenshaw(saved['lap'], torch.cat(g_txm, 1), K, dtype, mutate)  # (magnitudes in, magnitudes out: every term is non-negative)
    out['H'] = (dHp, dHm)
    return out


def cell_chain(saved) -> int:
    """One figure for every gradient of the cell: the gate chain, the longest sum behind it (N rows into a weight, 4C columns into a data
    gradient) and the K - 1 propagations over rows of at most the largest out-degree."""
    longest = int(out_degrees(saved['lap'], saved['N']).max()) if saved['lap'][0].numel() else 0
    return gate_chain() + max(saved['N'], 4 * saved['Co']) + clenshaw_chain(saved['K'], longest, longest)


def parse_mode(value: Optional[str]) -> str:
    """``TGMX_GCLSTM_BWD`` as the product reads it: 'py' and 'torch' are themselves, anything else is the one call."""
    return value if value in ('py', 'torch') else 'native'
