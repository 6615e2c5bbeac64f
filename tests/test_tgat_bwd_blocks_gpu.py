"""The six public building blocks of ``csrc/tgat_bwd.hip`` one by one against the float64 restatements of ``oracle/tgat_bwd_ref.py``
(which ``tests/test_tgat_bwd_ref_cpu.py`` pins to autograd): ``tgmx_sgemm_tn``, ``tgmx_colsum``, ``tgmx_relu_mask``,
``tgmx_add_cols``, ``tgmx_ln_backward`` and ``tgmx_tgat_attn_backward`` at every dispatch edge, through ctypes.

Every test here
* pre-fills outputs and workspaces with NaN (a known non-zero value where the call accumulates), gives them sentinel columns past
  the width (ld > width) and a sentinel tail of 4096 floats, and requires the sentinels unchanged: an out-of-range write inside the
  test's own allocation shows; nothing is handed to a kernel that it may not touch;
* launches twice and requires equal bits (the kernels are deterministic);
* reaches a kernel through a shape that dispatches to it: the A/B knobs (TGMX_ATTN_BWD_REG, ..._REG_NBV, ..._WPB) are read once per
  process and stay unset.

Bars: exact (``torch.equal``) for relu_mask, add_cols, the integer variants of sgemm_tn / colsum and the structural zeros;
``2e-5 * sqrt(R)`` for sgemm_tn / colsum on randn inputs (the bar of tests/test_gemm_gpu.py with the reduction length in place of K);
elementwise ``n * 2^-24 * magnitude`` for ln_backward (n = 2 O + 16) and the attention backward (n = C + H k + 8, + k for dtime),
the magnitude being the restatement's formula with absolute values.  ``pytest -rP`` prints the worst err / bound per case.
"""
import functools

import pytest
import torch

from oracle import tgat_bwd_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TAIL = 4096
NAN = float('nan')


def _lib():
    from tgm_amd import _native

    return _native.load(), _native


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class Buf:
    """A device matrix [rows, width] inside a wider, longer allocation: ``lead`` columns before it and the rest of ``ld`` after it hold
    ``fill``, and so does a tail of TAIL floats behind the last row.  ``view`` is the matrix, ``ptr`` its first element."""

    def __init__(self, rows, width, ld=None, lead=0, fill=NAN, data=None):
        ld = ld or width
        assert lead + width <= ld
        self.flat = torch.full((max(rows, 1) * ld + TAIL,), fill, dtype=torch.float32, device=DEV)
        self.fill, self.rows, self.width, self.ld, self.lead = fill, rows, width, ld, lead
        self.full = self.flat[: max(rows, 1) * ld].view(max(rows, 1), ld)
        self.view = self.full[:rows, lead:lead + width]
        if data is not None:
            self.view.copy_(data)
        self.ptr = self.flat.data_ptr() + 4 * lead

    def sentinels_intact(self):
        probe = torch.full_like(self.flat, self.fill)
        inside = torch.zeros_like(self.flat, dtype=torch.bool)
        inside[: max(self.rows, 1) * self.ld].view(max(self.rows, 1), self.ld)[: self.rows, self.lead:self.lead + self.width] = True
        return torch.equal(_bits(self.flat[~inside]), _bits(probe[~inside]))


def _report(tag, got, want, bound):
    """Prints the worst err / bound (pytest -rP) and returns it; ``bound`` a number or a tensor like ``want``."""
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == want.shape, f'{tag}: {got.shape} {got.dtype} vs {want.shape}'
    assert torch.isfinite(got).all(), f'{tag}: non-finite output'
    b = bound if torch.is_tensor(bound) else torch.full_like(want, bound)
    worst = ref.worst_ratio(got, want, b)
    print(f'[blocks] {tag}: max abs err {float((got.double() - want).abs().max()) if want.numel() else 0.0:.3e}, {worst:.4f}x the bound')
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_sgemm_tn
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tn_inputs(case, integer):
    """A [R, batch * M] (heads side by side), B, their float64 product [batch, M, N] -- computed once per case."""
    R, M, N, batch = case
    g = torch.Generator().manual_seed(R * 31 + M * 7 + N + batch)
    shared_b = case == (600, 86, 172, 2)  # the W_Q layout: every head multiplies the same B (strideB = 0)
    A = ref.randn_or_int((R, batch, M), integer, g)
    B = ref.randn_or_int((R, 1 if shared_b else batch, N), integer, g)
    want = ref.sgemm_tn(A.permute(1, 0, 2), B.expand(R, batch, N).permute(1, 0, 2))[0]
    return A, B, want, shared_b


@pytest.mark.parametrize('integer', [False, True], ids=['randn', 'int'])
@pytest.mark.parametrize('layout,accumulate', [('dense', 0), ('slices', 0), ('slices', 1)])
@pytest.mark.parametrize('case', ref.SGEMM_TN_CASES, ids=str)
def test_sgemm_tn(case, layout, accumulate, integer):
    """(R, M, N, batch).  pick_splits: s = min(ceil(2048 / tiles), ceil(R / 64), 512), rows_per_split = ceil(R / s) rounded up to 8.
    (0,5,7): no rows -- zeros, or C kept under accumulate.  (7,33,65): ragged 32 x 64 tiles, clamped edge loads.  (65,32,64): two
    splits of 33 -> 40 rows.  (300,128|129,64): the fourth wave's tile ends / a second workgroup with one live wave.
    (1345,320,640): 100 tiles -> 21 splits of 65 -> 72 rows, the last two empty.  (33000,8,12): the 512-split cap.
    (12600,172,344): the headline fc1 gradient.  (600,86,273,2): heads side by side, sA = 86, sB = 276 (the W_V fold).
    (600,86,172,2): sB = 0, a shared B (the W_Q layout).  'slices': A, B column slices (odd first column) of wider tensors, ldc > N."""
    lib, native = _lib()
    R, M, N, batch = case
    A, B, want, shared_b = _tn_inputs(case, integer)
    nb = 1 if shared_b else batch
    ldb_heads = 276 if case == (600, 86, 273, 2) else N  # floats between the heads' blocks of B
    wide = layout == 'slices'
    bA = Buf(R, batch * M, ld=batch * M + (5 if wide else 0), lead=3 if wide else 0, fill=7.0, data=A.reshape(R, batch * M))
    bB = Buf(R, nb * ldb_heads, ld=nb * ldb_heads + (7 if wide else 0), lead=1 if wide else 0, fill=7.0)
    if R:
        bB.view.unflatten(1, (nb, ldb_heads))[:, :, :N].copy_(B)
    ldc = N + (3 if wide else 0)
    g = torch.Generator().manual_seed(9)
    c0 = ref.randn_or_int((batch * M, N), integer, g) if accumulate else torch.full((batch * M, N), NAN)
    ws_bytes = lib.tgmx_sgemm_tn_workspace_bytes(R, M, N, batch)
    assert ws_bytes % 4 == 0 and ws_bytes >= 4 * M * N * batch
    outs = []
    for _ in range(2):
        bC = Buf(batch * M, N, ld=ldc, fill=3.0, data=c0)
        ws = Buf(1, ws_bytes // 4)
        native.check(lib.tgmx_sgemm_tn(bA.ptr, bA.ld, bB.ptr, bB.ld, bC.ptr, ldc, R, M, N, batch, M, 0 if shared_b else ldb_heads, M * ldc,
                                       accumulate, ws.ptr, native.stream_ptr()), 'sgemm_tn')
        torch.cuda.synchronize()
        assert bC.sentinels_intact(), 'C: a write outside [M, N]'
        assert ws.sentinels_intact(), 'workspace: a write past tgmx_sgemm_tn_workspace_bytes'
        outs.append(bC.view.contiguous().clone())
    assert _same_bits(outs[0], outs[1]), 'two launches differ'
    got = outs[0].reshape(batch, M, N)
    full = want + c0.view(batch, M, N).double() if accumulate else want
    if integer or R == 0:  # every partial sum is an integer below 2^24: float32 is exact, and so must the result be
        assert torch.equal(got.cpu().double(), full), f'{int((got.cpu().double() != full).sum())} elements differ'
    else:
        assert _report(f'sgemm_tn {case} {layout} acc={accumulate}', got, full, ref.gemm_bar(R)) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_colsum
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('integer', [False, True], ids=['randn', 'int'])
@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('case', ref.COLSUM_CASES, ids=str)
def test_colsum(case, accumulate, integer):
    """(R, C).  splits = min(ceil(R / 64), 256): (63,5) one split, (64,256) a full 256-column block, (65,257) two splits and a second
    column block of one live lane, (16400,7) 257 -> the 256-split cap, (12600,200) a column slice with ld = 2 C like dtime[:, T:]."""
    lib, native = _lib()
    R, C = case
    x = ref.randn_or_int((R, C), integer, torch.Generator().manual_seed(R * 3 + C))
    want = ref.colsum(x)[0]
    bX = Buf(R, C, ld=2 * C, lead=C, fill=7.0, data=x) if case == (12600, 200) else Buf(R, C, ld=C + 3, lead=1, fill=7.0, data=x)
    o0 = ref.randn_or_int((1, C), integer, torch.Generator().manual_seed(4)) if accumulate else torch.full((1, C), NAN)
    outs = []
    for _ in range(2):
        bO = Buf(1, C, fill=3.0, data=o0)
        ws = Buf(1, 256 * C)
        native.check(lib.tgmx_colsum(bX.ptr, bX.ld, R, C, bO.ptr, accumulate, ws.ptr, native.stream_ptr()), 'colsum')
        torch.cuda.synchronize()
        assert bO.sentinels_intact() and ws.sentinels_intact(), 'a write past out[C] or past the 256 * C workspace'
        outs.append(bO.view.clone())
    assert _same_bits(outs[0], outs[1]), 'two launches differ'
    full = want + o0[0].double() if accumulate else want
    if integer or R == 0:
        assert torch.equal(outs[0][0].cpu().double(), full)
    else:
        assert _report(f'colsum {case} acc={accumulate}', outs[0][0], full, ref.gemm_bar(R)) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_relu_mask, tgmx_add_cols
# ---------------------------------------------------------------------------------------------------------------------------
def _activations(R, C, g):
    """0.0, -0.0, tiny positives and negatives (denormals included) among ordinary values."""
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38, 1e-30, -1e-30])
    h = torch.randn(R, C, generator=g)
    pick = torch.randint(0, 16, (R, C), generator=g)
    return torch.where(pick < 8, special[pick.clamp(max=7)], h)


ELEMENTWISE_SHAPES = [(1, 1), (5, 3), (20000, 211)]  # 4.22 M elements > 16 384 blocks x 256: the grid-stride loop runs


@pytest.mark.parametrize('R,C', ELEMENTWISE_SHAPES)
def test_relu_mask(R, C):
    lib, native = _lib()
    g = torch.Generator().manual_seed(R + C)
    grad, act = torch.randn(R, C, generator=g), _activations(R, C, g)
    want = ref.relu_mask(grad, act)[0]
    bH = Buf(R, C, ld=C + 8, lead=5, fill=1.0, data=act)  # (the padding of the activations is positive: reading it would keep a gradient)
    outs = []
    for _ in range(2):
        bG = Buf(R, C, ld=C + 4, lead=1, fill=3.0, data=grad)
        native.check(lib.tgmx_relu_mask(bG.ptr, bG.ld, bH.ptr, bH.ld, R, C, native.stream_ptr()), 'relu_mask')
        torch.cuda.synchronize()
        assert bG.sentinels_intact(), 'a write outside [R, C]'
        outs.append(bG.view.clone())
    assert _same_bits(outs[0], outs[1])
    assert torch.equal(outs[0].cpu().double(), want)


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('R,C', ELEMENTWISE_SHAPES)
def test_add_cols(R, C, accumulate):
    lib, native = _lib()
    g = torch.Generator().manual_seed(R + C + 1)
    src, dst0 = _activations(R, C, g), torch.randn(R, C, generator=g) if accumulate else torch.full((R, C), NAN)
    want = ref.add_cols(dst0, src, accumulate)[0]
    bS = Buf(R, C, ld=C + 8, lead=5, fill=7.0, data=src)
    outs = []
    for _ in range(2):
        bD = Buf(R, C, ld=C + 4, lead=1, fill=3.0, data=dst0)
        native.check(lib.tgmx_add_cols(bD.ptr, bD.ld, bS.ptr, bS.ld, R, C, accumulate, native.stream_ptr()), 'add_cols')
        torch.cuda.synchronize()
        assert bD.sentinels_intact(), 'a write outside [R, C]'
        outs.append(bD.view.clone())
    assert _same_bits(outs[0], outs[1])
    # (one float32 addition: the float64 sum of two float32 values rounded to float32 IS the float32 sum -- 53 >= 2 * 24 + 2 bits)
    assert torch.equal(outs[0].cpu(), want.float())


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_ln_backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', ref.LN_ROWS)
@pytest.mark.parametrize('O', ref.LN_WIDTHS)
def test_ln_backward(O, R):
    """One wave per row, four rows per workgroup (R = 1, 2, 5, 37: the last group is ragged); O = 64 | 65: one / two columns per
    lane, 300: five.  Every ld is larger than O.  O = 1: du must be exactly 0."""
    lib, native = _lib()
    dout, y, res, gamma = ref.ln_case(R, O)
    eps = 1e-5
    du, dgx, du_mag, dgx_mag = ref.ln_backward(dout, y, res, gamma, eps)
    bD, bY, bR = Buf(R, O, ld=O + 3, lead=1, data=dout), Buf(R, O, ld=O + 5, lead=2, data=y), Buf(R, O, ld=O + 1, data=res)
    bG = Buf(1, O, data=gamma[None])
    outs = []
    for _ in range(2):
        bU, bX = Buf(R, O, ld=O + 2, lead=1), Buf(R, O, ld=O + 7, lead=3)
        native.check(lib.tgmx_ln_backward(bD.ptr, bD.ld, bY.ptr, bY.ld, bR.ptr, bR.ld, bG.ptr, O, eps, R, bU.ptr, bU.ld, bX.ptr, bX.ld,
                                          native.stream_ptr()), 'ln_backward')
        torch.cuda.synchronize()
        assert bU.sentinels_intact() and bX.sentinels_intact(), 'a write outside [R, O]'
        outs.append((bU.view.clone(), bX.view.clone()))
    assert _same_bits(outs[0][0], outs[1][0]) and _same_bits(outs[0][1], outs[1][1])
    n = ref.ln_chain(O) * ref.EPS
    if O == 1:
        assert torch.equal(outs[0][0].cpu(), torch.zeros(R, 1))
    else:
        assert _report(f'ln_backward du O={O} R={R}', outs[0][0], du, n * du_mag) <= 1.0
    assert _report(f'ln_backward dgx O={O} R={R}', outs[0][1], dgx, n * dgx_mag) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tgat_attn_backward
# ---------------------------------------------------------------------------------------------------------------------------
# launch_attn_backward (csrc/tgat_bwd.hip) takes the register kernel tgat_attn_backward_reg_kernel<H, G, NBV> when
#   (H == 1 || H == 2) && k <= 20 && (d <= 64 || nbv) && D > 0 && D % 4 == 0 && D / 4 <= 64 && T <= 128 && ex (and, nbv: nbrf, dnbr) 16-byte aligned,
#   nbv = d > 64 && d % 4 == 0 && d / 4 <= 64 && R <= 2048;  G = 10 when k <= 10, else 20;
# and otherwise the LDS kernel tgat_attn_backward_kernel<H, KMAX>: KMAX = 20 when H <= 2 and k <= 20, else 64.  R = k + 8 <= 72 here.
ATTN_ROUTES = {
    (1, 5, 1, 4, 8): 'reg <1,10>: H = 1, k <= 10, d <= 64, D % 4 == 0, T <= 128',
    (1, 20, 3, 8, 128): 'reg <1,20>: H = 1, 10 < k <= 20; T = 128: both time columns of every lane live',
    (2, 10, 8, 12, 16): 'reg <2,10>: H = 2, k <= 10',
    (2, 13, 4, 16, 70): 'reg <2,20>: H = 2, k = 13 (span bodies 4, 8, 12, 16 and G = 20); T = 70: the second time column partly live',
    (2, 20, 1, 172, 100): 'reg <2,20>: the headline leaf layer (d = 1, D / 4 = 43 lanes)',
    (2, 20, 172, 172, 100): 'reg <2,20,NBV>: d = 172 > 64, d % 4 == 0, d / 4 = 43 <= 64, R = 28 <= 2048',
    (2, 4, 1, 6, 10): 'LDS <2,20>: D % 4 != 0 fails the register test',
    (2, 6, 5, 0, 9): 'LDS <2,20>: D == 0 fails the register test; no edge section',
    (2, 20, 4, 8, 130): 'LDS <2,20>: T > 128 fails the register test; three time chunks',
    (2, 20, 66, 8, 16): 'LDS <2,20>: d = 66 > 64 and d % 4 != 0 (no nbv); two column chunks',
    (2, 20, 130, 12, 16): 'LDS <2,20>: d = 130, d % 4 != 0; three column chunks',
    (2, 20, 200, 8, 16): 'reg <2,20,NBV>: d = 200 is a multiple of 4 with d / 4 = 50 <= 64 and R <= 2048, so nbv holds: 50 float4 lanes',
    (2, 20, 201, 8, 16): 'LDS <2,20>: d = 201 > 192 and d % 4 != 0 (no nbv): the chunk loop over four column chunks',
    (4, 16, 8, 12, 16): 'LDS <4,64>: H = 4 fails the register test; G = 16',
    (8, 8, 8, 4, 12): 'LDS <8,64>: H = 8; G = 8',
    (4, 1, 5, 3, 3): 'LDS <4,64>: k = 1',
    (1, 64, 4, 8, 6): 'LDS <1,64>: k > 20; all 64 lanes, both reduce-scatters of 32',
    (2, 32, 3, 4, 7): 'LDS <2,64>: k > 20; G = 32, both reduce-scatters of 32',
}
DROP_P, DROP_SEED, DROP_STREAM, DROP_ROW0 = 0.1, 0x1234ABCD5678, 6, 5


@functools.lru_cache(maxsize=None)
def _attn_inputs(shape):
    return ref.attn_case(*shape)


@functools.lru_cache(maxsize=None)
def _attn_keep(shape, drop):
    """[R, H, k]: tgmx_dropout over ones [R, H * k] with the descriptor the backward gets (element ((row0 + r) H + h) k + s)."""
    H, k = shape[0], shape[1]
    R = k + 8
    if not drop:
        return torch.ones(R, H, k)
    lib, native = _lib()
    ones, out = torch.ones(R, H * k, device=DEV), torch.full((R, H * k), NAN, device=DEV)
    native.check(lib.tgmx_dropout(ones.data_ptr(), H * k, R, H * k, native.dropout_desc(DROP_P, DROP_SEED, DROP_STREAM, DROP_ROW0), out.data_ptr(),
                                  H * k, native.stream_ptr()), 'dropout')
    torch.cuda.synchronize()
    keep = out.cpu().view(R, H, k)
    inv = torch.tensor(1.0 / (1.0 - float(torch.tensor(DROP_P))), dtype=torch.float64).float()
    assert bool(((keep == 0) | (keep == inv)).all()) and 0 < int((keep == 0).sum()) < keep.numel() // 2
    return keep


@functools.lru_cache(maxsize=None)
def _attn_reference(shape, drop, with_dnbr):
    c = _attn_inputs(shape)
    k, d = shape[1], shape[2]
    dn0 = torch.randn(c['R'], k, d, generator=torch.Generator().manual_seed(3)) if with_dnbr else None
    out = ref.attn_backward(c['qf'], c['probs'], c['dzbar'], c['nbrf'], c['ex'], c['seed_t'], c['nbr_t'], c['tw'], c['tb'], c['scale'],
                            _attn_keep(shape, drop), c['no_valid'], dn0)
    return dn0, out


def _run_attn(shape, drop, with_dnbr, strided, misalign_ex=False):
    """One configuration, launched twice: returns (case, reference, dqf [R, H, C], dnbr or None, dtime [R, 2T]) after the structural
    checks (sentinels, equal bits)."""
    lib, native = _lib()
    H, k, d, D, T = shape
    c = _attn_inputs(shape)
    R, C = c['R'], c['C']
    dn0, want = _attn_reference(shape, drop, with_dnbr)
    Cs = C + 3 if strided else C
    # a row without a valid slot carries its uniform weights NEGATED: the marker of include/tgm_amd.h (tgmx_tgat_attn_backward)
    probs = torch.where(c['no_valid'][:, None, None], -c['probs'], c['probs'])
    heads = lambda t: t.reshape(R * H, C)
    bQ, bZ = Buf(R * H, C, ld=Cs, data=heads(c['qf'])), Buf(R * H, C, ld=Cs, data=heads(c['dzbar']))  # (NaN between the heads: never read)
    dev = {n: c[n].to(DEV).contiguous() for n in ('nbrf', 'seed_t', 'nbr_t', 'tw', 'tb')}
    probs = probs.to(DEV).contiguous()
    ex_flat = torch.zeros(R * k * D + 8, device=DEV)
    ex = ex_flat[1:1 + R * k * D] if misalign_ex else ex_flat[: R * k * D]
    ex.copy_(c['ex'].reshape(-1))
    assert (ex.data_ptr() % 16 != 0) == misalign_ex
    desc = native.dropout_desc(DROP_P, DROP_SEED, DROP_STREAM, DROP_ROW0) if drop else None
    outs = []
    for _ in range(2):
        bDq, bDt = Buf(R * H, C, ld=Cs), Buf(R, 2 * T)
        bDn = Buf(R * k, d, fill=3.0, data=dn0.reshape(R * k, d)) if with_dnbr else None
        native.check(lib.tgmx_tgat_attn_backward(bQ.ptr, probs.data_ptr(), bZ.ptr, dev['nbrf'].data_ptr(), d, ex.data_ptr() if D else None, D,
                                                 dev['seed_t'].data_ptr(), dev['nbr_t'].data_ptr(), dev['tw'].data_ptr(), dev['tb'].data_ptr(), T, H, k, R,
                                                 c['scale'], Cs if strided else 0, bDq.ptr, bDn.ptr if with_dnbr else None, bDt.ptr, desc,
                                                 native.stream_ptr()), 'tgat_attn_backward')
        torch.cuda.synchronize()
        # (columns [C, head_stride) of dqf are unspecified: zeroed by the rows without upstream gradient, left alone by the others)
        assert _same_bits(bDq.flat[R * H * Cs:], torch.full((TAIL,), NAN, device=DEV)), 'dqf: a write past the last row'
        assert bDt.sentinels_intact(), 'dtime: a write past [R, 2T]'
        assert bDn is None or bDn.sentinels_intact(), 'dnbr: a write past [R, k, d]'
        outs.append((bDq.view.contiguous().clone(), bDn.view.clone() if with_dnbr else None, bDt.view.clone()))
    for a, b in zip(outs[0], outs[1]):
        assert a is None or _same_bits(a, b), 'two launches differ'
    dqf, dnbr, dtime = outs[0]
    return c, dn0, want, dqf.reshape(R, H, C), dnbr.reshape(R, k, d) if with_dnbr else None, dtime


def _check_attn(tag, shape, got, c, dn0, want, rows=None):
    H, k, d, D, T = shape
    dqf, dnbr, dtime = got
    sel = slice(None) if rows is None else rows
    worst = {}
    for name, g in (('dqf', dqf), ('dnbr', dnbr), ('dtime', dtime)):
        if g is None:
            continue
        n = ref.attn_chain(c['C'], H, k, name == 'dtime') * ref.EPS
        worst[name] = _report(f'attn_backward {tag} {name}', g[sel], want[name][sel], n * want[name + '_mag'][sel])
    return worst


# (misaligned (2,20,200,8,16): d = 200 in the LDS kernel as well -- a chunk loop whose last chunk ends on a multiple of 4)
ATTN_CONFIGS = [(s, False) for s in ref.ATTN_SHAPES] + [((2, 20, 172, 172, 100), True), ((2, 20, 200, 8, 16), True)]


@pytest.mark.parametrize('strided', [False, True], ids=['stride0', 'strideC+3'])
@pytest.mark.parametrize('with_dnbr', [False, True], ids=['dnbr_null', 'dnbr_randn'])
@pytest.mark.parametrize('drop', [False, True], ids=['p0', 'p0.1'])
@pytest.mark.parametrize('shape,misalign_ex', ATTN_CONFIGS, ids=lambda v: str(v).replace(' ', ''))
def test_attn_backward(shape, misalign_ex, drop, with_dnbr, strided):
    """(H, k, d, D, T) -> the route ATTN_ROUTES names, by the condition of launch_attn_backward quoted there.  misalign_ex: ``ex`` one
    float past a 16-byte boundary fails ``(bits & 15) == 0`` and the shape falls back to the LDS kernel, same bound.
    Rows (oracle.tgat_bwd_ref.attn_case): every count of valid slots 1 .. k left-padded (every span body), fully valid, an interior
    hole, all-zero dzbar (exact zeros, dnbr untouched), two rows without a valid slot (identical / differing slot features:
    ds = 0, the reference's masked_fill), two rows with dt ~ 2^30 (arguments past kCosSmallLimit = 8e6: the double reduction),
    a random mask."""
    assert shape in ATTN_ROUTES
    H, k, d, D, T = shape
    c, dn0, want, dqf, dnbr, dtime = _run_attn(shape, drop, with_dnbr, strided, misalign_ex)
    zero_row = k + 2
    assert torch.equal(dqf[zero_row].cpu(), torch.zeros(H, c['C'])) and torch.equal(dtime[zero_row].cpu(), torch.zeros(2 * T)), 'zero-dzbar row'
    if with_dnbr:
        assert _same_bits(dnbr[zero_row].cpu(), dn0[zero_row]), 'zero-dzbar row: dnbr touched'
    dt, arg = ref.time_args(c['seed_t'], c['nbr_t'], c['tw'], c['tb'])
    assert float(arg[k + 5:k + 7].abs().max()) > 8.0e6 and float(arg.abs().max()) < 2.1e9
    tag = f'{shape}{" misaligned" if misalign_ex else ""} p={DROP_P if drop else 0} dnbr={"randn" if with_dnbr else "NULL"} stride={"C+3" if strided else 0}'
    worst = _check_attn(tag, shape, (dqf, dnbr, dtime), c, dn0, want)
    assert max(worst.values()) <= 1.0, worst
    # rows without a valid slot: nothing flows through the scores
    nv = c['no_valid']
    assert torch.equal(dqf[nv].cpu(), torch.zeros(int(nv.sum()), H, c['C'])), 'all-pad rows: dqf must be exactly 0 (ds = 0)'


def test_attn_backward_rejects_more_than_64_slot_head_pairs():
    """k * H = 66: TGMX_REQUIRE refuses before any launch (a RuntimeError through _native.check); the outputs stay as they were."""
    lib, native = _lib()
    H, k, d, D, T, R = 2, 33, 2, 4, 3, 4
    C = d + D + T
    z = lambda *s: torch.zeros(*s, device=DEV)
    qf, probs, dz, nbrf, ex = z(R, H, C), torch.full((R, H, k), 1.0 / k, device=DEV), z(R, H, C), z(R, k, d), z(R, k, D)
    st, nt = torch.ones(R, dtype=torch.int64, device=DEV), torch.zeros(R, k, dtype=torch.int64, device=DEV)
    tw, tb = z(T), z(T)
    dqf, dtime = Buf(R * H, C), Buf(R, 2 * T)
    with pytest.raises(RuntimeError, match='k \\* n_heads <= 64'):
        native.check(lib.tgmx_tgat_attn_backward(qf.data_ptr(), probs.data_ptr(), dz.data_ptr(), nbrf.data_ptr(), d, ex.data_ptr(), D, st.data_ptr(),
                                                 nt.data_ptr(), tw.data_ptr(), tb.data_ptr(), T, H, k, R, 0.5, 0, dqf.ptr, None, dtime.ptr, None,
                                                 native.stream_ptr()), 'tgat_attn_backward')
    torch.cuda.synchronize()
    assert bool(torch.isnan(dqf.flat).all()) and bool(torch.isnan(dtime.flat).all()), 'a kernel ran'


# ---------------------------------------------------------------------------------------------------------------------------
# the saving forward on rows without a valid slot: the marker it leaves for the backward, and its one-slot shortcut under dropout
# ---------------------------------------------------------------------------------------------------------------------------
def test_attn_reduce_all_pad_rows_under_dropout_against_temporal_attention():
    """``tgmx_tgat_attn_reduce`` with attention dropout on rows without a valid slot, through the rest of the layer in float64,
    against ``oracle.tgat_ref.temporal_attention`` with the device's keep mask.  Row 0: the sampler's all-pad row (k identical
    slots: one slot read).  Row 1: an all-pad row of a layer above the leaves in train mode -- equal slot inputs, but k DIFFERENT
    rows of the layer below (each drew its own dropout masks): the uniform average over the k slots, not k times slot 0.  Rows 2, 3:
    fully valid, left-padded.  Bar: 1e-5 * max(1, |ref|), the forward parity bar of tests/test_tgat_gpu.py.  The saved weights of
    rows 0 and 1 are the uniform weights NEGATED (the backward's marker), those of the other rows the softmax."""
    from oracle import tgat_ref

    lib, native = _lib()
    H, k, d, D, T, O, B = 2, 5, 8, 4, 6, 16, 4
    C, dh = d + D + T, O // H
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g)
    p = {'W_Q.weight': rnd(O, O) * 0.3, 'W_KV.weight': rnd(2 * O, C) * 0.3, 'W_O.weight': rnd(O, O) * 0.3, 'W_O.bias': rnd(O) * 0.1,
         'layer_norm.weight': 1.0 + 0.1 * rnd(O), 'layer_norm.bias': 0.1 * rnd(O)}
    p = {n: v.double() for n, v in p.items()}
    node_x, tw, tb = rnd(B, d), (1.0 / 10 ** torch.linspace(0, 4, T, dtype=torch.float64)).float(), rnd(T) * 0.1
    nid = torch.randint(0, 50, (B, k), generator=g, dtype=torch.int32)
    nid[0] = nid[1] = -1
    nid[3, :3] = -1
    mask = nid != -1
    nbrf, ex = rnd(B, k, d), torch.rand(B, k, D, generator=g)
    nbrf[0] = nbrf[0, 0]
    ex[~mask] = 0.0
    seed_t = torch.randint(1000, 5000, (B,), generator=g)
    nbr_t = seed_t[:, None] - torch.randint(1, 900, (B, k), generator=g)
    nbr_t[~mask] = 0
    _, arg = ref.time_args(seed_t, nbr_t, tw, tb)
    nbr_time = torch.cos(arg.double())
    time_feat = torch.cos(tb.double()).expand(B, T)
    # the folded query of csrc/tgat.hip: qf[b, h] = Q[b, head h] @ W_K[head h rows]
    R_in = torch.cat([torch.nn.functional.pad(node_x.double(), (0, O - d - T)), time_feat], 1)
    Q = (R_in @ p['W_Q.weight'].T).view(B, H, dh)
    WK, WV = p['W_KV.weight'][:O].view(H, dh, C), p['W_KV.weight'][O:].view(H, dh, C)
    qf = torch.einsum('bhd,hdc->bhc', Q, WK).float().contiguous().to(DEV)
    ones, keep_dev = torch.ones(B, H * k, device=DEV), torch.full((B, H * k), NAN, device=DEV)
    desc = native.dropout_desc(0.25, DROP_SEED, DROP_STREAM, 0)
    native.check(lib.tgmx_dropout(ones.data_ptr(), H * k, B, H * k, desc, keep_dev.data_ptr(), H * k, native.stream_ptr()), 'dropout')
    keep = keep_dev.cpu().view(B, H, k)
    assert 0 < int((keep[:2] == 0).sum()) < 2 * H * k, 'the all-pad rows need kept and dropped slots'
    dev = [t.contiguous().to(DEV) for t in (nbrf, ex, seed_t, nbr_t, nid, tw, tb)]
    zbar, probs = Buf(B * H, C), Buf(B * H, k)
    native.check(lib.tgmx_tgat_attn_reduce(qf.data_ptr(), dev[0].data_ptr(), d, dev[1].data_ptr(), D, dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(),
                                           dev[5].data_ptr(), dev[6].data_ptr(), 0, 0, T, H, k, B, dh ** -0.5, 0, zbar.ptr, probs.ptr, desc,
                                           native.stream_ptr()), 'attn_reduce')
    torch.cuda.synchronize()
    assert zbar.sentinels_intact() and probs.sentinels_intact()
    A = probs.view.cpu().view(B, H, k)
    assert torch.equal(A[:2], torch.full((2, H, k), -1.0 / k)), 'rows without a valid slot: the weights are saved negated'
    assert bool((A[2:] >= 0).all()) and float((A[2:].sum(-1) - 1).abs().max()) < 1e-6 and bool((A[3, :, :3] == 0).all())
    oattn = torch.einsum('bhc,hdc->bhd', zbar.view.cpu().double().view(B, H, C), WV).reshape(B, O)
    got = torch.nn.functional.layer_norm(oattn @ p['W_O.weight'].T + p['W_O.bias'] + R_in, (O,), p['layer_norm.weight'], p['layer_norm.bias'], 1e-5)
    want = tgat_ref.temporal_attention(p, '', H, node_x.double(), time_feat, ex.double(), nbrf.double(), nbr_time, mask,
                                       drop=(keep.double(), torch.ones(B, O, dtype=torch.float64)))
    for r in range(B):
        worst = float(((got[r] - want[r]).abs() / (1e-5 * want[r].abs().clamp(min=1.0))).max())
        print(f'[blocks] attn_reduce under dropout, row {r}: {worst:.4f}x the 1e-5 bound')
        assert worst <= 1.0, f'row {r}: {worst:.3g}x the bound'
