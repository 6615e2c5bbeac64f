"""The DyGFormer inference kernels one by one against the float64 restatements of ``oracle/fwd_blocks_ref.py`` (which
``tests/test_fwd_blocks_ref_cpu.py`` pins to torch and to ``tests/dygformer_restate.py``), through ctypes: ``tgmx_layernorm_rows``
(``csrc/dense.hip``), ``tgmx_mha_small``, ``tgmx_dygformer_prologue`` and ``tgmx_dygformer_tail`` (``csrc/dygformer.hip``).  The
conventions are those of ``tests/test_tgn_bwd_blocks_gpu.py`` (the helpers of ``tests/test_tgat_bwd_blocks_gpu.py`` are imported):

* outputs are pre-filled with NaN and followed by a sentinel tail of 4096 floats; where a kernel leaves the columns past the width
  alone (``ldy = d + 3``, ``ldo = H dh + 4``) those are sentinels too, and the inputs' padding columns hold NaN;
* every case is launched twice and the bits must be equal (none of these kernels has atomics);
* bars: elementwise ``n * 2^-24 * magnitude`` with n counted from the kernel code (``wave_ln_chain``, ``mha_chain``, ``time_chain``,
  ``dyg_mean_chain``), ``gemm_bar(D)`` for the output GEMM of the tail, nothing tuned on the device's result; gathered features and
  structural zeros are exact.  ``pytest -rP`` prints the worst err / bound per case.

Measured on an MI355X, worst err / bound over the cases of each kernel: layernorm_rows 0.046 (at (5, 64)); mha_small 0.027 (at
(2, 17, 3, 5), the row of equal scores); dygformer_prologue's time channel 0.080 (at the workload's widths with row indices; node and edge
channels bit for bit); dygformer_tail mean 0.500 (at (5, 3, 63, 7): n = 4 leaves a single rounding of 3 adds and a division little room),
out 0.014 of gemm_bar(D) (at (5, 3, 200, 7)).  What the bounds still catch is listed in ``oracle.fwd_blocks_ref.MUTATIONS``.  No bound
was exceeded and no kernel was changed.
"""
import functools

import pytest
import torch

from oracle import fwd_blocks_ref as ref
from oracle.tgat_bwd_ref import EPS
from test_tgat_bwd_blocks_gpu import DEV, Buf, _lib, _report, _same_bits

pytestmark = pytest.mark.gpu

ln_rows_case = functools.lru_cache(maxsize=None)(ref.ln_rows_case)
mha_case = functools.lru_cache(maxsize=None)(ref.mha_case)
dyg_prologue_case = functools.lru_cache(maxsize=None)(ref.dyg_prologue_case)
dyg_tail_case = functools.lru_cache(maxsize=None)(ref.dyg_tail_case)
ln_rows_bounds = functools.lru_cache(maxsize=None)(lambda *a: ref.ln_rows_bounds(ln_rows_case(*a)))
mha_bounds = functools.lru_cache(maxsize=None)(lambda *a: ref.mha_bounds(mha_case(*a)))
dyg_prologue_want = functools.lru_cache(maxsize=None)(lambda *a: ref.dyg_prologue_run(dyg_prologue_case(*a)))
dyg_tail_bounds = functools.lru_cache(maxsize=None)(lambda *a: ref.dyg_tail_bounds(dyg_tail_case(*a)))


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


def _untouched(*bufs):
    return all(bool(torch.isnan(b.flat).all()) for b in bufs)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_layernorm_rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R,d', ref.LN_ROWS_CASES)
def test_layernorm_rows(R, d):
    """(R, d).  One wave per row, four rows per block: R = 1, 2, 5, 37 (ragged last blocks).  d = 1 (variance 0: beta), 63, 64, 65, 200,
    512: one lane short of a trip, a full trip, one lane into the second, eight trips.  ldx = d + 1 (NaN in the padding), ldy = d + 3
    (sentinels).  Rows (oracle.fwd_blocks_ref.ln_rows_case): constant (exactly beta in float64; the kernel's plain mean may be off
    by rstd d 2^-24 |x|, and the bound says so), offset 1e4 with spread 1, spread 0.01, randn."""
    lib, native = _lib()
    c = ln_rows_case(R, d)
    want, bound = ln_rows_bounds(R, d)
    x = Buf(R, d, ld=d + 1, data=c['x'].to(DEV))
    g, b = _dev(c['g']), _dev(c['b'])
    outs = []
    for _ in range(2):
        y = Buf(R, d, ld=d + 3)
        native.check(lib.tgmx_layernorm_rows(x.ptr, x.ld, R, d, g.data_ptr(), b.data_ptr(), ref.LN_EPS, y.ptr, y.ld, native.stream_ptr()), 'layernorm_rows')
        torch.cuda.synchronize()
        assert y.sentinels_intact(), 'a write past a row\'s d columns or past the last row'
        outs.append(y.view.clone())
    assert _same_bits(outs[0], outs[1]), 'two launches differ'
    got = outs[0].cpu()
    if d == 1:
        assert _same_bits(got, c['b'].expand(R, 1)), 'd = 1: the mean of one value is that value, the row is beta'
    assert _report(f'layernorm_rows {(R, d)}', got, want, bound) <= 1.0


def test_layernorm_rows_no_rows():
    lib, native = _lib()
    y = Buf(0, 8)
    native.check(lib.tgmx_layernorm_rows(None, 8, 0, 8, None, None, ref.LN_EPS, y.ptr, 8, native.stream_ptr()), 'layernorm_rows R = 0')
    torch.cuda.synchronize()
    assert _untouched(y)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_mha_small
# ---------------------------------------------------------------------------------------------------------------------------
def _mha_call(c, qkv, out):
    lib, native = _lib()
    rc = lib.tgmx_mha_small(qkv.ptr, qkv.ld, c['B'], c['T'], c['H'], c['dh'], out.ptr, out.ld, native.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('B,T,H,dh', ref.MHA_CASES)
def test_mha_small(B, T, H, dh):
    """(B, T, H, dh).  (1,1,1,1): one token, the weight is 1.  T = 15, 16, 17: both sides of a 16-row score tile (the pad columns of the
    last tile must not reach the softmax).  H = 2, 3: the head's column offset.  dh = 3, 5, 33, 100: head dimensions that are no
    multiple of 4 / 16.  (3,64,2,32): four row tiles, one per wave.  (2,65,1,128): a fifth row tile, past 64 KiB of LDS.
    (2,100,2,100), (1,128,3,33): seven and eight score tiles.  (2,128,1,128): the whole envelope, 135 168 bytes of LDS.  ldq = 3 H dh + 4
    (NaN in the padding), ldo = H dh + 4 (sentinels).  Rows (oracle.fwd_blocks_ref.mha_case): a zero query (all scores equal: the
    weights are 1 / T), a query with one key at a score of 200 (the other weights underflow)."""
    _, native = _lib()
    c = mha_case(B, T, H, dh)
    want, bound = mha_bounds(B, T, H, dh)
    D = H * dh
    qkv = Buf(B * T, 3 * D, ld=3 * D + 4, data=c['qkv'].reshape(B * T, 3 * D).to(DEV))
    outs = []
    for _ in range(2):
        out = Buf(B * T, D, ld=D + 4)
        native.check(_mha_call(c, qkv, out), 'mha_small')
        assert out.sentinels_intact(), 'a write past a row\'s H dh columns or past the last row'
        outs.append(out.view.clone())
    assert _same_bits(outs[0], outs[1]), 'two launches differ'
    got = outs[0].cpu().reshape(B, T, D)
    assert _report(f'mha_small {(B, T, H, dh)}', got, want, bound) <= 1.0
    if T >= 2:  # the zero query: the mean of the values, to within the bound of an exact 1 / T
        mean_v = c['qkv'][0, :, 2 * D:].double().mean(0)
        assert _report(f'mha_small {(B, T, H, dh)} equal scores', got[0, 1], mean_v, bound[0, 1]) <= 1.0


def test_mha_small_no_sequences():
    lib, native = _lib()
    out = Buf(0, 8)
    native.check(lib.tgmx_mha_small(None, 24, 0, 4, 2, 4, out.ptr, 8, native.stream_ptr()), 'mha_small B = 0')
    torch.cuda.synchronize()
    assert _untouched(out)


@pytest.mark.parametrize('B,T,H,dh', ref.MHA_UNSUPPORTED_CASES)
def test_mha_small_outside_the_envelope(B, T, H, dh):
    """T = 129 and dh = 129: TGMX_E_UNSUPPORTED, nothing launched, the output untouched, a message in tgmx_last_error."""
    lib, native = _lib()
    D = H * dh
    qkv = Buf(B * T, 3 * D, ld=3 * D + 4, data=torch.randn(B * T, 3 * D))
    out = Buf(B * T, D, ld=D + 4)
    assert _mha_call(dict(B=B, T=T, H=H, dh=dh), qkv, out) == native.E_UNSUPPORTED
    assert _untouched(out)
    msg = lib.tgmx_last_error()
    assert msg and b'envelope' in msg, msg


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_dygformer_prologue
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P,k,widths,rows_given', ref.DYG_PROLOGUE_CASES + [ref.DYG_PROLOGUE_BIG_CASE], ids=str)
def test_dygformer_prologue(P, k, widths, rows_given):
    """(P, k, (dN, dE, dT, ldn, lde, ldt), rows given).  Widths (1,1,1,4,4,4): padded columns in every channel; (6,5,8,8,8,8); the
    workload's (128,172,100).  src_rows / dst_rows NULL (rows p and P + p of S = 2 P) and given (S = 5; a row index of -1 and one of S
    make the whole sequence pads: only the seed's slot 0 carries anything).  Slot ids of -1: zeros in the node and the time channel
    (no time encoding), the edge channel still copies the slot's features.  Slot ids >= num_nodes: zero node features, the time
    encoding still computed.  k = 0 with NULL neighbour pointers.  (87384, 1, 4+4+4): 2 P L W is 128 past 16384 blocks x 256.
    Unix-scale times: gaps of 1, 0, 2^24 + 1, 2^31 - 1.  The kernel writes every column up to ldn / lde / ldt; node and edge are exact."""
    lib, native = _lib()
    c = dyg_prologue_case(P, k, widths, rows_given)
    node_w, edge_w, time_w, tmag = dyg_prologue_want(P, k, widths, rows_given)
    dN, dE, dT, ldn, lde, ldt = widths
    R = 2 * P * (k + 1)
    d = {n: _dev(c[n]) for n in ('node_x', 'src', 'dst', 'edge_time', 'nids', 'nbr_t', 'nbr_x', 'src_rows', 'dst_rows', 'tw', 'tb')}
    if k:
        assert d['nids'].dtype == torch.int32 and d['nbr_t'].dtype == torch.int64 and tuple(d['nbr_x'].shape) == (c['S'], k, dE)
    outs = []
    for _ in range(2):
        bn, be, bt = Buf(R, ldn), Buf(R, lde), Buf(R, ldt)
        native.check(lib.tgmx_dygformer_prologue(d['node_x'].data_ptr(), c['N'], dN, d['src'].data_ptr(), d['dst'].data_ptr(), d['edge_time'].data_ptr(), P,
                                                 _p(d['nids']), _p(d['nbr_t']), _p(d['nbr_x']), c['S'], k, dE, _p(d['src_rows']), _p(d['dst_rows']),
                                                 d['tw'].data_ptr(), d['tb'].data_ptr(), dT, bn.ptr, ldn, be.ptr, lde, bt.ptr, ldt, native.stream_ptr()),
                     'dygformer_prologue')
        torch.cuda.synchronize()
        assert bn.sentinels_intact() and be.sentinels_intact() and bt.sentinels_intact(), 'a write past the last row'
        outs.append((bn.view.clone(), be.view.clone(), bt.view.clone()))
    assert all(_same_bits(a, b) for a, b in zip(*outs)), 'two launches differ'
    node, edge, time = (t.cpu() for t in outs[0])
    assert torch.equal(node.double(), node_w), 'node channel: gathered rows, zeros for pads, ids out of range and padded columns'
    assert torch.equal(edge.double(), edge_w), 'edge channel: the sampler\'s rows, zeros for slot 0, pad sequences and padded columns'
    assert torch.equal(time[tmag == 0], torch.zeros(int((tmag == 0).sum()))), 'time channel: exact zeros for id == -1 and padded columns'
    assert _report(f'dygformer_prologue {(P, k, widths, rows_given)} time', time, time_w, ref.time_chain() * EPS * tmag) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_dygformer_tail
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P,Np,D,E', ref.DYG_TAIL_CASES)
def test_dygformer_tail(P, Np, D, E):
    """(P, Np, D, E).  Np = 1, 3, 32 tokens per side; D = 1, 63, 64, 65 (the 64-thread block), 200, 257 (a second trip of the 256-thread
    stride); E = 1, 7, 172; P = 1, 5 (mean row side P + p: sources first).  ldx = D + 3 (NaN in the padding), ldm = D + 5: the kernel
    zeroes [D, ldm).  mean within (Np + 1) 2^-24 sum|x| / Np; out within gemm_bar(D) of the float64 product of the float64 mean."""
    lib, native = _lib()
    c = dyg_tail_case(P, Np, D, E)
    (mean_w, out_w), (bm, bo) = dyg_tail_bounds(P, Np, D, E)
    x = Buf(2 * P * Np, D, ld=c['ldx'], data=c['x'].to(DEV))
    w, b = _dev(c['out_w']), _dev(c['out_b'])
    outs = []
    for _ in range(2):
        mean, out = Buf(2 * P, c['ldm']), Buf(2 * P, E)
        native.check(lib.tgmx_dygformer_tail(x.ptr, x.ld, P, Np, D, mean.ptr, c['ldm'], w.data_ptr(), b.data_ptr(), E, out.ptr, native.stream_ptr()),
                     'dygformer_tail')
        torch.cuda.synchronize()
        assert mean.sentinels_intact() and out.sentinels_intact(), 'a write past [2 P, ldm] or [2 P, E]'
        outs.append((mean.view.clone(), out.view.clone()))
    assert _same_bits(outs[0][0], outs[1][0]) and _same_bits(outs[0][1], outs[1][1]), 'two launches differ'
    mean, out = (t.cpu() for t in outs[0])
    assert torch.equal(mean[:, D:], torch.zeros(2 * P, c['ldm'] - D)), 'columns [D, ldm) of mean must be exactly 0'
    assert _report(f'dygformer_tail {(P, Np, D, E)} mean', mean, mean_w, bm) <= 1.0
    assert _report(f'dygformer_tail {(P, Np, D, E)} out', out, out_w, bo) <= 1.0


def test_dygformer_tail_no_pairs():
    lib, native = _lib()
    mean, out = Buf(0, 8), Buf(0, 4)
    native.check(lib.tgmx_dygformer_tail(None, 8, 0, 2, 8, mean.ptr, 8, None, None, 4, out.ptr, native.stream_ptr()), 'dygformer_tail P = 0')
    torch.cuda.synchronize()
    assert _untouched(mean, out)
