"""The GraphMixer inference kernels of ``csrc/mixer.hip`` one by one against the float64 restatements of ``oracle/fwd_blocks_ref.py``
(which ``tests/test_fwd_blocks_ref_cpu.py`` pins to torch and to ``tests/graphmixer_restate.py``), through ctypes:
``tgmx_mixer_prologue``, ``tgmx_mixer_token`` and its TPNet twin ``tgmx_tpnet_token_mix``, ``tgmx_mixer_tail``.  The conventions are those
of ``tests/test_tgn_bwd_blocks_gpu.py`` (the helpers of ``tests/test_tgat_bwd_blocks_gpu.py`` are imported):

* outputs are pre-filled with NaN and followed by a sentinel tail of 4096 floats; where a kernel leaves the columns past the width
  alone (token: ``ldo = C + 5``) those are sentinels too, and the inputs' padding columns (``ldx = C + 3``, ``ldz = C + 3``) hold NaN;
* every case is launched twice and the bits must be equal (none of these kernels has atomics);
* bars: elementwise ``n * 2^-24 * magnitude`` with n counted from the kernel code (``time_chain``, ``token_chain``, ``wave_ln_chain``,
  ``tail_chains``), nothing tuned on the device's result; gathered features and structural zeros are exact.  ``pytest -rP`` prints the
  worst err / bound per case.

Measured on an MI355X, worst err / bound over the cases of each kernel: mixer_prologue 0.085 (at (7, 20, 172, 100, 272); the unix-scale
arguments of cosf included); mixer_token z1 0.026 (at (1, 2, 63, 1)), y 0.020 (at (3, 5, 65, 2)), its constant columns 0.016 of the plain
bound ``rstd K 2^-24 |x|``; tpnet_token_mix z1 0.029 (at (1, 1, 65, 1)), y 0.017, its constant columns 0.029 of the tighter bound without
the ``1 / sqrt(eps)`` term; mixer_tail 0.166 (at (256, 65, 0, (3, 2))).  The token bound is a worst case over a chain of 3 K + Ht + 28
operations through two LayerNorms' first-order sensitivities; the device's error is a random walk far below it.  What the bounds still
catch is listed in ``oracle.fwd_blocks_ref.MUTATIONS``.  No bound was exceeded and no kernel was changed.
"""
import functools

import pytest
import torch

from oracle import fwd_blocks_ref as ref
from test_tgat_bwd_blocks_gpu import DEV, Buf, _lib, _report, _same_bits

pytestmark = pytest.mark.gpu

prologue_case = functools.lru_cache(maxsize=None)(ref.prologue_case)
token_case = functools.lru_cache(maxsize=None)(ref.token_case)
tail_case = functools.lru_cache(maxsize=None)(ref.tail_case)
prologue_bounds = functools.lru_cache(maxsize=None)(lambda *a: ref.prologue_bounds(prologue_case(*a)))
token_bounds = functools.lru_cache(maxsize=None)(lambda refine, *a: ref.token_bounds(token_case(*a), refine))
tail_bounds = functools.lru_cache(maxsize=None)(lambda *a: ref.tail_bounds(tail_case(*a)))


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


def _untouched(*bufs):
    return all(bool(torch.isnan(b.flat).all()) for b in bufs)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_mixer_prologue
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,K,D,T,ldo', ref.PROLOGUE_CASES + [ref.PROLOGUE_BIG_CASE])
def test_mixer_prologue(S, K, D, T, ldo):
    """(S, K, D, T, ldo).  (1,1,0,1,1): one thread, edge_x = NULL.  (3,5,13,7,20), (2,3,4,5,16): a ragged block, padded columns.
    (7,20,172,100,272): the workload's widths, several blocks.  (65539,4,3,5,8): S K ldo is 96 past 8192 blocks x 256 -- the block cap
    holds and the grid stride takes a second trip for exactly the tail.  seed_t is unix-scale int64 (subtract in int64, THEN round:
    float first is off by up to 128); the gaps are 1, 0, 2^24 + 1, 2^31 - 1, a pad slot with nbr_t = 0 (the gap is the seed time: cosf
    at 1.7e9), the rest within 40.  The kernel writes every column up to ldo: the edge columns bit for bit, [D + T, ldo) exactly 0."""
    lib, native = _lib()
    c = prologue_case(S, K, D, T, ldo)
    want, bound = prologue_bounds(S, K, D, T, ldo)
    ex, st, nt, tw, tb = (_dev(c[n]) for n in ('edge_x', 'seed_t', 'nbr_t', 'tw', 'tb'))
    outs = []
    for _ in range(2):
        out = Buf(S * K, ldo)
        native.check(lib.tgmx_mixer_prologue(_p(ex), st.data_ptr(), nt.data_ptr(), S, K, D, tw.data_ptr(), tb.data_ptr(), T, out.ptr, ldo,
                                             native.stream_ptr()), 'mixer_prologue')
        torch.cuda.synchronize()
        assert out.sentinels_intact(), 'a write past [S K, ldo]'
        outs.append(out.view.clone())
    assert _same_bits(outs[0], outs[1]), 'two launches differ'
    got = outs[0].cpu()
    if D:
        assert _same_bits(got[:, :D], c['edge_x']), 'the edge columns are copies'
    assert torch.equal(got[:, D + T:], torch.zeros(S * K, ldo - D - T)), 'columns [D + T, ldo) must be exactly 0'
    assert _report(f'mixer_prologue {(S, K, D, T, ldo)}', got, want, bound) <= 1.0


def test_mixer_prologue_no_seeds():
    lib, native = _lib()
    out = Buf(0, 8)
    native.check(lib.tgmx_mixer_prologue(None, None, None, 0, 4, 3, None, None, 5, out.ptr, 8, native.stream_ptr()), 'mixer_prologue S = 0')
    torch.cuda.synchronize()
    assert _untouched(out)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_mixer_token, tgmx_tpnet_token_mix
# ---------------------------------------------------------------------------------------------------------------------------
def _token_call(entry, c, x, z1, y):
    lib, native = _lib()
    w = {n: _dev(c[n]) for n in ('tg', 'tbeta', 'w1', 'b1', 'w2', 'b2', 'cg', 'cb')}
    rc = getattr(lib, entry)(x.ptr, x.ld, c['S'], c['K'], c['C'], w['tg'].data_ptr(), w['tbeta'].data_ptr(), _p(w['w1']), _p(w['b1']), c['Ht'],
                             _p(w['w2']), w['b2'].data_ptr(), w['cg'].data_ptr(), w['cb'].data_ptr(), ref.LN_EPS, z1.ptr, y.ptr, z1.ld,
                             native.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('entry', ['tgmx_mixer_token', 'tgmx_tpnet_token_mix'])
@pytest.mark.parametrize('S,K,C,Ht', ref.TOKEN_CASES)
def test_mixer_token(S, K, C, Ht, entry):
    """(S, K, C, Ht).  C = 1, 63, 65, 127, 128, 129, 257, 627: one lane, both sides of a 64-lane trip of pass 2, both sides of the
    kTokThreads = 128 chunk of pass 1, a third chunk, and 16 380 of the 16 384 floats of LDS.  K = 1 (variance 0: LayerNorm gives
    beta), 2, 5, 20, 30: odd and even over the two waves of pass 2.  Ht = 0 (w1 = NULL), 1, K / 2, 39 at K = 30.  ldx = C + 3 (NaN
    in the padding), ldo = C + 5 (sentinels).  The last seed's special columns (oracle.fwd_blocks_ref.token_case): K equal awkward
    values, offset 1e4 with spread 1, spread 0.01.  Both entry points on every case; tgmx_tpnet_token_mix (kRefine) meets the
    tighter bound on the constant columns: no 1 / sqrt(eps) term, the normalised column is exactly tbeta."""
    _, native = _lib()
    c = token_case(S, K, C, Ht)
    refine = entry == 'tgmx_tpnet_token_mix'
    (z1w, yw), (bz1, by) = token_bounds(refine, S, K, C, Ht)
    x = Buf(S * K, C, ld=C + 3, data=c['x'].reshape(S * K, C).to(DEV))
    outs = []
    for _ in range(2):
        z1, y = Buf(S * K, C, ld=C + 5), Buf(S * K, C, ld=C + 5)
        native.check(_token_call(entry, c, x, z1, y), entry)
        assert z1.sentinels_intact() and y.sentinels_intact(), 'a write past a row\'s C columns or past the last row'
        outs.append((z1.view.clone(), y.view.clone()))
    assert _same_bits(outs[0][0], outs[1][0]) and _same_bits(outs[0][1], outs[1][1]), 'two launches differ'
    z1g, yg = (t.cpu().reshape(S, K, C) for t in outs[0])
    tag = f'{entry[5:]} {(S, K, C, Ht)}'
    assert _report(f'{tag} z1', z1g, z1w, bz1) <= 1.0
    assert _report(f'{tag} y', yg, yw, by) <= 1.0
    const = c['const_cols']
    if bool(const.any()):  # the constant columns alone: the plain kernel within rstd K 2^-24 |x|, the refined one within the tight bound
        assert _report(f'{tag} z1, constant columns', z1g[S - 1][:, const], z1w[S - 1][:, const], bz1[S - 1][:, const]) <= 1.0


@pytest.mark.parametrize('entry', ['tgmx_mixer_token', 'tgmx_tpnet_token_mix'])
def test_mixer_token_outside_the_lds_envelope(entry):
    """(2, 20, 628, 10) needs 4 * (20 * 628 + 30 * 128) = 65 600 bytes of LDS: TGMX_E_UNSUPPORTED, nothing launched, z1 / y untouched, a
    message in tgmx_last_error.  (2, 20, 627, 10), 16 380 floats, runs: test_mixer_token."""
    lib, native = _lib()
    S, K, C, Ht = ref.TOKEN_UNSUPPORTED_CASE
    assert 4 * ref.token_lds_floats(K, C, Ht) > 65536 >= 4 * ref.token_lds_floats(K, C - 1, Ht)
    c = token_case(S, K, C, Ht)
    x = Buf(S * K, C, ld=C + 3, data=c['x'].reshape(S * K, C).to(DEV))
    z1, y = Buf(S * K, C, ld=C + 5), Buf(S * K, C, ld=C + 5)
    assert _token_call(entry, c, x, z1, y) == native.E_UNSUPPORTED
    assert _untouched(z1, y)
    msg = lib.tgmx_last_error()
    assert msg and b'LDS' in msg and b'628' in msg, msg


def test_mixer_token_no_seeds():
    lib, native = _lib()
    z1, y = Buf(0, 8), Buf(0, 8)
    native.check(lib.tgmx_mixer_token(None, 8, 0, 4, 8, None, None, None, None, 2, None, None, None, None, ref.LN_EPS, z1.ptr, y.ptr, 8,
                                      native.stream_ptr()), 'mixer_token S = 0')
    torch.cuda.synchronize()
    assert _untouched(z1, y)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_mixer_tail
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,F,pad,split', ref.TAIL_CASES)
def test_mixer_tail(C, F, pad, split):
    """(C, F, ldo - C - F, (n0, n1)).  C = 1, 255, 256, 257: the 256-thread stride over the link mean's columns.  F = 1, 64, 65, 100: the
    64-lane chunks of the node part.  S = 9 seeds, K = 5 slots with 0, 1, 5, 3, 2, 5, 0, 4, 1 valid ones; a pad slot's z row holds 1e30 and
    must not reach the mean (ldz = C + 3, NaN in the padding).  tg_cnt = 0, 1, 3, 4, 5, 300, 1000, 2, 7 over kTailWaves = 4.  The seeds
    come as (S, 0, 0), (0, 0, S), (0, S, 0) and three-way splits.  Exact: a seed without a valid slot has a link mean of 0; cnt == 0
    leaves the seed's own node row, bit for bit; the tail columns [C + F, ldo) are 0."""
    lib, native = _lib()
    c = tail_case(C, F, pad, split)
    want, bound = tail_bounds(C, F, pad, split)
    S, K, ldo = c['S'], c['K'], c['ldo']
    n0, n1 = split
    z = Buf(S * K, C, ld=C + 3, data=c['z'].reshape(S * K, C).to(DEV))
    d = {n: _dev(c[n]) for n in ('nids', 'node_x', 'tg_nbr', 'tg_lo', 'tg_cnt')}
    groups = [_dev(g) if g.numel() else None for g in (c['seeds'][:n0], c['seeds'][n0:n0 + n1], c['seeds'][n0 + n1:])]
    assert all(d[n].dtype == torch.int32 for n in ('nids', 'tg_nbr', 'tg_lo', 'tg_cnt')) and c['seeds'].dtype == torch.int32
    assert int(c['tg_nbr'].max()) < ref.TAIL_NODES and int((c['tg_lo'] + c['tg_cnt']).max()) <= c['tg_nbr'].numel()
    outs = []
    for _ in range(2):
        out = Buf(S, ldo)
        native.check(lib.tgmx_mixer_tail(z.ptr, z.ld, S, K, C, d['nids'].data_ptr(), d['node_x'].data_ptr(), ref.TAIL_NODES, F, d['tg_nbr'].data_ptr(),
                                         d['tg_lo'].data_ptr(), d['tg_cnt'].data_ptr(), _p(groups[0]), n0, _p(groups[1]), n1, _p(groups[2]), out.ptr, ldo,
                                         native.stream_ptr()), 'mixer_tail')
        torch.cuda.synchronize()
        assert out.sentinels_intact(), 'a write past [S, ldo]'
        outs.append(out.view.clone())
    assert _same_bits(outs[0], outs[1]), 'two launches differ'
    got = outs[0].cpu()
    no_slot = torch.tensor(ref.TAIL_VALID) == 0
    assert int(no_slot.sum()) == 2 and torch.equal(got[no_slot, :C], torch.zeros(2, C)), 'no valid slot: the link mean is exactly 0'
    empty = c['tg_cnt'] == 0
    assert _same_bits(got[empty, C:C + F], c['node_x'][c['seeds'][empty].long()]), 'cnt == 0: the seed\'s own row, bit for bit'
    assert torch.equal(got[:, C + F:], torch.zeros(S, pad)), 'columns [C + F, ldo) must be exactly 0'
    assert _report(f'mixer_tail {(C, F, pad, split)}', got, want, bound) <= 1.0


def test_mixer_tail_no_seeds():
    lib, native = _lib()
    out = Buf(0, 8)
    native.check(lib.tgmx_mixer_tail(None, 4, 0, 5, 4, None, None, 10, 3, None, None, None, None, 0, None, 0, None, out.ptr, 8, native.stream_ptr()),
                 'mixer_tail S = 0')
    torch.cuda.synchronize()
    assert _untouched(out)
