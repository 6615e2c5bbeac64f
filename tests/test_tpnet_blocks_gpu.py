"""The kernels of ``csrc/tpnet.hip`` one by one against the float64 restatements of ``oracle/tpnet_fwd_ref.py`` (which
``tests/test_tpnet_fwd_ref_cpu.py`` pins to ``tests/tpnet_restate.py`` and the reference fixtures), through ctypes: ``tgmx_tpnet_update``
(``tpnet_stage_kernel`` + ``tpnet_apply_kernel``), ``tgmx_tpnet_pair_features`` (the 16 instances of ``tpnet_pair_kernel``),
``tgmx_tpnet_tokens``, ``tgmx_tpnet_mean``, and ``tgmx_tpnet_forward`` / ``tgmx_tpnet_forward_train`` bit for bit against those parts.
The conventions are those of ``tests/test_tgn_fwd_blocks_gpu.py`` (helpers from ``tests/test_tgat_bwd_blocks_gpu.py``):

* outputs sit in NaN-filled ``Buf``s followed by a sentinel tail of 4096 floats that must be unchanged (integer outputs: a tail of
  sentinel words); the tables of ``update`` are such buffers too;
* every case is launched twice and must give equal bits (``csrc/tpnet.hip`` adds no floats atomically);
* copies are bit-exact (level 0 of the tables, a row nobody names when the decay is exactly 1, the node / edge / pair columns of the
  token matrix, ``mean`` at k = 1), structural zeros are exact, the integer cases of ``update`` are exact, a concatenated Gram matrix
  is bit-symmetric, a pad id gives the bits of id N - 1;
* everything else: elementwise ``(n + 8) * 2^-24 * magnitude`` with n counted from the kernel code (``update_chain``, ``gram_chain``,
  ``mean_chain``), plus ``4 * 2^-24 |log1p|`` under scaling, and one rounding of a double result for the time columns; nothing tuned
  on the device's result.  ``pytest -rP`` prints the worst err / bound per case.

Measured on an MI355X, worst err / bound over the cases of each kernel: update 0.279 (level 4 of (40, 30, 64, 7, 'times_equal'); the
hub case (100, 50, 130, 2) 0.170, the float-``now`` cases 0.161 and 0.109); pair features 0.181 (NL = 4 concat, dim 64, tables one float
into their allocations, raw; the 65 539-item case 0.117); mean 0.112 at (3, 7, 5); the time columns of the token matrix 0.993 (the
65 552-row case: the bound IS the half-ulp rounding of the double result, and some element among a hundred thousand comes close to a
tie); ``lg`` within its 4 * 2^-53 everywhere; ``tgmx_tpnet_forward``'s ``out`` 5.6e-8 ... 7.4e-7 from the float64 encoder (bar 1e-4).
Every bit-for-bit assertion held, no sentinel was disturbed, the integer cases (the 65 539-row one included) were exact; no kernel
change was needed.
"""
import ctypes
import functools

import pytest
import torch

import tpnet_restate as tr
from oracle import tpnet_fwd_ref as ref
from oracle.tgat_bwd_ref import EPS
from test_tgat_bwd_blocks_gpu import DEV, Buf, _lib, _report, _same_bits
from test_tgn_fwd_blocks_gpu import ISENT, IBuf, _dev, _ptr, _untouched

pytestmark = pytest.mark.gpu

update_case = functools.lru_cache(maxsize=None)(ref.update_case)
update_bounds = functools.lru_cache(maxsize=None)(lambda case: ref.update_bounds(update_case(*case)))
pair_case = functools.lru_cache(maxsize=None)(lambda case, items=None: ref.pair_case(*case, items=items))
token_case = functools.lru_cache(maxsize=None)(ref.token_case)
mean_case = functools.lru_cache(maxsize=None)(ref.mean_case)
E_INVALID, E_UNSUPPORTED = -1, -3


def _bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tpnet_update
# ---------------------------------------------------------------------------------------------------------------------------
class UpdateRun:
    """One tgmx_tpnet_update over the case's tables, every buffer guarded: the tables and msg are Bufs (NaN tails), head and now_out
    IBufs.  ``levels`` / ``dim`` / ``n`` / ``null_table`` override what the call is TOLD (the buffers keep the case's sizes)."""

    def __init__(self, c, levels=None, dim=None, n=None, null_table=None):
        lib, native = _lib()
        self.c, N, d, L = c, c['N'], c['dim'], c['L']
        self.P = [Buf(N, d, data=_dev(t)) for t in c['tables']]
        self.msg = Buf(1, max(L, 1) * 2 * c['n'] * d)
        self.head = IBuf(N, dtype=torch.int32)
        self.head.view.fill_(native.TPNET_HEAD_EMPTY)
        self.now_out = IBuf(1)
        is_f64 = isinstance(c['now'], float)
        self.now = torch.tensor([c['now']], dtype=torch.float64 if is_f64 else torch.int64, device=DEV)
        self.src, self.dst, self.time = _dev(c['src']), _dev(c['dst']), _dev(c['time'])
        assert self.src.dtype == torch.int32 and self.time.dtype == torch.int64
        tb = native.TPNetTables()
        tb.levels, tb.dim, tb.num_nodes = (L + 1 if levels is None else levels), (d if dim is None else dim), N
        for i, p in enumerate(self.P):
            tb.P[i] = None if i == null_table else p.ptr
        self.rc = lib.tgmx_tpnet_update(ctypes.byref(tb), self.src.data_ptr(), self.dst.data_ptr(), self.time.data_ptr(), c['n'] if n is None else n,
                                        c['lam'], self.now.data_ptr(), int(is_f64), self.now_out.ptr, self.msg.ptr, self.head.ptr,
                                        native.stream_ptr())
        torch.cuda.synchronize()
        self.empty = native.TPNET_HEAD_EMPTY

    def guards_intact(self):
        return all(p.sentinels_intact() for p in self.P) and self.msg.sentinels_intact() and self.head.sentinels_intact() and self.now_out.sentinels_intact()

    def head_is_empty(self):
        return bool((self.head.view == self.empty).all())

    def nothing_touched(self):
        same = all(_same_bits(p.view, _dev(t)) for p, t in zip(self.P, self.c['tables']))
        return same and self.guards_intact() and self.head_is_empty() and _untouched(self.msg) and bool((self.now_out.flat == ISENT).all())


def _check_update(case, exact):
    c = update_case(*case)
    want, bounds = update_bounds(case)
    a, b = UpdateRun(c), UpdateRun(c)
    assert a.rc == 0 and b.rc == 0
    assert a.guards_intact() and b.guards_intact(), 'a write past a table, past msg [L, 2 n, dim], past head [N] or past now_out'
    assert all(_same_bits(p.view, q.view) for p, q in zip(a.P, b.P)), 'two launches differ'
    assert a.head_is_empty(), 'head holds TGMX_TPNET_HEAD_EMPTY again on exit'
    assert int(a.now_out.view[0]) == int(c['time'][-1])
    assert _same_bits(a.P[0].view, _dev(c['tables'][0])), 'level 0 is never written'
    worst = 0.0
    for i in range(1, c['L'] + 1):
        got = a.P[i].view.cpu()
        if exact:
            assert torch.equal(want[i], want[i].round()) and _same_bits(got, want[i].float()), f'level {i}: integers, order-free'
        worst = max(worst, _report(f'update {case} level {i}', got, want[i], bounds[i]))
    if 'unnamed' in c and c['L']:
        u = c['unnamed']
        for i in range(1, c['L'] + 1):
            got, was = a.P[i].view[u].cpu(), c['tables'][i][u]
            if c['flag'] in ('now_is_next', 'exact'):
                assert _same_bits(got, was), 'a row nobody names keeps its bits when the decay is exactly 1 (-0.0 and a denormal among them)'
            else:  # float32(sc) and one multiply
                assert bool(((got.double() - want[i][u]).abs() <= 2.001 * EPS * want[i][u].abs()).all()), 'the two-rounding bound of a rescale'
        if c['flag'] == 'now_is_next':
            assert _bits_of(c['tables'][1][u, :1]).item() == -2 ** 31 and 0 < float(c['tables'][1][u, -1]) < 2.0 ** -126
    return worst


@pytest.mark.parametrize('case', ref.UPDATE_CASES, ids=str)
def test_update(case):
    """Every level elementwise against float64 within (count + 5 + 8) 2^-24 (|P sc| + sum |msg|), count the row's own number of
    messages.  The planted rows (oracle.tpnet_fwd_ref.update_case): a hub whose contributions lie in chunks 0, 2 and 3 of the apply
    kernel's 64-entry scan (n = 100) or across j = 64 (n = 40); a node whose only contribution is j = 2 n - 1, the last entry, in the
    second chunk or later (n >= 33): the scan starts at head & ~63 and must not stop short of 2 n; a self loop (n = 33: its
    contributions are j = 31 and j = 64); one edge twice; an edge with src >= N and one with dst = -1 (no contribution to either end);
    a node nobody names (bits kept under now == next, one rescale otherwise).  (33, .., 'float_now') and (12, .., 'float_now') hand
    ``now`` over as a double (now_is_f64 = 1) and are judged against the oracle with the same float."""
    assert _check_update(case, exact=False) <= 1.0


@pytest.mark.parametrize('case', ref.UPDATE_EXACT_CASES + [ref.UPDATE_BIG_CASE], ids=str)
def test_update_exact(case):
    """Small-integer tables and lam = 0: every factor is 1 and every sum an integer below 2^24, so the result is the float64 one bit for
    bit whatever the order.  The BIG case has 2 n L = 65 540 stage items and N = 65 539 apply rows: wave_blocks caps both grids at
    16 384 blocks x 4 waves and the grid-stride loops take a second trip for exactly the tail."""
    assert _check_update(case, exact=True) == 0.0


def test_update_no_edges_touches_nothing():
    r = UpdateRun(update_case(12, 15, 63, 1, ''), n=0)
    assert r.rc == 0 and r.nothing_touched()


@pytest.mark.parametrize('what', ['levels=9', 'dim=0', 'null table', '2n >= HEAD_EMPTY'])
def test_update_refusals(what):
    """The refusals return TGMX_E_INVALID before anything is launched; the oversized n is a number only (the buffers are the case's)."""
    c = update_case(12, 15, 63, 1, '')
    kw = {'levels=9': dict(levels=9), 'dim=0': dict(dim=0), 'null table': dict(null_table=1), '2n >= HEAD_EMPTY': dict(n=0x7F7F7F7F // 2 + 1)}[what]
    r = UpdateRun(c, **kw)
    assert r.rc == E_INVALID and r.nothing_touched()


def test_update_one_level_only_moves_the_clock():
    c = update_case(12, 15, 63, 0, '')
    r = UpdateRun(c)
    assert r.rc == 0 and r.guards_intact() and r.head_is_empty() and _untouched(r.msg)
    assert _same_bits(r.P[0].view, _dev(c['tables'][0])) and int(r.now_out.view[0]) == int(c['time'][-1])


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tpnet_pair_features
# ---------------------------------------------------------------------------------------------------------------------------
def _pair_tables(c):
    """(TPNetTables, the tensors it points into).  offset: every table is a view one float into its allocation -- 4-byte aligned only."""
    _, native = _lib()
    keep = []
    tb = native.TPNetTables()
    tb.levels, tb.dim, tb.num_nodes = len(c['tables']), c['dim'], c['N']
    for i, t in enumerate(c['tables']):
        if c['offset']:
            store = torch.full((t.numel() + 1,), float('nan'), device=DEV)
            store[1:].copy_(_dev(t).view(-1))
            keep.append(store)
            tb.P[i] = store.data_ptr() + 4
            assert tb.P[i] % 8 == 4
        else:
            keep.append(_dev(t))
            tb.P[i] = keep[-1].data_ptr()
            assert tb.P[i] % 8 == 0
    return tb, keep


def _pair(c, tb=None, n=None, ldo=None, k=None):
    lib, native = _lib()
    keep = None
    if tb is None:
        tb, keep = _pair_tables(c)
    total = c['n'] * (2 if c['b1'] is not None else 1)
    out = Buf(total, c['ldo'])
    a, rows, b0, b1 = _dev(c['a']), (None if c['a_rows'] is None else _dev(c['a_rows'])), _dev(c['b0']), (None if c['b1'] is None else _dev(c['b1']))
    rc = lib.tgmx_tpnet_pair_features(ctypes.byref(tb), a.data_ptr(), _ptr(rows), c['a_num_rows'], c['k'] if k is None else k, b0.data_ptr(), _ptr(b1),
                                      c['bmod'], c['n'] if n is None else n, c['concat'], c['scale'], out.ptr, c['ldo'] if ldo is None else ldo,
                                      native.stream_ptr())
    torch.cuda.synchronize()
    del keep
    return rc, out


def _check_pair(tag, c):
    want, bound = ref.pair_bounds(c)
    (rc, x), (rc2, y) = _pair(c), _pair(c)
    assert rc == 0 and rc2 == 0
    assert x.sentinels_intact() and y.sentinels_intact(), 'a write past [n or 2 n, ldo]'
    assert _same_bits(x.view, y.view), 'two launches differ'
    got, NR = x.view.cpu(), c['NR']
    assert got.shape[0] == want.shape[0]
    assert _same_bits(got[:, NR * NR:], torch.zeros(got.shape[0], c['ldo'] - NR * NR)), 'columns NR^2 .. ldo are zeros'
    body = got[:, :NR * NR].contiguous()
    if c['concat']:
        sq = body.view(-1, NR, NR)
        assert _same_bits(sq, sq.transpose(1, 2).contiguous()), 'a Gram matrix: out[r, s] and out[s, r] are one value'
    return _report(tag, body, want, bound)


@pytest.mark.parametrize('case', ref.PAIR_CASES, ids=lambda c: '-'.join(map(str, c)))
def test_pair_features(case):
    """(NL, concat, dim, scale, k, rows, b1, short_bmod, ldo_pad, offset): all 16 instances of tpnet_pair_kernel (NL = 1 .. 4, Gram
    and cross, float2 and scalar loads) at dim = 1, 2, 63, 64, 65, 128, 130, 300, ELEMENTWISE -- a transposed cross block or a
    misplaced entry fails, not just a large one.  offset = 1: an even dim with 4-byte aligned tables, the scalar route that odd dims
    alone reach otherwise.  Slots hold the ids 0, N - 1 and -1; a_rows holds a -1 and an a_num_rows (both read as pads); b is indexed
    by q mod 4 with 6 sequences; items [n, 2 n) against b1."""
    assert _check_pair(f'pair {case}', pair_case(case)) <= 1.0


def test_pair_features_big():
    """65 539 items, one wave each: 3 past 16 384 blocks x 4 waves.  dim = 2: every sum has two terms."""
    assert _check_pair('pair BIG', pair_case(ref.PAIR_BIG_CASE, items=65539)) <= 1.0


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('concat', [1, 0])
def test_pair_pad_id_is_the_last_row_bit_for_bit(concat, offset):
    base = pair_case((3, concat, 130, 1, 1, 0, 1, 0, 0, offset))
    N = base['N']
    c = dict(base, a=torch.tensor([-1, N - 1, 5, -1, N - 1, 5], dtype=torch.int32).view(6, 1), b0=torch.tensor([4, 4, 4, -1, N - 1, -1], dtype=torch.int32),
             b1=torch.tensor([N - 1, -1, 7, 2, 2, 2], dtype=torch.int32))
    rc, out = _pair(c)
    got = out.view.cpu()
    assert rc == 0 and out.sentinels_intact()
    for i, j in ((0, 1), (3, 4), (6, 7), (9, 10)):
        assert _same_bits(got[i], got[j]), (i, j)
    assert not _same_bits(got[0], got[2])


def test_pair_refusals():
    """NL = 5: TGMX_E_UNSUPPORTED; ldo below NR^2 and n not a multiple of k: TGMX_E_INVALID; the output untouched each time."""
    _, native = _lib()
    c = pair_case((4, 0, 64, 0, 5, 0, 0, 0, 0, 0))
    tb, keep = _pair_tables(c)
    extra = _dev(c['tables'][0])
    tb.P[4], tb.levels = extra.data_ptr(), 5
    wide = dict(c, ldo=25)
    rc, out = _pair(wide, tb=tb)
    assert rc == E_UNSUPPORTED == native.E_UNSUPPORTED and _untouched(out) and out.sentinels_intact()
    for kw in (dict(ldo=15), dict(n=c['n'] - 1)):
        rc, out = _pair(c, **kw)
        assert rc == E_INVALID and _untouched(out) and out.sentinels_intact(), kw


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tpnet_tokens
# ---------------------------------------------------------------------------------------------------------------------------
def _tokens(c, B=None):
    lib, native = _lib()
    R = 2 * c['B'] * c['k']
    out = Buf(R, c['ldo'])
    d = {n: (None if c[n] is None else _dev(c[n])) for n in ('node_x', 'edge_time', 'nids', 'nbr_t', 'nbr_x', 'rows', 'tw', 'tb', 'pf')}
    assert d['nids'].dtype == torch.int32 and d['nbr_t'].dtype == torch.int64 and d['edge_time'].dtype == torch.int64
    rc = lib.tgmx_tpnet_tokens(_ptr(d['node_x']), c['N'], c['dN'], d['edge_time'].data_ptr(), c['B'] if B is None else B, d['nids'].data_ptr(),
                               d['nbr_t'].data_ptr(), _ptr(d['nbr_x']), c['S'], c['k'], c['dE'], _ptr(d['rows']), _ptr(d['tw']), _ptr(d['tb']), c['dT'],
                               _ptr(d['pf']), c['ldpf'], c['pfd'], out.ptr, c['ldo'], native.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def _check_tokens(tag, c):
    want, bound, _ = ref.token_run(c)
    (rc, x), (rc2, y) = _tokens(c), _tokens(c)
    assert rc == 0 and rc2 == 0
    assert x.sentinels_intact() and y.sentinels_intact(), 'a write past [2 B k, ldo]'
    assert _same_bits(x.view, y.view), 'two launches differ'
    got = x.view.cpu()
    t0, t1 = c['dN'], c['dN'] + c['dT']
    exact = torch.ones(c['ldo'], dtype=torch.bool)
    exact[t0:t1] = False
    assert _same_bits(got[:, exact], want[:, exact].float()), 'node, edge and pair columns are copies; their zeros and the padding are exact'
    k, Q = c['k'], 2 * c['B']
    hr = torch.arange(Q) if c['rows'] is None else c['rows'].long()
    inb = (hr >= 0) & (hr < c['S'])
    ids = torch.where(inb[:, None], c['nids'].long()[hr.clamp(0, c['S'] - 1)], torch.full((), -1, dtype=torch.int64)).reshape(-1)
    pad, beyond = ids == -1, ids >= c['N']
    assert bool(pad.view(Q, k).all(1).any()) and bool(beyond.any()), 'an all-pad sequence and an id >= num_nodes are among the tokens'
    assert c['rows'] is None or int((~inb).sum()) == 2
    assert _same_bits(got[pad][:, :t1], torch.zeros(int(pad.sum()), t1)), 'pad slots: node and time columns are zeros'
    if c['dE']:
        assert _same_bits(got[(~inb).repeat_interleave(k)][:, t1:t1 + c['dE']], torch.zeros(int((~inb).sum()) * k, c['dE']))
        assert bool(got[pad & inb.repeat_interleave(k)][:, t1:t1 + c['dE']].any()), 'a pad slot of a row in range keeps what the sampler wrote'
    if c['dN']:
        assert not bool(got[beyond][:, :t0].any())
    if c['dT']:
        assert bool((got[beyond][:, t0:t1] != 0).all()), 'an id >= num_nodes that is not a pad still has its time encoding'
    return _report(tag, got, want, bound)


@pytest.mark.parametrize('case', ref.TOKEN_CASES, ids=str)
def test_tokens(case):
    """(B, k, dN, dT, dE, pfd, ldo, rows): each width alone (the other three segments have zero width), mixed widths with padding
    columns, 63 | 64 | 65 around a 64-lane trip, the example's 128 | 100 | 172 | 2 x 36.  Tokens (oracle.tpnet_fwd_ref.token_case): an
    all-pad row, pad slots whose edge features are not zero, an id >= num_nodes that is not a pad, gaps 1, 0, 2^24 + 1 and 2^31 - 1;
    rows = 1: row indices with a -1 and an S (all pads, zero edge features).  The time columns: cos in double, rounded once."""
    assert _check_tokens(f'tokens {case}', token_case(*case)) <= 1.0


def test_tokens_big():
    """2 B k = 65 552 token rows, one wave each: 16 past 16 384 blocks x 4 waves."""
    assert _check_tokens('tokens BIG', token_case(*ref.TOKEN_BIG_CASE)) <= 1.0


def test_tokens_no_pairs_touches_nothing():
    rc, out = _tokens(token_case(*ref.TOKEN_CASES[8]), B=0)
    assert rc == 0 and _untouched(out) and out.sentinels_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tpnet_mean
# ---------------------------------------------------------------------------------------------------------------------------
def _mean(z_ptr, ldz, Q, k, C, ldo):
    lib, native = _lib()
    out = Buf(Q, C, ld=ldo)
    rc = lib.tgmx_tpnet_mean(z_ptr, ldz, Q, k, C, out.ptr, ldo, native.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize('Q,k,C', ref.MEAN_CASES + [ref.MEAN_BIG_CASE])
def test_mean(Q, k, C):
    """z rows three floats wider than C (the gap holds 1e30), out rows one float wider.  (65539, 1, 32): Q C = 8192 x 256 + 96 -- the
    block cap holds and the grid stride takes a second trip for the tail.  k = 1: a copy, bit for bit."""
    c = mean_case(Q, k, C)
    want, bound = ref.mean_bounds(c)
    z = Buf(Q * k, C, ld=c['ldz'], fill=1e30, data=_dev(c['z']))
    (rc, a), (rc2, b) = _mean(z.ptr, c['ldz'], Q, k, C, c['ldo']), _mean(z.ptr, c['ldz'], Q, k, C, c['ldo'])
    assert rc == 0 and rc2 == 0 and a.sentinels_intact() and b.sentinels_intact(), 'a write past [Q, C] of ldo'
    assert _same_bits(a.view, b.view), 'two launches differ'
    if k == 1:
        assert _same_bits(a.view.cpu(), c['z'])
    assert _report(f'mean {(Q, k, C)}', a.view.cpu(), want, bound) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# tgmx_tpnet_forward / tgmx_tpnet_forward_train against their parts
# ---------------------------------------------------------------------------------------------------------------------------
FWD_E, FWD_NL, FWD_DIM = 8, 2, 10
up4 = lambda v: (v + 3) // 4 * 4


def _forward(c, num_layers, with_tables, train=False, fix_ids=True, seed=0):
    """One call over a token case (its pf is not used: the call computes its own).  Returns a dict of the guarded buffers, the device
    inputs and a state_dict for tests/tpnet_restate.tpnet_forward."""
    lib, native = _lib()
    g = torch.Generator().manual_seed(500 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    B, k, dN, dT, dE, N, E = c['B'], c['k'], c['dN'], c['dT'], c['dE'], c['N'], FWD_E
    Q, R = 2 * B, 2 * B * k
    NR = 2 * FWD_NL
    od = NR * NR if with_tables else 0
    W = dN + dT + dE + 2 * od
    Ht, Hc = max(k // 2, 1), 2 * E
    nids = c['nids'].clone()
    if fix_ids:
        nids[nids >= N] = 3
    tw, tb = (c['tw'], c['tb']) if dT else (torch.zeros(0), torch.zeros(0))
    sd = {'time_encoder.w.weight': tw[:, None], 'time_encoder.w.bias': tb, 'projection_layer.0.weight': r(2 * E, W) / W ** 0.5,
          'projection_layer.0.bias': 0.1 * r(2 * E), 'projection_layer.2.weight': r(E, 2 * E) / (2 * E) ** 0.5, 'projection_layer.2.bias': 0.1 * r(E)}
    if with_tables:
        for i in range(FWD_NL):
            sd[f'random_projections.random_projections.{i}'] = r(N, FWD_DIM) / FWD_DIM ** 0.25
        sd.update({'random_projections.mlp.0.weight': r(4 * od, od) / od ** 0.5, 'random_projections.mlp.0.bias': 0.1 * r(4 * od),
                   'random_projections.mlp.2.weight': r(od, 4 * od) / (4 * od) ** 0.5, 'random_projections.mlp.2.bias': 0.1 * r(od)})
    for l in range(num_layers):
        p = f'mlp_mixers.{l}.'
        sd.update({p + 'token_norm.weight': 1 + 0.1 * r(k), p + 'token_norm.bias': 0.1 * r(k), p + 'token_feedforward.ffn.0.weight': r(Ht, k) / k ** 0.5,
                   p + 'token_feedforward.ffn.0.bias': 0.1 * r(Ht), p + 'token_feedforward.ffn.3.weight': r(k, Ht) / Ht ** 0.5,
                   p + 'token_feedforward.ffn.3.bias': 0.1 * r(k), p + 'channel_norm.weight': 1 + 0.1 * r(E), p + 'channel_norm.bias': 0.1 * r(E),
                   p + 'channel_feedforward.ffn.0.weight': r(Hc, E) / E ** 0.5, p + 'channel_feedforward.ffn.0.bias': 0.1 * r(Hc),
                   p + 'channel_feedforward.ffn.3.weight': r(E, Hc) / Hc ** 0.5, p + 'channel_feedforward.ffn.3.bias': 0.1 * r(E)})
    src, dst = (torch.randint(0, N, (B,), generator=g, dtype=torch.int32) for _ in range(2))
    dev = {n: _dev(v.reshape(-1) if n == 'time_encoder.w.weight' else v) for n, v in sd.items()}
    opt = lambda t: None if t is None else _dev(t)
    inp = dict(node_x=opt(c['node_x']), src=_dev(src), dst=_dev(dst), edge_time=_dev(c['edge_time']), nids=_dev(nids), nbr_t=_dev(c['nbr_t']),
               nbr_x=opt(c['nbr_x']), rows=opt(c['rows']))
    blk = native.TPNetFwd()
    blk.node_x, blk.num_nodes, blk.src, blk.dst, blk.edge_time, blk.B = _ptr(inp['node_x']), N, inp['src'].data_ptr(), inp['dst'].data_ptr(), \
        inp['edge_time'].data_ptr(), B
    blk.nbr_nids, blk.nbr_t, blk.nbr_x, blk.S, blk.rows = inp['nids'].data_ptr(), inp['nbr_t'].data_ptr(), _ptr(inp['nbr_x']), c['S'], _ptr(inp['rows'])
    blk.k, blk.dN, blk.dE, blk.dT, blk.E, blk.num_layers, blk.eps = k, dN, dE, dT, E, num_layers, 1e-5
    blk.rp_concat, blk.rp_scale, blk.rp_out_dim = 1, 1, od
    P = lambda n: dev[n].data_ptr()
    if with_tables:
        blk.tables.levels, blk.tables.dim, blk.tables.num_nodes = FWD_NL, FWD_DIM, N
        for i in range(FWD_NL):
            blk.tables.P[i] = P(f'random_projections.random_projections.{i}')
        blk.rp_w1, blk.rp_b1, blk.rp_w2, blk.rp_b2 = (P(f'random_projections.mlp.{n}') for n in ('0.weight', '0.bias', '2.weight', '2.bias'))
    blk.tw, blk.tb = _ptr(dev['time_encoder.w.weight']), _ptr(dev['time_encoder.w.bias'])
    blk.proj_w0, blk.proj_b0, blk.proj_w2, blk.proj_b2 = (P(f'projection_layer.{n}') for n in ('0.weight', '0.bias', '2.weight', '2.bias'))
    for l in range(num_layers):
        ly, p = blk.layers[l], f'mlp_mixers.{l}.'
        ly.tok_g, ly.tok_b, ly.ch_g, ly.ch_b = (P(p + n) for n in ('token_norm.weight', 'token_norm.bias', 'channel_norm.weight', 'channel_norm.bias'))
        ly.tok_w1, ly.tok_b1, ly.tok_w2, ly.tok_b2 = (P(p + 'token_feedforward.ffn.' + n) for n in ('0.weight', '0.bias', '3.weight', '3.bias'))
        ly.ch_w1, ly.ch_b1, ly.ch_w2, ly.ch_b2 = (P(p + 'channel_feedforward.ffn.' + n) for n in ('0.weight', '0.bias', '3.weight', '3.bias'))
        ly.tok_hidden, ly.ch_hidden = Ht, Hc
    ld = dict(ldf=up4(max(od, 1)), ldfh=up4(max(4 * od, 1)), ldx0=up4(W), ldhp=up4(2 * E), ldz=up4(E), ldh=up4(Hc))
    R2 = 2 * R if od else 1
    bufs = dict(feat=Buf(R2, ld['ldf']), feat_h=Buf(R2, ld['ldfh']), pf=Buf(R2, ld['ldf']), x0=Buf(R, ld['ldx0']), hp=Buf(R, ld['ldhp']),
                z=Buf(R, ld['ldz']), z1=Buf(R, ld['ldz']), y=Buf(R, ld['ldz']), h=Buf(R, ld['ldh']), out=Buf(Q, E))
    for n in ('feat', 'feat_h', 'pf', 'x0', 'hp', 'z', 'z1', 'y', 'h', 'out'):
        setattr(blk, n, bufs[n].ptr)
    for n, v in ld.items():
        setattr(blk, n, v)
    lg = None
    if train:
        lg = torch.full((R + 64,), float('nan'), dtype=torch.float64, device=DEV)
        sz, sz1 = Buf(max(num_layers, 1) * R, ld['ldz']), Buf(max(num_layers, 1) * R, ld['ldz'])
        save = native.TPNetSave(sz.ptr, sz1.ptr, lg.data_ptr())
        rc = lib.tgmx_tpnet_forward_train(ctypes.byref(blk), ctypes.byref(save), None, native.stream_ptr())
        bufs.update(save_z=sz, save_z1=sz1)
    else:
        rc = lib.tgmx_tpnet_forward(ctypes.byref(blk), native.stream_ptr())
    torch.cuda.synchronize()
    native.check(rc, 'tpnet_forward')
    assert all(b.sentinels_intact() for b in bufs.values()), 'a write past a scratch buffer or past out'
    return dict(bufs=bufs, inp=inp, sd=sd, dev=dev, blk=blk, ld=ld, od=od, W=W, lg=lg, nids=nids, src=src, dst=dst, R=R)


@pytest.mark.parametrize('rows', [0, 1], ids=['identity', 'rows'])
@pytest.mark.parametrize('with_tables', [1, 0], ids=['tables', 'no_tables'])
@pytest.mark.parametrize('num_layers', [0, 2])
def test_forward_is_its_parts(num_layers, with_tables, rows):
    """After tgmx_tpnet_forward: feat holds the bits of tgmx_tpnet_pair_features alone, x0 those of tgmx_tpnet_tokens alone fed the
    call's own pf, out those of tgmx_tpnet_mean alone over the call's own z; out is within the 1e-4 bar of tests/test_tpnet_gpu.py of
    the float64 restatement of the whole encoder (row indices outside hop 0 restated as an all-pad row)."""
    lib, native = _lib()
    c = token_case(6, 8, 5, 4, 4, 4, 25, rows)
    f = _forward(c, num_layers, with_tables)
    bufs, inp, blk, ld, od, R, k, B, E = f['bufs'], f['inp'], f['blk'], f['ld'], f['od'], f['R'], c['k'], c['B'], FWD_E
    st = native.stream_ptr()
    if od:
        feat = Buf(2 * R, ld['ldf'])
        native.check(lib.tgmx_tpnet_pair_features(ctypes.byref(blk.tables), inp['nids'].data_ptr(), _ptr(inp['rows']), c['S'], k, inp['src'].data_ptr(),
                                                  inp['dst'].data_ptr(), B, R, 1, 1, feat.ptr, ld['ldf'], st), 'pair_features')
        torch.cuda.synchronize()
        assert feat.sentinels_intact() and _same_bits(feat.view, bufs['feat'].view)
    x0 = Buf(R, ld['ldx0'])
    native.check(lib.tgmx_tpnet_tokens(inp['node_x'].data_ptr(), c['N'], c['dN'], inp['edge_time'].data_ptr(), B, inp['nids'].data_ptr(),
                                       inp['nbr_t'].data_ptr(), inp['nbr_x'].data_ptr(), c['S'], k, c['dE'], _ptr(inp['rows']), blk.tw, blk.tb, c['dT'],
                                       bufs['pf'].ptr if od else None, ld['ldf'], od, x0.ptr, ld['ldx0'], st), 'tokens')
    out = Buf(2 * B, E)
    native.check(lib.tgmx_tpnet_mean(bufs['z'].ptr, ld['ldz'], 2 * B, k, E, out.ptr, E, st), 'mean')
    torch.cuda.synchronize()
    assert x0.sentinels_intact() and _same_bits(x0.view, bufs['x0'].view)
    assert out.sentinels_intact() and _same_bits(out.view, bufs['out'].view)
    # the whole encoder in float64: an out-of-range row index is one more hop-0 row of pads with zero edge features
    S = c['S']
    sel = torch.arange(2 * B) if c['rows'] is None else c['rows'].long()
    sel = torch.where((sel >= 0) & (sel < S), sel, torch.full((), S))
    nids = torch.cat([f['nids'], torch.full((1, k), -1, dtype=torch.int32)])[sel]
    nbr_t = torch.cat([c['nbr_t'], torch.zeros(1, k, dtype=torch.int64)])[sel]
    nbr_x = torch.cat([c['nbr_x'], torch.zeros(1, k, c['dE'])])[sel]
    rp = dict(num_layer=FWD_NL - 1, concat=True, scale=True) if od else None
    zs, zd = tr.tpnet_forward(f['sd'], num_layers, rp, c['node_x'], f['src'], f['dst'], c['edge_time'], nids, nbr_t, nbr_x)
    err = tr.rel_err(bufs['out'].view, torch.cat([zs, zd]))
    print(f'[blocks] forward layers={num_layers} tables={with_tables} rows={rows}: out vs float64 {err:.3e}')
    assert err < 1e-4


@pytest.mark.parametrize('case', [c for c in ref.TOKEN_CASES if c[2] + c[3] + c[4] > 0], ids=str)
def test_saved_log_gaps(case):
    """save->lg of tgmx_tpnet_forward_train (num_layers = 0, no tables): the double the forward feeds the cosine, log(double(gap + 1)),
    within 4 * 2^-53 relative of the host's float64 log (an ulp each), exactly 0 at a gap of 0 and exactly -1 on a pad slot; x0 holds the
    bits of tgmx_tpnet_tokens alone."""
    c = dict(token_case(*case), pf=None, pfd=0)
    f = _forward(c, 0, 0, train=True, fix_ids=False)
    _, _, want = ref.token_run(dict(c, ldo=f['ld']['ldx0']))
    lg = f['lg'].cpu()
    assert bool(torch.isnan(lg[f['R']:]).all()), 'a write past lg [2 B k]'
    got = lg[: f['R']]
    pad = want == -1
    assert bool(pad.any()) and torch.equal(got[pad], want[pad]), 'exactly -1 on pads'
    assert bool((want == 0).any()) and bool(((got - want).abs() <= 4 * 2.0 ** -53 * want.abs()).all())
    rc, x0 = _tokens(dict(c, ldo=f['ld']['ldx0'], ldpf=0))
    assert rc == 0 and _same_bits(x0.view, f['bufs']['x0'].view)
