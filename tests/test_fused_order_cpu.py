"""Row order of the fused hop-0 + hop-1 launch (recency.hip: fused_row_of), through its host mirror tgmx_fused_row_order: which hop-1
row the i-th hop-1 wave takes.  Mode 0 is the identity, mode 1 deals the seeds round-robin across equal seed groups, mode 2 also
runs the newest quad of every seed's rows first.  No device is needed."""

import ctypes

import numpy as np
import pytest

R = 4  # waves per workgroup of the fused launch: the quad

S0S = [1, 3, 21, 222, 600]
K0S = [1, 4, 5, 20, 64]
LAYOUTS = ['none', 'one', 'two', 'three_equal', 'three_unequal']


def _group_end(S0, layout):
    """Exclusive end offsets of the seed groups (None: plain seed arrays), or 'skip' where S0 does not split that way."""
    if layout == 'none':
        return None
    if layout == 'one':
        return [S0]
    if layout == 'two':
        return [S0 // 2, S0] if S0 % 2 == 0 else 'skip'
    if layout == 'three_equal':
        return [S0 // 3, 2 * (S0 // 3), S0] if S0 % 3 == 0 else 'skip'
    if S0 < 3:
        return 'skip'
    a = max(1, S0 // 6)
    return [a, a + max(1, S0 // 2), S0] if a + max(1, S0 // 2) < S0 else 'skip'


def _equal(S0, ge):
    return ge is not None and len(ge) >= 2 and all(e == (g + 1) * (S0 // len(ge)) for g, e in enumerate(ge)) and S0 % len(ge) == 0


def _order(S0, k0, ge, mode):
    from tgm_amd import _native

    lib = _native.load()
    out = np.full(S0 * k0, -1, dtype=np.int64)
    arr = None if ge is None else (ctypes.c_int64 * len(ge))(*ge)
    rc = lib.tgmx_fused_row_order(S0, k0, 0 if ge is None else len(ge), arr, mode, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out


def _expected(S0, k0, ge, mode):
    """The issue's formulas, written out row by row."""
    deal = mode >= 1 and _equal(S0, ge)
    quads = mode == 2 and k0 % R == 0
    G = len(ge) if deal else 1
    n = S0 // G
    out = np.empty(S0 * k0, dtype=np.int64)
    for i in range(S0 * k0):
        if quads:
            u, r = divmod(i, R)
            c = k0 // R - 1 - u // S0
            t, j = u % S0, c * R + r
        else:
            t, j = divmod(i, k0)
        s0 = (t % G) * n + t // G if deal else t
        out[i] = s0 * k0 + j
    return out


CASES = [(S0, k0, lay) for S0 in S0S for k0 in K0S for lay in LAYOUTS if _group_end(S0, lay) != 'skip']


def test_every_layout_is_covered():
    for lay in LAYOUTS:
        assert any(c[2] == lay for c in CASES), lay
    assert any(c[0] % R and c[2] == 'three_equal' and c[1] % R == 0 for c in CASES)  # workgroups straddle seeds


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('S0,k0,layout', CASES)
def test_permutation_and_formula(S0, k0, layout, mode):
    ge = _group_end(S0, layout)
    got = _order(S0, k0, ge, mode)
    assert np.array_equal(np.sort(got), np.arange(S0 * k0)), 'not a permutation'
    assert np.array_equal(got, _expected(S0, k0, ge, mode))


@pytest.mark.parametrize('S0,k0,layout', CASES)
def test_fallbacks_are_the_identity(S0, k0, layout):
    ge = _group_end(S0, layout)
    ident = np.arange(S0 * k0)
    assert np.array_equal(_order(S0, k0, ge, 0), ident)
    if not _equal(S0, ge):  # no groups, one group, unequal groups: nothing to deal
        assert np.array_equal(_order(S0, k0, ge, 1), ident)
        if k0 % R:
            assert np.array_equal(_order(S0, k0, ge, 2), ident)
    elif k0 % R:  # equal groups, no quads: mode 2 is mode 1
        assert np.array_equal(_order(S0, k0, ge, 2), _order(S0, k0, ge, 1))
    if S0 == 1 and k0 == R:
        assert np.array_equal(_order(S0, k0, ge, 2), ident)


@pytest.mark.parametrize('S0,k0,layout', [c for c in CASES if c[2] in ('two', 'three_equal') and c[1] % R == 0])
def test_mode2_chunks(S0, k0, layout):
    ge = _group_end(S0, layout)
    got = _order(S0, k0, ge, 2).reshape(-1, R)
    seed, j = got // k0, got % k0
    assert (seed == seed[:, :1]).all(), 'an aligned chunk spans seeds'
    assert (j == j[:, :1] + np.arange(R)).all() and (j[:, 0] % R == 0).all(), 'a chunk is not one quad'
    C = k0 // R
    quad = j[:, 0] // R
    assert np.array_equal(quad, np.repeat(np.arange(C - 1, -1, -1), S0)), 'quads do not run newest first'
    assert (quad[-S0:] == 0).all()
    # the seeds of a quad's pass are dealt round-robin from the groups
    G, n = len(ge), S0 // len(ge)
    t = np.arange(S0)
    assert np.array_equal(seed[:S0, 0], (t % G) * n + t // G)


def test_mode1_deals_the_groups():
    S0, k0, ge = 6, 5, [2, 4, 6]
    got = _order(S0, k0, ge, 1)
    assert list(got // k0)[::k0] == [0, 2, 4, 1, 3, 5]
    assert list(got[:k0] % k0) == list(range(k0))


def test_sizes_beyond_the_fast_division_keep_the_identity():
    """Past rows * max(S0, k0) = 2^32 the 32-bit reciprocals are no longer exact: every mode is the identity there."""
    S0, k0 = 16386, 16  # rows * S0 just above 2^32, equal groups of 8193
    ge = [S0 // 2, S0]
    assert S0 * k0 * S0 >= 1 << 32
    for mode in (1, 2):
        assert np.array_equal(_order(S0, k0, ge, mode), np.arange(S0 * k0))
    S0 = 16380  # just below: dealt
    ge = [S0 // 2, S0]
    assert S0 * k0 * S0 < 1 << 32
    for mode in (1, 2):
        got = _order(S0, k0, ge, mode)
        assert np.array_equal(np.sort(got), np.arange(S0 * k0)) and got[k0 if mode == 1 else R] // k0 == S0 // 2


def test_bad_arguments():
    from tgm_amd import _native

    lib = _native.load()
    out = np.zeros(4, dtype=np.int64)
    p = out.ctypes.data_as(ctypes.c_void_p)
    assert lib.tgmx_fused_row_order(1, 4, 0, None, 3, p) != 0  # no such mode
    assert lib.tgmx_fused_row_order(1, 4, 2, None, 1, p) != 0  # groups without their ends
    assert lib.tgmx_fused_row_order(1, 4, 0, None, 1, None) != 0
