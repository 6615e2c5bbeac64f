"""Which part of the ring update rides which lookup launch (``tgmx_recency_step_plan``, no GPU needed).

The schedules give bit-identical results by construction, so the GPU parity tests cannot see a boundary that moved; this
file pins the table of ``include/tgm_amd.h`` row by row, at both edges of every boundary.  The plan reads sizes and
pointer VALUES only: the pointers below are made-up aligned addresses and nothing is dereferenced.
"""
import json
import os
import subprocess
import sys

import pytest

from tgm_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# TGMX_RIDE_* / TGMX_AFTER_* / TGMX_PLAN_FUSED01 (include/tgm_amd.h)
NONE, SORT, MERGE, SORT_MERGE, PLACE_ONLY, ALL, SORT_MERGE_PLACE, MERGE_PLACE = range(8)
A_NONE, A_COMMIT, A_PRESORTED, A_MERGE_PRESORTED, A_BLOCK, A_LARGE = range(6)

WIDE = dict(D=64, B=20, k=[20, 20, 2])  # hop 0 + hop 1 as one launch
NARROW = dict(D=4, B=10, k=[8, 3, 2])  # hop 1 goes to the narrow-row kernel: two launches


def header_constants():
    import re

    text = open(os.path.join(ROOT, 'include', 'tgm_amd.h')).read()
    return {k: int(v) for k, v in re.findall(r'^#define (TGMX_(?:RIDE|AFTER|PLAN)_[A-Z0-9_]+) (\d+)', text, flags=re.M)}


def block(shape, m, directed, n_hops, S=600, static=False, groups=None):
    """A RecencyStep of m ring entries (m = n directed, m = 2 n undirected)."""
    assert directed or m % 2 == 0
    st = _native.RecencyStep()
    addr = iter(range(1 << 20, 1 << 30, 1 << 16))  # non-null, 64 KiB apart: every alignment the plan looks at
    st.ring, st.ring_x, st.status, st.scratch = next(addr), next(addr), next(addr), next(addr)
    if static:
        st.indptr = next(addr)
    else:
        st.write_pos = next(addr)
    st.D, st.B, st.num_nodes = shape['D'], shape['B'], 1000
    st.seed_nid0, st.seed_ts0 = next(addr), next(addr)
    if groups:
        st.n_groups = len(groups)
        for g, n in enumerate(groups):
            st.grp_nid[g], st.grp_ts[g], st.grp_n[g] = next(addr), next(addr), n
        st.S0 = 0
    else:
        st.S0 = S
    st.n_hops = n_hops
    for h in range(n_hops):
        st.k[h] = shape['k'][h]
        st.out_nid[h], st.out_ts[h], st.out_x[h] = next(addr), next(addr), next(addr)
    st.n = m if directed else m // 2
    st.directed = int(directed)
    if st.n:
        st.src, st.dst, st.ts, st.edge_x = next(addr), next(addr), next(addr), next(addr)
    st.timed_hop = -1
    return st


def plan_of(st):
    p = _native.load().tgmx_recency_step_plan(st)
    return dict(fused=p & 1, stage=[(p >> 4) & 15, (p >> 8) & 15], blocks=[(p >> 12) & 31, (p >> 17) & 31],
                lds=[0, 512, 1024, None][(p >> 22) & 3], after=(p >> 24) & 15, spare=p & 0xE | (p >> 28))  # fmt: skip


def row(fused, stage0=NONE, blocks0=0, stage1=NONE, blocks1=0, lds=0, after=A_NONE):
    return dict(fused=fused, stage=[stage0, stage1], blocks=[blocks0, blocks1], lds=lds, after=after, spare=0)


# m -> directed flags to try: m = n directed, m = 2 n undirected, so an odd m exists only directed
EDGES = {1: [True], 256: [True, False], 257: [True], 512: [True, False], 513: [True],
         1024: [True, False], 1025: [True], 4096: [True, False], 4097: [True]}  # fmt: skip

# the table, written out: (launches, m) -> the plan
FUSED_ROWS = {
    1: row(1, ALL, 1, lds=512, after=A_COMMIT),
    256: row(1, ALL, 1, lds=512, after=A_COMMIT),
    257: row(1, ALL, 1, lds=512, after=A_COMMIT),
    512: row(1, ALL, 1, lds=512, after=A_COMMIT),
    513: row(1, SORT_MERGE_PLACE, 3, lds=1024, after=A_COMMIT),
    1024: row(1, SORT_MERGE_PLACE, 4, lds=1024, after=A_COMMIT),
    1025: row(1, SORT_MERGE, 5, lds=0, after=A_PRESORTED),
    4096: row(1, SORT_MERGE, 16, lds=0, after=A_PRESORTED),
    4097: row(1, after=A_LARGE),
}
TWO_LAUNCH_ROWS = {
    1: row(0, SORT_MERGE, 1, PLACE_ONLY, 1, after=A_COMMIT),
    256: row(0, SORT_MERGE, 1, PLACE_ONLY, 1, after=A_COMMIT),
    257: row(0, SORT, 2, MERGE_PLACE, 2, after=A_COMMIT),
    512: row(0, SORT, 2, MERGE_PLACE, 2, after=A_COMMIT),
    513: row(0, SORT, 3, MERGE_PLACE, 3, after=A_COMMIT),
    1024: row(0, SORT, 4, MERGE_PLACE, 4, after=A_COMMIT),
    1025: row(0, SORT, 5, MERGE, 5, after=A_PRESORTED),
    4096: row(0, SORT, 16, MERGE, 16, after=A_PRESORTED),
    4097: row(0, after=A_LARGE),
}
ONE_HOP_ROWS = {
    1: row(0, SORT, 1, after=A_MERGE_PRESORTED),
    256: row(0, SORT, 1, after=A_MERGE_PRESORTED),
    257: row(0, SORT, 2, after=A_MERGE_PRESORTED),
    512: row(0, SORT, 2, after=A_MERGE_PRESORTED),
    513: row(0, SORT, 3, after=A_MERGE_PRESORTED),
    1024: row(0, SORT, 4, after=A_MERGE_PRESORTED),
    1025: row(0, SORT, 5, after=A_MERGE_PRESORTED),
    4096: row(0, SORT, 16, after=A_MERGE_PRESORTED),
    4097: row(0, after=A_LARGE),
}


def test_constants_match_the_header():
    c = header_constants()
    assert c == {
        'TGMX_PLAN_FUSED01': 1,
        'TGMX_RIDE_NONE': NONE, 'TGMX_RIDE_SORT': SORT, 'TGMX_RIDE_MERGE': MERGE, 'TGMX_RIDE_SORT_MERGE': SORT_MERGE,
        'TGMX_RIDE_PLACE_ONLY': PLACE_ONLY, 'TGMX_RIDE_ALL': ALL, 'TGMX_RIDE_SORT_MERGE_PLACE': SORT_MERGE_PLACE,
        'TGMX_RIDE_MERGE_PLACE': MERGE_PLACE,
        'TGMX_AFTER_NONE': A_NONE, 'TGMX_AFTER_COMMIT': A_COMMIT, 'TGMX_AFTER_PRESORTED': A_PRESORTED,
        'TGMX_AFTER_MERGE_PRESORTED': A_MERGE_PRESORTED, 'TGMX_AFTER_BLOCK': A_BLOCK, 'TGMX_AFTER_LARGE': A_LARGE,
    }  # fmt: skip
    assert sorted(v for k, v in c.items() if '_RIDE_' in k) == list(range(8))  # no gaps
    assert sorted(v for k, v in c.items() if '_AFTER_' in k) == list(range(6))


@pytest.mark.parametrize('m', sorted(EDGES))
@pytest.mark.parametrize('n_hops', [2, 3])
def test_fused_launch_rows(m, n_hops):
    for directed in EDGES[m]:
        assert plan_of(block(WIDE, m, directed, n_hops)) == FUSED_ROWS[m], (m, directed)


@pytest.mark.parametrize('m', sorted(EDGES))
@pytest.mark.parametrize('n_hops', [2, 3])
def test_two_launch_rows(m, n_hops):
    for directed in EDGES[m]:
        assert plan_of(block(NARROW, m, directed, n_hops)) == TWO_LAUNCH_ROWS[m], (m, directed)


@pytest.mark.parametrize('m', sorted(EDGES))
@pytest.mark.parametrize('shape', [WIDE, NARROW], ids=['wide', 'narrow'])
def test_single_hop_rows(m, shape):
    for directed in EDGES[m]:
        assert plan_of(block(shape, m, directed, 1)) == ONE_HOP_ROWS[m], (m, directed)


@pytest.mark.parametrize('m', sorted(EDGES))
@pytest.mark.parametrize('shape', [WIDE, NARROW], ids=['wide', 'narrow'])
def test_nothing_rides_without_a_hop_or_a_seed(m, shape):
    whole = row(0, after=A_LARGE if m == 4097 else A_BLOCK)
    for directed in EDGES[m]:
        assert plan_of(block(shape, m, directed, 0)) == whole  # update only
        for n_hops in (1, 2, 3):
            assert plan_of(block(shape, m, directed, n_hops, S=0)) == whole  # no seed: no lookup launch to ride
            assert plan_of(block(shape, m, directed, n_hops, groups=[0, 0])) == whole


def test_seed_groups_count_as_seeds():
    assert plan_of(block(WIDE, 800, False, 2, groups=[3, 0, 4])) == row(1, SORT_MERGE_PLACE, 4, lds=1024, after=A_COMMIT)
    assert plan_of(block(NARROW, 800, False, 2, groups=[3, 0, 4])) == row(0, SORT, 4, MERGE_PLACE, 4, after=A_COMMIT)


@pytest.mark.parametrize('n_hops', [0, 1, 2, 3])
def test_no_batch_and_static_index_take_no_update(n_hops):
    assert plan_of(block(WIDE, 0, True, n_hops)) == row(1 if n_hops >= 2 else 0)
    assert plan_of(block(NARROW, 0, True, n_hops)) == row(0)
    assert plan_of(block(WIDE, 0, True, n_hops, static=True)) == row(1 if n_hops >= 2 else 0)  # k1 * D * 4 = 5120 bytes: wide enough
    assert plan_of(block(NARROW, 0, True, n_hops, static=True)) == row(0)


def test_bit_0_is_the_fused_launch_as_before():
    """Bit 0 alone is what both Python callers read (``& 1``): one launch for hops 0 + 1 exactly for wide rows, two or more hops and
    at least one seed, whatever the batch."""
    lib = _native.load()
    for m, flags in sorted(EDGES.items()) + [(0, [True])]:
        for directed in flags:
            for n_hops in (0, 1, 2, 3):
                for static in (False, True) if m == 0 else (False,):
                    assert lib.tgmx_recency_step_plan(block(WIDE, m, directed, n_hops, static=static)) & 1 == (1 if n_hops >= 2 else 0)
                    assert lib.tgmx_recency_step_plan(block(WIDE, m, directed, n_hops, S=0, static=static)) & 1 == 0
                    assert lib.tgmx_recency_step_plan(block(NARROW, m, directed, n_hops, static=static)) & 1 == 0
    assert lib.tgmx_recency_step_plan(None) == 0


_NO_RIDE_CHILD = """
import json, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_rider_plan_cpu as t
print(json.dumps([t.plan_of(t.block(shape, m, True, 2)) for shape in (t.WIDE, t.NARROW) for m in (400, 800, 3200, 4097)]))
"""


def test_no_ride_knob_moves_the_whole_update_behind_the_lookups():
    """TGMX_NO_RIDE is read once per process: a child process with it set."""
    env = dict(os.environ, TGMX_NO_RIDE='1')
    out = subprocess.run([sys.executable, '-c', _NO_RIDE_CHILD.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))],
                         env=env, check=True, capture_output=True, text=True).stdout  # fmt: skip
    plans = json.loads(out.strip().splitlines()[-1])
    assert plans == [row(1, after=A_BLOCK)] * 3 + [row(1, after=A_LARGE)] + [row(0, after=A_BLOCK)] * 3 + [row(0, after=A_LARGE)]
