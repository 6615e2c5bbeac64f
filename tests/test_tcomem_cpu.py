"""tCoMemPredictor and PopTrackPredictor without a device: the restatement against every g20 / g21 fixture (state, window and the structure
of integer queries bit for bit, float32 scores by the project's criterion against the float64 record), the kept behaviours by their figures,
the reference's argument checks (order, types, messages) and the refusal of CPU tensors after them, the import paths, the argument struct's
size and the hash mirror against the kernel's constants."""
import ctypes
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

import tcomem_restate as tr
from golden_util import GOLDEN_DIR, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, 'g20_tcomem_*.npz')))
EXPECTED = ['ring_wrap_k2', 'counts', 'popularity', 'no_history', 'window_moves', 'wiki_small_k50_int64', 'wiki_small_k50_float32',
            'wiki_small_k5_int64', 'wiki_small_k5_float32', 'epoch_f32', 'burst', 'selfloop_bothways', 'equal_ts', 'stale', 'query_dtypes']  # fmt: skip
POPTRACK = ['d09', 'd10', 'd037', 'int32']
with open(os.path.join(GOLDEN_DIR, 'g20_tcomem_self_noise.json')) as _f:
    NOISE = json.load(_f)

# the project's score criterion (tests/test_ncn_gpu.py): e = max |got - ref64| / max(1, |ref64|) must stay below 1e-4, and within RATIO of the
# reference's own float32 distance from float64 where that distance says something
BAR, RATIO, NOISE_FLOOR = 1e-4, 2.0, 1e-7


def check_scores(name, what, got, ref64):
    noise = NOISE[name]
    e = tr.rel_err(got, ref64)
    print(f'{name} {what}: vs float64 {e:.3e}, reference float32 vs float64 {noise:.3e}, ratio {e / noise if noise else float("inf"):.2f}')
    assert e < BAR
    if noise >= NOISE_FLOOR:
        assert e <= RATIO * noise
    return e


def calls_of(meta, a):
    """[(src, dst, ts)] per call, as int64 numpy"""
    b = a['bounds']
    return [(a['src'][b[c] : b[c + 1]], a['dst'][b[c] : b[c + 1]], a['ts'][b[c] : b[c + 1]]) for c in range(meta['calls'])]


def queries_of(meta, a, c):
    """[(src, dst, pred, pred64, dtype name, rows)] asked after call c"""
    return [(a[f'q{c}_{j}_src'], a[f'q{c}_{j}_dst'], a[f'q{c}_{j}_pred'], a[f'q{c}_{j}_pred64'], m['dtype'], m['rows'])
            for j, m in enumerate(meta['queries'][c])]  # fmt: skip


def state_of(a, c):
    """the reference's recent_ts, recent_dst, recent_len, recent_pos, popularity after call c"""
    return a['ring_ts'][:, c], a['ring_dst'][:, c], a['len'][c], a['pos'][c], a['pop'][c]


def nested_of(a, c):
    """the reference's node_to_co_occurrence after call c: both directions of every recorded pair"""
    out = {}
    for (x, y), n in zip(a[f'co{c}_pairs'].tolist(), a[f'co{c}_count'].tolist()):
        out.setdefault(x, {})[y] = n
        out.setdefault(y, {})[x] = n
    return out


def test_every_scenario_has_its_fixture():
    assert FIXTURES == sorted('g20_tcomem_' + n for n in EXPECTED) == sorted(NOISE)
    for name in FIXTURES + ['g21_poptrack_' + n for n in POPTRACK]:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, name + '.npz')) < 200_000


@pytest.mark.parametrize('name', ['g20_tcomem_' + n for n in EXPECTED])
def test_restatement_reproduces_the_fixture(name):
    meta, a = load(name)
    model = None
    for c, (s, d, t) in enumerate(calls_of(meta, a)):
        if model is None:
            model = tr.TCoMemRestated(s, d, t, meta['num_nodes'], meta['k'], meta['co_occurrence_weight'])
        else:
            model.update(s, d, t)
        assert (model.window_start, model.window_end, model.window_size) == (a['window_start'][c], a['window_end'][c], a['window_size'][c])
        ts, dst, ln, pos, pop = state_of(a, c)
        assert ts.dtype == np.float32 and dst.dtype == np.int64 and ln.dtype == pos.dtype == pop.dtype == np.float32
        assert np.array_equal(model.recent_ts, ts) and np.array_equal(model.recent_dst, dst)
        assert np.array_equal(model.len, ln) and np.array_equal(model.pos, pos) and np.array_equal(model.pop, pop)
        assert model.nested_counts() == nested_of(a, c)
        for j, (qs, qd, pred, pred64, dtype, _) in enumerate(queries_of(meta, a, c)):
            assert pred.dtype == np.float32 and pred64.dtype == np.float64
            got = model.scores(qs, qd, dtype)
            assert got.dtype == np.float32
            assert tr.rel_err(model.scores64(qs, qd, dtype), pred64) < 1e-12  # the record is this evaluation
            check_scores(name, f'call {c} query {j} ({dtype}), restated', got, pred64)
            if dtype in tr.INTEGER_QUERIES:  # the truncated term: one answer per source, in the reference's record and here
                for v in set(qs.tolist()):
                    assert len(set(pred[qs == v].tolist())) == 1 and set(got[qs == v].tolist()) == {float(model.base(v))}


@pytest.mark.parametrize('name', ['g21_poptrack_' + n for n in POPTRACK])
def test_poptrack_restatement_is_bit_for_bit(name):
    meta, a = load(name)
    model = None
    for c, (s, d, t) in enumerate(calls_of(meta, a)):
        if model is None:
            model = tr.PopTrackRestated(s, d, t, meta['num_nodes'], meta['k'], meta['decay'])
        else:
            model.update(s, d, t)
        assert a[f'pop{c}'].dtype == np.float32 and np.array_equal(model.popularity, a[f'pop{c}'])
        assert np.array_equal(model(a['q_src'], a['q_dst']), a[f'q{c}_pred'])
    assert meta['calls'] == 11


def test_fixtures_pin_the_kept_behaviours():
    # five events of one source with k = 3
    five = tr.TCoMemRestated([0] * 5, [1, 2, 3, 4, 5], [1, 2, 3, 4, 5], 6, 3)
    assert five.recent_ts[0].tolist() == [4, 5, 3] and five.recent_dst[0].tolist() == [4, 5, 3]
    assert five.pos[0] == 2 and five.len[0] == 3
    # float32 storage and window arithmetic at Unix scale
    base = 1_600_000_000
    m = tr.TCoMemRestated([0, 1], [1, 2], [base, base + 1000], 3, 2)
    assert m.window_start == base and m.size == 1000
    m.update([0], [1], [base + 900])
    assert m.recent_ts[0, 1] == 1_600_000_896
    m.update([0], [1], [base + 1100])
    assert m.window_start == 1_600_000_128 and m.window_size == 1024 and m.window_end == base + 1100
    _, a = load('g20_tcomem_epoch_f32')
    assert not (a['ring_ts'][np.isfinite(a['ring_ts'])] % 128).any() and not (a['window_start'] % 128).any()
    # all-equal timestamps give a window of 1; the end never moves back
    _, a = load('g20_tcomem_equal_ts')
    assert a['window_start'][0] == 49 and a['window_end'][0] == 50 and a['window_size'].tolist() == [1, 1, 1]
    _, a = load('g20_tcomem_stale')
    assert a['window_end'][1] == a['window_end'][0] and a['ts'][a['bounds'][1]] < a['window_end'][0]  # late events do not move the end back
    late = a['ts'][a['bounds'][2] + 2]
    assert late == 300 and late < a['window_start'][2] == 5000  # older than the window it arrives in,
    assert (a['ring_ts'][:, 2] == late).any()  # it entered the ring all the same
    # a self-loop counts 2, both directions hold one count
    _, a = load('g20_tcomem_selfloop_bothways')
    assert nested_of(a, 0) == {1: {1: 4, 2: 2}, 2: {1: 2, 2: 2}}
    # integer queries add nothing, float32 and float64 queries differ from them by the term
    meta, a = load('g20_tcomem_query_dtypes')
    (qs, qd, p64i, *_), (_, _, p32i, *_), (_, _, pf, *_), (_, _, pd, *_) = queries_of(meta, a, 1)
    assert np.array_equal(p64i, p32i) and (pf >= p64i).all() and (pf > p64i).any() and pf.dtype == pd.dtype == np.float32
    counts = nested_of(a, 1)
    assert all((f > i) == (counts.get(s, {}).get(d, 0) > 0) for s, d, f, i in zip(qs.tolist(), qd.tolist(), pf.tolist(), p64i.tolist()))
    # a source with no history answers 0
    meta, a = load('g20_tcomem_no_history')
    qs, qd, pred, *_ = queries_of(meta, a, 0)[0]
    assert pred[(qs == 9) & (qd == 1)].tolist() == [0.0]


# ---- the product's surface, as far as it goes without a device ---------------------------------------------------------------------------
T = torch.Tensor


def test_tcomem_argument_checks_carry_the_reference_s_messages():
    from tgm_amd.nn import tCoMemPredictor

    src, dst, ts = T([1, 1]), T([2, 2]), T([1, 2])
    for ratio in (0, -0.1, 1.1):
        with pytest.raises(ValueError, match=r'^Window ratio must be in \(0, 1\]$'):
            tCoMemPredictor(src, dst, ts, num_nodes=10, k=5, window_ratio=ratio)
    for w in (0, 1.5):
        with pytest.raises(ValueError, match=r'^Co-occurrence weight must be in \(0, 1\]$'):
            tCoMemPredictor(src, dst, ts, num_nodes=10, k=5, co_occurrence_weight=w)
    for k in (0, -5):
        with pytest.raises(ValueError, match=r'^K must be positive$'):
            tCoMemPredictor(src, dst, ts, num_nodes=10, k=k)
    for n in (0, -10):
        with pytest.raises(ValueError, match=r'^``num_nodes`` must be set to the total number of nodes\.$'):
            tCoMemPredictor(src, dst, ts, num_nodes=n, k=5)
    with pytest.raises(ValueError, match=r'^``k`` must be smaller than ``num_nodes``\.$'):
        tCoMemPredictor(src, dst, ts, num_nodes=10, k=11)
    with pytest.raises(TypeError, match=r"^src, dst, ts must all be Tensor, got src: <class 'str'>, dst: <class 'str'>, ts: <class 'str'>$"):
        tCoMemPredictor('1', '2', '3', num_nodes=10, k=5)
    with pytest.raises(ValueError, match=r'^mismatch shape: src: 1, dst: 2, ts: 2$'):
        tCoMemPredictor(T([1]), dst, ts, num_nodes=10, k=5)
    with pytest.raises(ValueError, match=r'^src, dst, ts must have at len > 1, got src: 0, dst: 0, ts: 0$'):
        tCoMemPredictor(T([]), T([]), T([]), num_nodes=10, k=5)
    # the reference's order: ratio, weight, k, num_nodes, k <= num_nodes, the data
    with pytest.raises(ValueError, match='Window ratio'):
        tCoMemPredictor(1, 2, 3, num_nodes=0, k=0, window_ratio=0, co_occurrence_weight=0)
    with pytest.raises(ValueError, match='Co-occurrence weight'):
        tCoMemPredictor(1, 2, 3, num_nodes=0, k=0, co_occurrence_weight=0)
    with pytest.raises(ValueError, match='K must be positive'):
        tCoMemPredictor(1, 2, 3, num_nodes=0, k=0)
    with pytest.raises(ValueError, match='num_nodes'):
        tCoMemPredictor(1, 2, 3, num_nodes=0, k=5)
    with pytest.raises(ValueError, match='smaller than'):
        tCoMemPredictor(1, 2, 3, num_nodes=4, k=5)
    with pytest.raises(TypeError):
        tCoMemPredictor(1, 2, 3, num_nodes=5, k=5)  # k == num_nodes passes


def test_poptrack_argument_checks_carry_the_reference_s_messages():
    from tgm_amd.nn import PopTrackPredictor

    src, dst, ts = torch.tensor([0, 1]), torch.tensor([2, 3]), torch.tensor([1, 2])
    with pytest.raises(ValueError, match=r'^K must be positive$'):
        PopTrackPredictor(src, dst, ts, num_nodes=4, k=-5)
    for decay in (-0.5, 0, 2):
        with pytest.raises(ValueError, match=r'^Decay must be in \(0,1\]$'):
            PopTrackPredictor(src, dst, ts, num_nodes=4, k=2, decay=decay)
    with pytest.raises(ValueError, match=r'^``num_nodes`` must be set to the total number of nodes\.$'):
        PopTrackPredictor(src, dst, ts, num_nodes=0)
    with pytest.raises(ValueError, match=r'^``k`` must be smaller than ``num_nodes``\.$'):
        PopTrackPredictor(src, dst, ts, num_nodes=4, k=10)
    with pytest.raises(TypeError, match=r"^src, dst, ts must all be Tensor, got src: <class 'str'>, dst: <class 'str'>, ts: <class 'str'>$"):
        PopTrackPredictor('1', '2', '3', num_nodes=2, k=1)
    with pytest.raises(ValueError, match=r'^src, dst, ts must have at len > 1, got src: 0, dst: 0, ts: 0$'):
        PopTrackPredictor(T([]), T([]), T([]), num_nodes=2, k=1)
    with pytest.raises(ValueError, match='K must be positive'):  # the order: k, decay, num_nodes, k <= num_nodes, the data
        PopTrackPredictor(1, 2, 3, num_nodes=0, k=0, decay=0)
    with pytest.raises(ValueError, match='Decay'):
        PopTrackPredictor(1, 2, 3, num_nodes=0, k=1, decay=0)
    with pytest.raises(ValueError, match='num_nodes'):
        PopTrackPredictor(1, 2, 3, num_nodes=0, k=1)
    with pytest.raises(ValueError, match='smaller than'):
        PopTrackPredictor(1, 2, 3, num_nodes=1, k=2)


def test_cpu_tensors_are_refused_after_the_argument_checks():
    from tgm_amd.exceptions import NativeLibraryError
    from tgm_amd.nn import PopTrackPredictor, tCoMemPredictor
    from tgm_amd.nn.modules import PopTrackPredictor as pop_by_module_path, tCoMemPredictor as by_module_path
    from tgm_amd.nn.modules.poptrack import PopTrackPredictor as pop_by_file_path
    from tgm_amd.nn.modules.t_comem import tCoMemPredictor as by_file_path

    assert tCoMemPredictor is by_module_path is by_file_path and PopTrackPredictor is pop_by_module_path is pop_by_file_path
    with pytest.raises(NativeLibraryError):
        tCoMemPredictor(T([1, 1]), T([2, 2]), T([1, 2]), num_nodes=10, k=5)
    with pytest.raises(NativeLibraryError):
        tCoMemPredictor(torch.tensor([1, 1]), torch.tensor([2, 2]), torch.tensor([1, 2]), 10, 5, capacity=64, co_occurrence_on_integer_queries=True)
    with pytest.raises(TypeError):  # both additions are keyword only
        tCoMemPredictor(torch.tensor([1, 1]), torch.tensor([2, 2]), torch.tensor([1, 2]), 10, 5, 0.15, 0.8, 64)
    with pytest.raises(NativeLibraryError):
        PopTrackPredictor(torch.tensor([0, 1]), torch.tensor([2, 3]), torch.tensor([1, 2]), num_nodes=4, k=2)

    model = tCoMemPredictor.__new__(tCoMemPredictor)  # update() on an object that never reached the device: the checks answer first
    with pytest.raises(TypeError, match=r"^src, dst, ts must all be Tensor, got src: <class 'int'>, dst: <class 'int'>, ts: <class 'int'>$"):
        model.update(1, 2, 3)
    with pytest.raises(ValueError, match=r'^src, dst, ts must have at len > 1, got src: 0, dst: 0, ts: 0$'):
        model.update(T([]), T([]), T([]))
    with pytest.raises(NativeLibraryError):
        model.update(T([1]), T([1]), T([7]))
    with pytest.raises(NativeLibraryError):
        model(T([1]), T([1]))
    with pytest.raises(NativeLibraryError):
        model.query_one_vs_many(T([1]), T([1]), T([[2, 3]]))
    pop = PopTrackPredictor.__new__(PopTrackPredictor)
    with pytest.raises(ValueError, match=r'^mismatch shape: src: 0, dst: 0, ts: 1$'):
        pop.update(T([]), T([]), T([1]))
    with pytest.raises(NativeLibraryError):
        pop.update(T([1]), T([1]), T([7]))


def test_struct_mirror_has_the_library_s_size():
    from tgm_amd import _native

    lib = _native.load()
    assert lib.tgmx_abi_sizeof(21) == ctypes.sizeof(_native.TCoMem) == 88
    assert lib.tgmx_tcomem_state_bytes() == 16
    assert lib.tgmx_abi_sizeof(20) == ctypes.sizeof(_native.EdgeBank)  # the shared header moved code, not layouts
    assert lib.tgmx_version() == 7


def test_hash_mirror_against_the_kernel_s_constants():
    """the multipliers and shifts of eb_hash, and the key's packing, read from the kernel sources"""
    table = open(os.path.join(ROOT, 'tgm_amd', 'csrc', 'pairtable.h')).read()
    body = re.search(r'eb_hash\(unsigned long long x\) \{(.*?)\n\}', table, flags=re.S).group(1)
    assert [int(m, 16) for m in re.findall(r'0x[0-9A-Fa-f]+', body)] == [0xBF58476D1CE4E5B9, 0x94D049BB133111EB]
    assert [int(m) for m in re.findall(r'x >> (\d+)', body)] == [30, 27, 31]
    assert 'kEbEmpty = ~0ull' in table and tr.EMPTY_KEY == (1 << 64) - 1
    kernel = open(os.path.join(ROOT, 'tgm_amd', 'csrc', 'tcomem.hip')).read()
    assert 's < d ? ((unsigned long long)s << 32) | (unsigned long long)d : ((unsigned long long)d << 32) | (unsigned long long)s' in kernel
    assert tr.hash64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF and tr.hash64(1) == 0x5692161D100B05E5  # splitmix64's published outputs
    assert tr.pair_key(1, 2) == tr.pair_key(2, 1) == (1 << 32) | 2 and tr.pair_key(7, 7) == (7 << 32) | 7
    assert tr.pair_key(2**31 - 1, 2**31 - 1) != tr.EMPTY_KEY
    assert tr.home_slot(3, 9, 128) == tr.home_slot(9, 3, 128) == tr.hash64((3 << 32) | 9) & 127
    slots = [tr.home_slot(s, d, 128) for s in range(40) for d in range(s, 40)]
    assert len(set(slots)) == 128  # it spreads: every slot of a small table is some pair's home
