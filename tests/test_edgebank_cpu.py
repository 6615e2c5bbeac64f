"""EdgeBankPredictor without a device: the reference's argument checks (types, messages, order), the refusal of CPU tensors, the dictionary
restatement against every g19 fixture, the argument struct's size, the table's growth rule and the hash mirror."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import edgebank_restate as er
from golden_util import GOLDEN_DIR, load

FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, 'g19_edgebank_*.npz')))
EXPECTED = ['unlimited_late_insert', 'unlimited_late_insert_p07', 'fixed_window', 'fixed_window_p07', 'eviction', 'ooo_fixed', 'ooo_unlimited',
            'wiki_small_unlimited', 'wiki_small_fixed', 'epoch_f32', 'last_arrival', 'stale_unlimited', 'pos_prob_07']  # fmt: skip


def calls_of(meta, a):
    """[(src, dst, ts)] per call, as int64 numpy"""
    b = a['bounds']
    return [(a['src'][b[c] : b[c + 1]], a['dst'][b[c] : b[c + 1]], a['ts'][b[c] : b[c + 1]]) for c in range(meta['calls'])]


def queries_of(meta, a, c):
    """[(src, dst, pred, dtype name, rows)] asked after call c"""
    return [(a[f'q{c}_{j}_src'], a[f'q{c}_{j}_dst'], a[f'q{c}_{j}_pred'], m['dtype'], m['rows']) for j, m in enumerate(meta['queries'][c])]


def test_every_scenario_has_its_fixture():
    assert FIXTURES == sorted('g19_edgebank_' + n for n in EXPECTED)
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, name + '.npz')) < 200_000


@pytest.mark.parametrize('name', ['g19_edgebank_' + n for n in EXPECTED])
def test_restatement_reproduces_the_fixture(name):
    meta, a = load(name)
    bank = None
    for c, (s, d, t) in enumerate(calls_of(meta, a)):
        if bank is None:
            bank = er.EdgeBankRestated(s, d, t, meta['memory_mode'], meta['window_ratio'], meta['pos_prob'])
        else:
            bank.update(s, d, t)
        assert bank.window_start == a['window_start'][c] and bank.window_end == a['window_end'][c]
        keys, ts = bank.memory_arrays()
        assert np.array_equal(keys, a[f'mem{c}_keys']) and np.array_equal(ts, a[f'mem{c}_ts'])
        for qs, qd, pred, dtype, _ in queries_of(meta, a, c):
            got = bank(qs.astype(dtype), qd.astype(dtype))
            assert got.dtype == pred.dtype and np.array_equal(got, pred)


def test_fixtures_pin_the_kept_behaviours():
    # float32 window arithmetic: the issue's example, and the fixture's first window
    bank = er.EdgeBankRestated([0, 1], [1, 2], [1_600_000_000, 1_600_001_000], 'fixed', 0.15)
    assert bank.size == 128 and bank.window_start == 1_600_000_896
    _, a = load('g19_edgebank_epoch_f32')
    assert a['window_start'][0] == 1_600_000_896
    # the last arrival, not the largest timestamp
    assert er.EdgeBankRestated([1, 1], [2, 2], [10, 5], 'fixed', 1.0).memory == {(1, 2): 5}
    _, a = load('g19_edgebank_last_arrival')
    assert a['mem0_keys'].tolist() == [[1, 2], [3, 4]] and a['mem0_ts'].tolist() == [5, 10] and a['mem1_ts'].tolist() == [5, 7]
    # unlimited mode drops what is older than the window start
    _, a = load('g19_edgebank_stale_unlimited')
    assert [5, 5] not in a['mem1_keys'].tolist() and [8, 8] in a['mem1_keys'].tolist()
    # integer queries with pos_prob = 0.7 answer zeros, float queries 0.7
    meta, a = load('g19_edgebank_pos_prob_07')
    (_, _, p64, *_), (_, _, p32, *_), (_, _, pf, *_) = queries_of(meta, a, 1)
    assert p64.dtype == np.int64 and not p64.any() and p32.dtype == np.int32 and not p32.any()
    assert pf.dtype == np.float32 and set(np.unique(pf).tolist()) == {0.0, float(np.float32(0.7))}


# ---- the product's surface, as far as it goes without a device ---------------------------------------------------------------------------
T = torch.Tensor


def test_constructor_argument_checks_carry_the_reference_s_messages():
    from tgm_amd.nn import EdgeBankPredictor

    src, dst, ts = T([2, 10]), T([3, 20]), T([1, 5])
    with pytest.raises(ValueError, match=r'^memory_mode must be "unlimited" or "fixed"$'):
        EdgeBankPredictor(src, dst, ts, memory_mode='foo')
    for ratio in (0, -0.1, 1.5):
        with pytest.raises(ValueError, match=r'^Window ratio must be in \(0, 1\]$'):
            EdgeBankPredictor(src, dst, ts, window_ratio=ratio)
    with pytest.raises(TypeError, match=r"^src, dst, ts must all be Tensor, got src: <class 'int'>, dst: <class 'int'>, ts: <class 'int'>$"):
        EdgeBankPredictor(1, 2, 3)
    with pytest.raises(TypeError, match='must all be Tensor, got src: <class \'torch.Tensor\'>, dst: <class \'list\'>'):
        EdgeBankPredictor(src, [3, 20], ts)
    with pytest.raises(ValueError, match=r'^mismatch shape: src: 2, dst: 2, ts: 1$'):
        EdgeBankPredictor(src, dst, T([1]))
    with pytest.raises(ValueError, match=r'^src, dst, ts must have at len > 1, got src: 0, dst: 0, ts: 0$'):
        EdgeBankPredictor(T([]), T([]), T([]))
    # the reference's order: the mode, the ratio, then the data
    with pytest.raises(ValueError, match='memory_mode'):
        EdgeBankPredictor(1, 2, 3, memory_mode='foo', window_ratio=0)
    with pytest.raises(ValueError, match='Window ratio'):
        EdgeBankPredictor(1, 2, 3, window_ratio=0)


def test_cpu_tensors_are_refused_after_the_argument_checks():
    from tgm_amd.exceptions import NativeLibraryError
    from tgm_amd.nn import EdgeBankPredictor
    from tgm_amd.nn.modules import EdgeBankPredictor as by_module_path
    from tgm_amd.nn.modules.edgebank import EdgeBankPredictor as by_file_path

    assert EdgeBankPredictor is by_module_path is by_file_path
    for mode in ('unlimited', 'fixed'):
        with pytest.raises(NativeLibraryError):
            EdgeBankPredictor(T([2, 10]), T([3, 20]), T([1, 5]), memory_mode=mode)
    with pytest.raises(NativeLibraryError):
        EdgeBankPredictor(torch.tensor([2, 10]), torch.tensor([3, 20]), torch.tensor([1, 5]), capacity=64)


def test_update_argument_checks_run_before_the_device_is_touched():
    """update() on an object that never reached the device: the checks answer first, then the refusal of CPU tensors"""
    from tgm_amd.exceptions import NativeLibraryError
    from tgm_amd.nn import EdgeBankPredictor

    bank = EdgeBankPredictor.__new__(EdgeBankPredictor)
    with pytest.raises(TypeError, match=r"^src, dst, ts must all be Tensor, got src: <class 'torch.Tensor'>, dst: <class 'NoneType'>, ts: <class 'int'>$"):
        bank.update(T([1]), None, 3)
    with pytest.raises(ValueError, match=r'^mismatch shape: src: 0, dst: 0, ts: 1$'):
        bank.update(T([]), T([]), T([1]))
    with pytest.raises(ValueError, match=r'^src, dst, ts must have at len > 1, got src: 0, dst: 0, ts: 0$'):
        bank.update(T([]), T([]), T([]))
    with pytest.raises(NativeLibraryError):
        bank.update(T([1]), T([1]), T([7]))
    with pytest.raises(NativeLibraryError):
        bank(T([1]), T([1]))
    with pytest.raises(NativeLibraryError):
        bank.query_one_vs_many(T([1]), T([1]), T([[2, 3]]))


def test_struct_mirror_has_the_library_s_size():
    from tgm_amd import _native

    lib = _native.load()
    assert lib.tgmx_abi_sizeof(20) == ctypes.sizeof(_native.EdgeBank) == 64
    assert lib.tgmx_edgebank_state_bytes() == 32
    assert lib.tgmx_version() == 7


# (capacity, offered since the last rehash, kept by it, incoming) -> capacity, by hand: the least power of two >= 2 (offered + kept + incoming),
# or the capacity as it is when that already holds
GROWTH = [
    ((0, 0, 0, 1), 2),
    ((0, 0, 0, 3), 8),
    ((0, 0, 0, 1000), 2048),
    ((0, 0, 0, 1024), 2048),
    ((0, 0, 0, 1025), 4096),
    ((8, 3, 0, 1), 8),       # 2 * 4 = 8: exactly half full is allowed
    ((8, 3, 0, 2), 16),      # 2 * 5 = 10
    ((8, 4, 0, 200), 512),   # 2 * 204 = 408
    ((16, 0, 5, 3), 16),     # after a rehash that kept 5: 2 * 8 = 16
    ((16, 0, 5, 4), 32),
    ((4096, 1000, 900, 148), 4096),  # 2 * 2048
    ((4096, 1000, 900, 149), 8192),
    ((1 << 20, 0, 0, 200), 1 << 20),
]


@pytest.mark.parametrize('args,expected', GROWTH)
def test_growth_rule(args, expected):
    from tgm_amd.nn.edgebank import grow_capacity

    capacity, offered, kept, incoming = args
    got = grow_capacity(*args)
    assert got == expected
    assert got & (got - 1) == 0 and got >= capacity
    assert 2 * (offered + kept + incoming) <= got  # the load stays at or below 0.5 whatever the events turn out to be


def test_growth_rule_over_a_run():
    """A stream of batches, every event a new pair and every rehash keeping all: the entries never pass half the capacity"""
    from tgm_amd.nn.edgebank import grow_capacity

    capacity, offered, kept = 8, 0, 0
    for n in [3, 1, 1, 200, 200, 1025, 7, 5000, 200]:
        new = grow_capacity(capacity, offered, kept, n)
        if new != capacity:
            assert new >= 2 * capacity
            capacity, kept, offered = new, kept + offered, 0
        offered += n
        assert kept + offered <= capacity // 2 and capacity & (capacity - 1) == 0


def test_hash_mirror():
    # splitmix64's finaliser: 0 is its fixed point, and the generator's published first output for seed 0 is the finaliser of its increment
    assert er.hash64(0) == 0
    assert er.hash64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert er.hash64(1) == 0x5692161D100B05E5
    assert er.pack_key(1, 2) == (1 << 32) | 2 and er.pack_key(2**31 - 1, 2**31 - 1) != er.EMPTY_KEY
    slots = [er.home_slot(s, d, 128) for s in range(40) for d in range(40)]
    assert min(slots) == 0 and max(slots) == 127 and len(set(slots)) == 128  # it spreads: every slot of a small table is some pair's home
