"""Shared by tests/test_tgbneg_cpu.py, tests/test_tgbneg_gpu.py and tests/golden/make_golden_tgbneg.py: evaluation sets as plain dicts, the
batches asked of them, the g33 fixtures, and the comparison of two answers.  An evaluation set here maps a tuple of Python integers (in the
hook's key order) to an int64 array of negative destinations; a batch is a dict of int64 arrays ``src, dst, time, edge_type``."""
from __future__ import annotations

import glob
import importlib
import os
import sys
import types

import numpy as np
import torch

import golden_util

STUB = os.path.join(golden_util.GOLDEN_DIR, '_tgb_stub')
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(golden_util.GOLDEN_DIR, 'g33_tgbneg_*.npz')))
EXPECTED = ['ragged', 'uniform', 'wide_keys', 'thgl', 'tkgl']
KEY_TGBL = ('src', 'dst', 'time')
KEY_TYPED = ('time', 'src', 'edge_type')
# every row length at which the copy takes another number of 16-byte vectors, trips or lanes
RAGGED_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 999, 1000)
FIELD_OF = {'src': 'src', 'dst': 'dst', 'time': 'time', 'edge_type': 'edge_type'}


def ensure_tgb() -> bool:
    """Make ``import tgb`` work: the installed package, else the stand-in under tests/golden/_tgb_stub.  True when the stand-in is used."""
    try:
        importlib.import_module('tgb.utils.info')
        return STUB in sys.path
    except ImportError:
        sys.path.insert(0, STUB)
        importlib.invalidate_caches()
        importlib.import_module('tgb.utils.info')
        return True


# ---- evaluation sets ----------------------------------------------------------------------------------------------------------------------


def ragged_set(lengths=RAGGED_LENGTHS, seed=33, num_ids=1500, key=KEY_TGBL):
    """One key per length, negatives drawn without replacement from [0, num_ids) where they fit (so rows overlap), sorted as TGB stores them."""
    rng = np.random.default_rng(seed)
    ev = {}
    for i, n in enumerate(lengths):
        k = tuple(int(x) for x in (10 + i, 500 + 7 * i, 1000 + 3 * i)[: len(key)])
        ev[k] = np.sort(rng.choice(max(num_ids, n), n, replace=False)).astype(np.int64)
    return ev


def uniform_set(P=40, Q=20, seed=34, num_ids=300, key=KEY_TGBL, time0=0):
    rng = np.random.default_rng(seed)
    ev = {}
    while len(ev) < P:
        k = (int(rng.integers(0, 50)), int(rng.integers(0, 50)), time0 + int(rng.integers(0, 1000)))[: len(key)]
        ev[tuple(k)] = np.sort(rng.choice(num_ids, Q, replace=False)).astype(np.int64)
    return ev


def wide_key_set(seed=35):
    """Keys that differ in exactly one field (each field in turn), time 0, times >= 2^40, ids up to 2^31 - 2; rows of different ids each."""
    rng = np.random.default_rng(seed)
    big_t, big_id = 1 << 40, (1 << 31) - 2
    keys = [(5, 6, 7), (4, 6, 7), (5, 9, 7), (5, 6, 8), (5, 6, 0), (0, 0, 0), (big_id, 6, 7), (5, big_id, 7), (big_id, big_id, big_t),
            (5, 6, big_t), (5, 6, big_t + 1), (5, 6, (1 << 62) + 3), (6, 5, 7), (7, 6, 5)]  # fmt: skip
    return {k: np.sort(rng.choice(4096, 3 + i, replace=False)).astype(np.int64) for i, k in enumerate(keys)}


def typed_set(seed=36, P=30):
    """(time, src, edge_type) keys, as the thgl / tkgl samplers are believed to hold them; some keys differ only in the edge type."""
    rng = np.random.default_rng(seed)
    ev = {}
    while len(ev) < P:
        t, s = int(rng.integers(0, 40)), int(rng.integers(0, 25))
        for e in range(int(rng.integers(1, 4))):
            ev[(t, s, e)] = np.sort(rng.choice(200, int(rng.integers(0, 12)), replace=False)).astype(np.int64)
    return ev


def batch_for(ev, order, key=KEY_TGBL, seed=0):
    """The positives ``order`` (indices into the set's keys, repeats allowed) as a batch; fields the key does not hold are arbitrary."""
    keys = list(ev)
    rng = np.random.default_rng(seed)
    out = {f: rng.integers(0, 100, len(order)).astype(np.int64) for f in ('src', 'dst', 'time', 'edge_type')}
    for j, f in enumerate(key):
        out[f] = np.array([keys[i][j] for i in order], dtype=np.int64)
    return out


def as_batch(fields, device='cpu', dtypes=None):
    """The batch object a hook reads; dtypes: field -> torch dtype (default int32 ids and edge types where they fit, int64 times)."""
    dtypes = dict(dtypes or {})
    ns = types.SimpleNamespace()
    for f, attr in (('src', 'edge_src'), ('dst', 'edge_dst'), ('time', 'edge_time'), ('edge_type', 'edge_type')):
        v = np.asarray(fields[f], dtype=np.int64)
        dt = dtypes.get(f, torch.int64 if f == 'time' or (v.size and v.max() >= 1 << 31) else torch.int32)
        setattr(ns, attr, torch.from_numpy(v).to(dt).to(device))
    return ns


def graph(device='cpu'):
    return types.SimpleNamespace(device=torch.device(device))


def expected(ev, fields, key=KEY_TGBL):
    """The definition, from the dict: per-position rows, their sorted unique union."""
    rows = [np.asarray(ev[tuple(int(fields[f][b]) for f in key)], dtype=np.int64) for b in range(len(fields['src']))]
    neg = np.unique(np.concatenate(rows)) if rows and sum(r.size for r in rows) else np.zeros(0, dtype=np.int64)
    return rows, neg.astype(np.int32)


def reference_neg_time(fields, n, device='cpu'):
    """The reference's expression, evaluated on ``device``."""
    t = np.asarray(fields['time'])
    gen = torch.Generator(device=device)
    gen.manual_seed(0)
    return torch.randint(int(t.min()), int(t.max()) + 1, (n,), device=device, generator=gen)


def check_answer(batch, ev, fields, key=KEY_TGBL, what='', suffix=''):
    """Everything a call produces against the definition: dtypes, neg, every list entry, the matrix / lengths / uniform, neg_time."""
    from tgm_amd.hooks import NegBatchList

    neg, lst, neg_time = (getattr(batch, a + suffix) for a in ('neg', 'neg_batch_list', 'neg_time'))
    rows, want = expected(ev, fields, key)
    assert neg.dtype == torch.int32 and np.array_equal(neg.cpu().numpy(), want), f'{what}: neg'
    assert isinstance(lst, list) and type(lst) is NegBatchList and len(lst) == len(rows), f'{what}: list'
    for b, r in enumerate(rows):
        assert lst[b].dtype == torch.int32 and lst[b].device == neg.device and np.array_equal(lst[b].cpu().numpy(), r), f'{what}: row {b}'
    lens = [r.size for r in rows]
    m = lst.matrix.cpu().numpy()
    assert lst.matrix.dtype == torch.int32 and m.shape[0] == len(rows) and m.shape[1] % 4 == 0 and m.shape[1] >= max(lens + [1]), f'{what}: matrix shape'
    assert lst.lengths.dtype == torch.int32 and lst.lengths.device == neg.device and lst.lengths.cpu().tolist() == lens, f'{what}: lengths'
    for b, r in enumerate(rows):
        assert np.array_equal(m[b, : r.size], r) and (m[b, r.size :] == -1).all(), f'{what}: matrix row {b}'
    assert lst.uniform == (lens[0] if len(set(lens)) == 1 else None), f'{what}: uniform'
    if lst.uniform is not None:
        assert torch.equal(lst.as_matrix().cpu(), torch.stack([t.cpu() for t in lst])), f'{what}: as_matrix'
    want_t = reference_neg_time(fields, len(want), neg.device)
    assert neg_time.dtype == torch.int64 and neg_time.shape == neg.shape and torch.equal(neg_time, want_t), f'{what}: neg_time'


def same_answer(a, b, what=''):
    """Two batches answered alike, bit for bit (device against host, run against run)."""
    assert a.neg.dtype == b.neg.dtype and torch.equal(a.neg.cpu(), b.neg.cpu()), f'{what}: neg'
    assert len(a.neg_batch_list) == len(b.neg_batch_list), f'{what}: list length'
    for i, (x, y) in enumerate(zip(a.neg_batch_list, b.neg_batch_list)):
        assert x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu()), f'{what}: row {i}'
    assert torch.equal(a.neg_batch_list.matrix.cpu(), b.neg_batch_list.matrix.cpu()), f'{what}: matrix'
    assert torch.equal(a.neg_batch_list.lengths.cpu(), b.neg_batch_list.lengths.cpu()) and a.neg_batch_list.uniform == b.neg_batch_list.uniform, f'{what}: lengths'


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------------------


def hook_class(name: str):
    import tgm_amd.hooks as hooks

    return getattr(hooks, name)


def load_fixture(name: str):
    """-> meta, the evaluation set (dict), the batch fields, the arrays the reference produced"""
    meta, a = golden_util.load(name)
    arity = len(meta['key'])
    ev = {tuple(int(x) for x in a['keys'][p, :arity]): a['row_val'][a['row_off'][p] : a['row_off'][p + 1]].astype(np.int64) for p in range(len(a['keys']))}
    fields = {f: a['batch_' + f] for f in ('src', 'dst', 'time', 'edge_type')}
    return meta, ev, fields, a


def check_fixture(name: str, batch, suffix=''):
    """The answer against what the reference's class gave for the same batch: neg, each list entry, dtypes; neg_time on the CPU generator."""
    meta, ev, fields, a = load_fixture(name)
    neg, lst, neg_time = (getattr(batch, x + suffix) for x in ('neg', 'neg_batch_list', 'neg_time'))
    assert str(neg.dtype) == meta['neg_dtype'] and np.array_equal(neg.cpu().numpy(), a['neg']), f'{name}: neg'
    assert len(lst) == len(a['list_len']), name
    off = np.concatenate([[0], np.cumsum(a['list_len'])])
    for b in range(len(lst)):
        assert str(lst[b].dtype) == meta['list_dtype'] and np.array_equal(lst[b].cpu().numpy(), a['list_val'][off[b] : off[b + 1]]), f'{name}: row {b}'
    assert str(neg_time.dtype) == meta['neg_time_dtype'] and neg_time.shape == neg.shape, f'{name}: neg_time dtype / shape'
    if neg_time.device.type == 'cpu':
        assert np.array_equal(neg_time.numpy(), a['neg_time']), f'{name}: neg_time'
