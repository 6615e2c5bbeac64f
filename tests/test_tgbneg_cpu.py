"""TGBNegativeEdgeSamplerHook, TGBTHGNegativeEdgeSamplerHook, TGBTKGNegativeEdgeSamplerHook on host tensors: the g33 fixtures recorded from the
reference's classes, the constructors' errors, the NegBatchList, the flattening the device table is built from."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tgbneg_cases as tc
from tgm_amd.hooks import (
    NegBatchList,
    TGBNegativeEdgeSamplerHook,
    TGBTHGNegativeEdgeSamplerHook,
    TGBTKGNegativeEdgeSamplerHook,
)
from tgm_amd.hooks.registry import list_hooks
from tgm_amd.hooks.tgb_sampler import flatten_eval_set, pad_rows

REPLAY = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'replay_reference_tgbneg.py')
NODE_TYPE = torch.arange(11, dtype=torch.int32)


def test_every_scenario_has_its_fixture():
    assert tc.FIXTURES == sorted(f'g33_tgbneg_{n}' for n in tc.EXPECTED)
    for name in tc.FIXTURES:
        assert os.path.getsize(os.path.join(tc.golden_util.GOLDEN_DIR, name + '.npz')) < 64 * 1024


@pytest.mark.parametrize('name', tc.FIXTURES)
def test_from_eval_set_against_fixture(name):
    """what the reference's class answered, reproduced exactly: neg, each list entry, neg_time, dtypes"""
    meta, ev, fields, _ = tc.load_fixture(name)
    hook = tc.hook_class(meta['cls']).from_eval_set(ev, split_mode=meta['split'])
    assert hook._key == tuple(meta['key'])  # the class's default order is the fixture's
    batch = tc.as_batch(fields)
    assert hook(tc.graph(), batch) is batch
    tc.check_fixture(name, batch)
    tc.check_answer(batch, ev, fields, tuple(meta['key']), name)


@pytest.mark.parametrize('name', tc.FIXTURES)
def test_reference_constructor_against_fixture(name):
    """the reference's constructor over the tgb package (the stand-in when it is not installed): host tensors go through query_batch"""
    tc.ensure_tgb()
    meta, ev, fields, _ = tc.load_fixture(name)
    kw = {'TGBTHGNegativeEdgeSamplerHook': dict(first_node_id=0, last_node_id=10, node_type=NODE_TYPE),
          'TGBTKGNegativeEdgeSamplerHook': dict(first_dst_id=0, last_dst_id=10)}.get(meta['cls'], {})  # fmt: skip
    prefix = tc.hook_class(meta['cls'])._dataset_prefix
    hook = tc.hook_class(meta['cls'])(f'{prefix}-foo', 'val', id='x', **kw)
    hook.neg_sampler.eval_set['val'] = ev
    batch = hook(tc.graph(), tc.as_batch(fields))
    tc.check_fixture(name, batch, suffix='_x')


def test_reference_test_files_in_place():
    """test_tgb_negative_sampling_hook.py and test_recipe.py of the reference, unedited, with ``tgm`` aliased to ``tgm_amd``"""
    r = subprocess.run([sys.executable, REPLAY], capture_output=True, text=True)
    if r.returncode == 77:
        pytest.skip('no reference checkout')
    print(r.stdout, r.stderr)
    assert r.returncode == 0


def test_surface():
    for cls, req in ((TGBNegativeEdgeSamplerHook, {'edge_src', 'edge_dst', 'edge_time'}),
                     (TGBTHGNegativeEdgeSamplerHook, {'edge_src', 'edge_dst', 'edge_time', 'edge_type'}),
                     (TGBTKGNegativeEdgeSamplerHook, {'edge_src', 'edge_dst', 'edge_time', 'edge_type'})):  # fmt: skip
        ev = tc.typed_set() if 'edge_type' in req else tc.uniform_set()
        h = cls.from_eval_set(ev)
        assert cls.has_state is False and h.requires == req and h.produces == {'neg', 'neg_batch_list', 'neg_time'}
        assert cls.from_eval_set(ev, id='foo').produces == {'neg_foo', 'neg_batch_list_foo', 'neg_time_foo'}
        assert 'foo' in repr(cls.from_eval_set(ev, id='foo')) and cls in list_hooks()
    import tgm_amd.hooks.negatives.tgb_sampler as m  # the reference's path

    assert m.TGBNegativeEdgeSamplerHook is TGBNegativeEdgeSamplerHook
    from tgm_amd.constants import METRIC_TGB_LINKPROPPRED, METRIC_TGB_NODEPROPPRED

    assert (METRIC_TGB_LINKPROPPRED, METRIC_TGB_NODEPROPPRED) == ('mrr', 'ndcg')


def test_neg_batch_list_is_a_list():
    ev = tc.ragged_set()
    fields = tc.batch_for(ev, [3, 12, 0, 3])
    batch = TGBNegativeEdgeSamplerHook.from_eval_set(ev)(tc.graph(), tc.as_batch(fields))
    lst = batch.neg_batch_list
    assert isinstance(lst, list) and isinstance(lst, NegBatchList) and len(lst) == 4
    assert [t.numel() for t in lst] == [4, 1000, 0, 4] == lst.lengths.tolist() and lst.uniform is None and lst.as_matrix() is None
    assert lst.matrix.shape == (4, 1000) and all(lst[b].data_ptr() == lst.matrix[b].data_ptr() for b in (0, 1, 3))  # views of the matrix
    assert torch.equal(torch.cat(lst), torch.cat(list(lst))) and lst[1:3][0] is lst[1]
    uni = TGBNegativeEdgeSamplerHook.from_eval_set(tc.uniform_set())
    ev = tc.uniform_set()
    lst = uni(tc.graph(), tc.as_batch(tc.batch_for(ev, [0, 1, 2]))).neg_batch_list
    assert lst.uniform == 20 and lst.as_matrix().shape == (3, 20)


def test_empty_batch():
    batch = tc.as_batch({f: np.zeros(0, dtype=np.int64) for f in ('src', 'dst', 'time', 'edge_type')})
    TGBNegativeEdgeSamplerHook.from_eval_set(tc.uniform_set())(tc.graph(), batch)
    assert batch.neg.dtype == torch.int32 and batch.neg.shape == (0,) and batch.neg_time.dtype == torch.int64 and batch.neg_time.shape == (0,)
    assert batch.neg_batch_list == []


def test_missing_key_names_the_first_position():
    ev = tc.uniform_set()
    fields = tc.batch_for(ev, [0, 1, 2, 3, 4])
    fields['dst'][3] += 1000
    fields['time'][1] += 5000
    hook = TGBNegativeEdgeSamplerHook.from_eval_set(ev)
    with pytest.raises(ValueError, match='`pip install --upgrade py-tgb`') as e:
        hook(tc.graph(), tc.as_batch(fields))
    assert str(e.value).startswith('TGBL Negative sampling failed for split_mode=val.')
    cause = e.value.__cause__
    assert isinstance(cause, ValueError) and 'batch position 1:' in str(cause) and f"time={fields['time'][1]}" in str(cause)
    good = tc.batch_for(ev, [4, 4, 0])
    tc.check_answer(hook(tc.graph(), tc.as_batch(good)), ev, good, what='after a missing key')


def test_constructor_errors():
    tc.ensure_tgb()
    for cls, kw in ((TGBNegativeEdgeSamplerHook, {}), (TGBTHGNegativeEdgeSamplerHook, dict(first_node_id=0, last_node_id=10, node_type=NODE_TYPE)),
                    (TGBTKGNegativeEdgeSamplerHook, dict(first_dst_id=0, last_dst_id=10))):  # fmt: skip
        good = cls._dataset_prefix + '-foo'
        with pytest.raises(ValueError, match='split_mode must be "val" or "test", got: invalid_mode'):
            cls(good, 'invalid_mode', **kw)
        for name in ('tgbn-trade', 'foo', 'tgbl-wiki' if cls._dataset_prefix != 'tgbl' else 'thgl-software'):
            with pytest.raises(ValueError, match=f'should only be registered for "{cls._dataset_prefix}-xxx" datasets, but got: {name}'):
                cls(name, 'val', **kw)
        with pytest.raises(ValueError, match='split_mode must be'):
            cls.from_eval_set(tc.typed_set() if kw else tc.uniform_set(), split_mode='train')
    thg = dict(first_node_id=0, last_node_id=10, node_type=NODE_TYPE)
    for bad, msg in ((dict(first_node_id=-1), 'First and last ID of node must be positive'), (dict(last_node_id=-1), 'First and last ID of node must be positive'),
                     (dict(last_node_id=100), 'last_node_id 100 must be within node_type'), (dict(node_type=None), 'Node type must not be None')):  # fmt: skip
        with pytest.raises(ValueError, match=msg):
            TGBTHGNegativeEdgeSamplerHook('thgl-software', 'val', **{**thg, **bad})
        with pytest.raises(ValueError, match=msg):
            TGBTHGNegativeEdgeSamplerHook.from_eval_set(tc.typed_set(), **{**thg, **bad})
    for bad in (dict(first_dst_id=-1, last_dst_id=10), dict(first_dst_id=0, last_dst_id=-1)):
        with pytest.raises(ValueError, match='First and last ID of node must be positive'):
            TGBTKGNegativeEdgeSamplerHook('tkgl-smallpedia', 'val', **bad)
    with pytest.raises(ValueError, match='key must name'):
        TGBNegativeEdgeSamplerHook.from_eval_set(tc.uniform_set(), key=('src', 'src', 'time'))
    with pytest.raises(ValueError, match="does not require 'edge_type'"):
        TGBNegativeEdgeSamplerHook.from_eval_set(tc.typed_set(), key=tc.KEY_TYPED)
    for bad_set in ({}, {(1, 2): np.arange(3)}, {(1, 2, 3): np.array([0.5])}, {(1, 2, 3): np.array([-1])}, {'a': np.arange(3)}, [1, 2]):
        with pytest.raises(ValueError, match='eval_set must be a non-empty dict'):
            TGBNegativeEdgeSamplerHook.from_eval_set(bad_set)


def test_import_error_without_tgb():
    """in a process of its own: no tgb package (an installed one is hidden) and the stand-in not on the path"""
    code = ('import sys\n'
            'assert not any(p.endswith("_tgb_stub") for p in sys.path)\n'
            'sys.modules["tgb"] = None  # an installed py-tgb is hidden: importing it raises ImportError\n'
            'import torch\n'
            'from tgm_amd.hooks import TGBNegativeEdgeSamplerHook as A, TGBTHGNegativeEdgeSamplerHook as B, TGBTKGNegativeEdgeSamplerHook as C\n'
            'for cls, name, kw in ((A, "tgbl-wiki", {}), (B, "thgl-software", dict(first_node_id=0, last_node_id=3, node_type=torch.arange(4))),\n'
            '                      (C, "tkgl-smallpedia", dict(first_dst_id=0, last_dst_id=3))):\n'
            '    try:\n'
            '        cls(name, "val", **kw)\n'
            '    except ImportError as e:\n'
            '        assert str(e) == f"TGB required for {cls.__name__}, try `pip install py-tgb`", e\n'
            '    else:\n'
            '        sys.exit(1)\n')  # fmt: skip
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr


def test_flatten_eval_set_layout():
    ev = tc.ragged_set()
    flat = flatten_eval_set(ev, 3)
    P = len(ev)
    assert flat['keys'].shape == (P, 4) and flat['keys'].dtype == np.int64 and (flat['keys'][:, 3] == 0).all()
    assert flat['indptr'].dtype == np.int64 and (flat['indptr'] % 4 == 0).all() and flat['pool'].dtype == np.int32 and flat['qpad'] == 1000
    for p, (k, v) in enumerate(ev.items()):
        lo = flat['indptr'][p]
        assert tuple(flat['keys'][p, :3]) == k and flat['rowlen'][p] == len(v) and np.array_equal(flat['pool'][lo : lo + len(v)], v)
        assert (flat['pool'][lo + len(v) : flat['indptr'][p + 1]] == -1).all()
    assert flat['max_id'] == max(int(v.max()) for v in ev.values() if len(v))
    assert flatten_eval_set({'cool'}, 3) is None and flatten_eval_set({(1, 2, 3): [[1]]}, 3) is None and flatten_eval_set(None, 3) is None
    assert flatten_eval_set({(1, 2, 3): np.array([(1 << 31) - 1])}, 3) is None
    m, lens = pad_rows([[0], [], [5, 6, 7, 8, 9]])
    assert m.shape == (3, 8) and lens.tolist() == [1, 0, 5] and m[2].tolist() == [5, 6, 7, 8, 9, -1, -1, -1]


def test_sampler_that_is_no_lookup_is_asked_every_time():
    """host tensors with a sampler object always go through query_batch (a Mock's eval_set is no dict of arrays)"""
    tc.ensure_tgb()
    hook = TGBNegativeEdgeSamplerHook('tgbl-foo', 'test')
    hook.neg_sampler.eval_set['test'] = {'cool'}
    hook.neg_sampler.query_batch = lambda s, d, t, split_mode: [[7, 3], [3]] if split_mode == 'test' else None
    fields = dict(src=np.array([1, 2]), dst=np.array([3, 4]), time=np.array([10, 20]), edge_type=np.zeros(2, dtype=np.int64))
    batch = hook(tc.graph(), tc.as_batch(fields))
    assert batch.neg.tolist() == [3, 7] and [t.tolist() for t in batch.neg_batch_list] == [[7, 3], [3]]
    assert torch.equal(batch.neg_time, tc.reference_neg_time(fields, 2))
