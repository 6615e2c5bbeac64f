#!/usr/bin/env python
"""Generate the TGB negative-sampler fixtures tests/golden/g33_tgbneg_*.npz by running the REFERENCE.

Runs only where the reference checkout is.  It imports the reference's ``TGBNegativeEdgeSamplerHook``, ``TGBTHGNegativeEdgeSamplerHook`` and
``TGBTKGNegativeEdgeSamplerHook`` (tgm/hooks/negatives/tgb_sampler.py), constructs each through its own constructor over the ``tgb``
package -- the stand-in under tests/golden/_tgb_stub when the real one is not installed --, hands its sampler an evaluation set of
tests/tgbneg_cases.py, calls the hook on one CPU batch and records plain .npz data:

    meta                    cls, key (the batch fields in the key tuples' order), split, neg_dtype / list_dtype / neg_time_dtype (the reference's)
    batch_src, batch_dst, batch_time, batch_edge_type     the batch (int64)
    keys [P, arity], row_off [P + 1], row_val             the evaluation set, flattened
    neg                     batch.neg
    list_len [B], list_val  batch.neg_batch_list, end to end
    neg_time                batch.neg_time (torch's CPU generator seeded 0)

    python tests/golden/make_golden_tgbneg.py

  g33_tgbneg_ragged      rows of 0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 999 and 1000 negatives, asked in another order, two of them twice
  g33_tgbneg_uniform     40 keys x 20 negatives, a batch of 25
  g33_tgbneg_wide_keys   keys that differ in one field, time 0, times >= 2^40, ids up to 2^31 - 2
  g33_tgbneg_thgl        (time, source, edge type) keys through the thgl class
  g33_tgbneg_tkgl        the same through the tkgl class
"""
from __future__ import annotations

import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('TGM_REFERENCE', os.path.join(os.path.dirname(REPO), 'reference'))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, '_pyg_stub'))
sys.path.insert(0, REFERENCE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tgbneg_cases as cases  # noqa: E402

cases.ensure_tgb()
from tgm.hooks.negatives import tgb_sampler as ref  # noqa: E402


def record(name: str, cls_name: str, ev: dict, fields: dict, key, **ctor) -> None:
    prefix = {'TGBNegativeEdgeSamplerHook': 'tgbl', 'TGBTHGNegativeEdgeSamplerHook': 'thgl', 'TGBTKGNegativeEdgeSamplerHook': 'tkgl'}[cls_name]
    hook = getattr(ref, cls_name)(f'{prefix}-foo', 'val', **ctor)
    hook.neg_sampler.eval_set['val'] = ev
    batch = cases.as_batch(fields)
    hook(types.SimpleNamespace(device=torch.device('cpu')), batch)
    rows, want = cases.expected(ev, fields, key)
    assert np.array_equal(batch.neg.numpy(), want)  # the definition the tests restate is the reference's
    for r, got in zip(rows, batch.neg_batch_list):
        assert np.array_equal(got.numpy(), r)
    keys = np.array(list(ev), dtype=np.int64).reshape(len(ev), len(key))
    lens = np.array([len(v) for v in ev.values()], dtype=np.int64)
    meta = dict(cls=cls_name, key=list(key), split='val', neg_dtype=str(batch.neg.dtype), list_dtype=str(batch.neg_batch_list[0].dtype),
                neg_time_dtype=str(batch.neg_time.dtype))  # fmt: skip
    arrays = dict(
        meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
        keys=keys, row_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), row_val=np.concatenate(list(ev.values())).astype(np.int32),
        neg=batch.neg.numpy(), list_len=np.array([t.numel() for t in batch.neg_batch_list], dtype=np.int64),
        list_val=torch.cat(batch.neg_batch_list).numpy(), neg_time=batch.neg_time.numpy(),
        **{'batch_' + f: np.asarray(v, dtype=np.int64) for f, v in fields.items()},
    )  # fmt: skip
    path = os.path.join(HERE, f'g33_tgbneg_{name}.npz')
    np.savez_compressed(path, **arrays)
    print(f'{path}: {os.path.getsize(path)} bytes, P = {len(ev)}, B = {len(fields["src"])}, unique = {batch.neg.numel()}')


def main() -> None:
    ev = cases.ragged_set()
    order = [12, 0, 5, 11, 3, 7, 1, 12, 9, 2, 10, 4, 6, 8, 5]
    record('ragged', 'TGBNegativeEdgeSamplerHook', ev, cases.batch_for(ev, order), cases.KEY_TGBL)
    ev = cases.uniform_set()
    record('uniform', 'TGBNegativeEdgeSamplerHook', ev, cases.batch_for(ev, list(np.random.default_rng(1).integers(0, 40, 25))), cases.KEY_TGBL)
    ev = cases.wide_key_set()
    record('wide_keys', 'TGBNegativeEdgeSamplerHook', ev, cases.batch_for(ev, list(range(len(ev) - 1, -1, -1)) + [0, 0]), cases.KEY_TGBL)
    ev = cases.typed_set()
    order = list(np.random.default_rng(2).integers(0, len(ev), 20))
    node_type = torch.arange(201, dtype=torch.int32)
    record('thgl', 'TGBTHGNegativeEdgeSamplerHook', ev, cases.batch_for(ev, order, cases.KEY_TYPED), cases.KEY_TYPED, first_node_id=0, last_node_id=200,
           node_type=node_type)  # fmt: skip
    record('tkgl', 'TGBTKGNegativeEdgeSamplerHook', ev, cases.batch_for(ev, order[::-1], cases.KEY_TYPED), cases.KEY_TYPED, first_dst_id=0, last_dst_id=200)


if __name__ == '__main__':
    main()
