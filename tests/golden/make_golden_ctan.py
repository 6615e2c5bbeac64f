#!/usr/bin/env python
"""Generate the CTANMemory fixtures tests/golden/g22_ctanmem_*.npz by running the REFERENCE.

Runs only where the reference checkout is.  It imports the reference's ``CTANMemory`` (tgm/nn/encoder/ctan.py) and ``LastAggregator``
(tgm/nn/encoder/tgn.py) with the PyG placeholder under tests/golden/_pyg_stub, drives them on the CPU through a scenario of
``update_state`` / ``reset_state`` operations and records plain .npz data:

    meta            num_nodes, memory_dim, init_time, ops: per operation 'update' or 'reset'
    src, dst, t     the events of all updates (int64), bounds [updates + 1]: update u offers [bounds[u], bounds[u + 1])
    src_emb{u}, dst_emb{u}   float32, the embeddings handed to update u (they may hold more rows than the update has events)
    memory [ops, N, M] float32, last_update [ops, N] int64   the reference's buffers after every operation

    python tests/golden/make_golden_ctan.py

The placeholder's ``ones`` initialiser does nothing, PyG's fills with 1: ``reset_state`` (``ones(last_update); last_update *= init_time``)
is run with PyG's.  Every scenario is also run through tests/ctan_restate.py, which must agree bit for bit.

  g22_ctanmem_basic            several calls over 12 nodes
  g22_ctanmem_f32_tie          times 1e9 + {1, 2, 3, 2}: equal as float32, so the first position wins while last_update is the int64 maximum
  g22_ctanmem_dup_in_batch     a node many times as source and destination, and a self-loop
  g22_ctanmem_rows_mismatch    embeddings with more rows than events (the evaluation loop's last one-vs-many query)
  g22_ctanmem_ooo              a later call with smaller times: plain overwrite
  g22_ctanmem_init_time_reset  init_time 77: updates, reset_state, updates
  g22_ctanmem_wiki_small       2 000 events, batches of 200, M 16
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('TGM_REFERENCE', os.path.join(os.path.dirname(REPO), 'reference'))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, '_pyg_stub'))
sys.path.insert(0, REFERENCE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import tgm.nn.encoder.ctan as ref_ctan  # noqa: E402
from tgm.nn.encoder.tgn import LastAggregator  # noqa: E402

import ctan_restate as cr  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

ref_ctan.ones = lambda tensor: tensor.data.fill_(1)  # torch_geometric.nn.inits.ones


def scenario(name: str, num_nodes: int, M: int, ops, init_time: int = 0, seed: int = 0, check=None) -> None:
    """ops: ('update', src, dst, t, extra_src_rows, extra_dst_rows) or ('reset',)"""
    rng = np.random.default_rng(seed)
    ref = ref_ctan.CTANMemory(num_nodes, M, aggr_module=LastAggregator(), init_time=init_time)
    ours = cr.CTANMemoryRestated(num_nodes, M, init_time)
    arrays, mem, lu, kinds, events = {}, [], [], [], []
    u = 0
    for op in ops:
        kinds.append(op[0])
        if op[0] == 'reset':
            ref.reset_state()
            ours.reset_state()
        else:
            _, s, d, t, xs, xd = op
            s, d, t = (np.asarray(v, dtype=np.int64) for v in (s, d, t))
            se = rng.standard_normal((len(s) + xs, M)).astype(np.float32)
            de = rng.standard_normal((len(s) + xd, M)).astype(np.float32)
            ref.update_state(torch.tensor(s), torch.tensor(d), torch.tensor(t), torch.tensor(se), torch.tensor(de))
            ours.update_state(s, d, t, se, de)
            arrays[f'src_emb{u}'], arrays[f'dst_emb{u}'] = se, de
            events.append((s, d, t))
            u += 1
        assert ref.memory.dtype == torch.float32 and ref.last_update.dtype == torch.int64
        assert np.array_equal(ref.memory.numpy(), ours.memory), (name, len(kinds), 'memory')
        assert np.array_equal(ref.last_update.numpy(), ours.last_update), (name, len(kinds), 'last_update')
        mem.append(ref.memory.numpy().copy())
        lu.append(ref.last_update.numpy().copy())
        if check:
            check(len(kinds) - 1, ref, arrays)
    cat = lambda i: np.concatenate([e[i] for e in events])
    bounds = np.cumsum([0] + [len(e[0]) for e in events]).astype(np.int64)
    meta = dict(num_nodes=num_nodes, memory_dim=M, init_time=init_time, ops=kinds)
    path = os.path.join(HERE, f'g22_ctanmem_{name}.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), src=cat(0), dst=cat(1), t=cat(2), bounds=bounds,
                        memory=np.stack(mem), last_update=np.stack(lu), **arrays)  # fmt: skip
    size = os.path.getsize(path)
    assert size < 400_000, (name, size)
    print(f'g22_ctanmem_{name}: {size} bytes, {len(kinds)} operations')


def up(s, d, t, xs=0, xd=0):
    return ('update', s, d, t, xs, xd)


def basic() -> None:
    rng = np.random.default_rng(2200)
    ops, lo = [], 0
    for n in (5, 1, 9, 16, 3):
        ops.append(up(rng.integers(0, 12, n), rng.integers(0, 12, n), np.sort(rng.integers(lo, lo + 50, n))))
        lo += 50
    scenario('basic', 12, 6, ops, seed=1)


def f32_tie() -> None:
    b = 1_000_000_000
    assert len({float(np.float32(b + i)) for i in (1, 2, 3)}) == 1  # equal as float32

    def check(i, ref, arrays):  # the issue's figures: node 1 gets the embedding of position 0 and last_update ...03
        assert np.array_equal(ref.memory[1].numpy(), arrays['src_emb0'][0]) and int(ref.last_update[1]) == b + 3
        assert np.array_equal(ref.memory[2].numpy(), arrays['src_emb0'][1]) and int(ref.last_update[2]) == b + 2

    scenario('f32_tie', 8, 4, [up([1, 2, 1, 4], [2, 3, 5, 1], [b + 1, b + 2, b + 3, b + 2])], seed=2, check=check)


def dup_in_batch() -> None:
    s = [3, 3, 0, 3, 5, 3, 2, 3, 3]
    d = [1, 3, 3, 4, 3, 3, 3, 0, 6]
    scenario('dup_in_batch', 7, 5, [up(s, d, [10, 11, 11, 12, 13, 13, 13, 14, 14]), up([3, 6], [3, 3], [20, 20])], seed=3)


def rows_mismatch() -> None:
    ops = [up([0, 1, 2, 3], [4, 5, 6, 0], [1, 2, 3, 4], xs=6, xd=6), up([1, 1], [2, 7], [5, 6], xs=3, xd=0), up([7], [7], [9], xs=0, xd=4)]
    scenario('rows_mismatch', 8, 4, ops, seed=4)


def ooo() -> None:
    ops = [up([0, 1, 2], [3, 4, 5], [100, 110, 120]), up([0, 4, 2], [1, 5, 2], [50, 40, 60]), up([5, 3], [0, 3], [45, 130])]
    scenario('ooo', 6, 3, ops, seed=5)


def init_time_reset() -> None:
    ops = [up([0, 1], [2, 3], [80, 90]), ('reset',), up([4, 1, 1], [0, 2, 4], [100, 95, 101]), ('reset',), ('reset',), up([5], [5], [78])]
    scenario('init_time_reset', 6, 4, ops, init_time=77, seed=6)


def wiki_small() -> None:
    s = make_stream('wiki', seed=2201, num_edges=2000, n_src=60, n_dst=40, edge_dim=0)
    src, dst, ts = s.src.numpy().astype(np.int64), s.dst.numpy().astype(np.int64), s.ts.numpy()
    scenario('wiki_small', 100, 16, [up(src[a : a + 200], dst[a : a + 200], ts[a : a + 200]) for a in range(0, 2000, 200)], seed=7)


if __name__ == '__main__':
    torch.set_num_threads(1)
    basic()
    f32_tie()
    dup_in_batch()
    rows_mismatch()
    ooo()
    init_time_reset()
    wiki_small()
