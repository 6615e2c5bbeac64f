#!/usr/bin/env python
"""Generate the decoder fixtures tests/golden/g26_decoder_*.npz by running the REFERENCE's ``LinkPredictor``, ``NodePredictor`` and
``GraphPredictor`` (tgm/nn/decoder/) with their merge / pooling operators (tgm/nn/modules/aggregation.py) on the host.

Runs only where the reference checkout is.  Every parameter is drawn here, uniform(-0.3, 0.3), inputs are standard normal.  Recorded as
plain .npz data:

    meta                kind ('link' | 'node' | 'graph'), kw (the constructor's arguments), op ('concat' | 'sum' | 'mean' | None), rows,
                        keys (the reference's state_dict keys, in its order, each prefixed 'p.')
    p.<state_dict key>  the parameters (float32)
    z_src, z_dst | z    the inputs (float32)
    out                 the reference's output

    python tests/golden/make_golden_decoders.py

The cases are tests/decoders_restate.py's CASES: the smallest shapes that reach each branch of the native head (widths that are and are
not multiples of the tiles, more rows than one block, one row, deep and wide last layers, both merges, both poolings, one node).  The
float32 restatement must reproduce every recorded output within 1e-5 of max(1, |ref|) before anything is written.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import decoders_restate as dr  # noqa: E402
from tgm.nn import GraphPredictor, LinkPredictor, NodePredictor  # noqa: E402
from tgm.nn.modules import ConcatMerge, LearnableSumMerge, MeanEmbdPooling, SumEmbdPooling  # noqa: E402


def fixture(name: str, seed: int) -> None:
    kind, kw, op, rows = dr.CASES[name]
    g = torch.Generator().manual_seed(seed)
    if kind == 'link':
        dim = kw['node_dim']
        model = LinkPredictor(**kw, merge_op=(ConcatMerge if op == 'concat' else LearnableSumMerge)(dim))
    elif kind == 'node':
        dim = kw['in_dim']
        model = NodePredictor(**kw)
    else:
        dim = kw['in_dim']
        model = GraphPredictor(**kw, graph_pooling=(MeanEmbdPooling if op == 'mean' else SumEmbdPooling)(dim))
    model.eval()
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.empty(p.shape).uniform_(-0.3, 0.3, generator=g))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in sd.items()} == dr.expected_keys(kind, kw, op), name
    inputs = {k: torch.randn(rows, dim, generator=g) for k in (('z_src', 'z_dst') if kind == 'link' else ('z',))}
    with torch.no_grad():
        out = model(*inputs.values())
    meta = dict(kind=kind, kw=kw, op=op, rows=rows, keys=[f'p.{k}' for k in sd])
    dr.close(dr.restate(meta, sd, inputs, torch.float32), out, name)
    dr.close(dr.restate(meta, sd, inputs).float(), out, name)
    path = os.path.join(HERE, f'g26_decoder_{name}.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), out=out.numpy(),
                        **{f'p.{k}': v.numpy() for k, v in sd.items()}, **{k: v.numpy() for k, v in inputs.items()})
    size = os.path.getsize(path)
    assert size < 400_000, (name, size)
    print(f'g26_decoder_{name}: {size} bytes, out {tuple(out.shape)}')


def main() -> None:
    for seed, name in enumerate(dr.EXPECTED_FIXTURES):
        fixture(name, 2600 + seed)


if __name__ == '__main__':
    torch.set_num_threads(1)
    main()
