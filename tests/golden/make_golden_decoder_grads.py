#!/usr/bin/env python
"""Generate the decoder gradient fixtures tests/golden/g30_decoder_grad_*.npz by running the REFERENCE's ``LinkPredictor`` and
``NodePredictor`` (tgm/nn/decoder/) under float32 autograd on the host.

Runs only where the reference checkout is.  Every parameter is drawn here, uniform(-0.3, 0.3); inputs and the upstream gradient are
standard normal.  Recorded as plain .npz data:

    meta                kind ('link' | 'node'), kw (the constructor's arguments), op ('concat' | 'sum' | None), rows, keys (the reference's
                        state_dict keys, in its order, each prefixed 'p.')
    p.<state_dict key>  the parameters (float32)
    z_src, z_dst | z    the inputs (float32)
    dout                the upstream gradient, the shape of the reference's output
    g.<name>            the reference's float32 gradient of every input and of every parameter (``out.backward(dout)``)

    python tests/golden/make_golden_decoder_grads.py

The cases are tests/decoders_bwd_restate.py's GRAD_CASES.  The float64 restatement of the gradients must agree with every recorded one
within 1e-5 of max(1, |ref|) before anything is written.
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

import decoders_bwd_restate as br  # noqa: E402
import decoders_restate as dr  # noqa: E402
from tgm.nn import LinkPredictor, NodePredictor  # noqa: E402
from tgm.nn.modules import ConcatMerge, LearnableSumMerge  # noqa: E402


def fixture(name: str, seed: int) -> None:
    kind, kw, op, rows = br.GRAD_CASES[name]
    g = torch.Generator().manual_seed(seed)
    if kind == 'link':
        dim = kw['node_dim']
        model = LinkPredictor(**kw, merge_op=(ConcatMerge if op == 'concat' else LearnableSumMerge)(dim))
    else:
        dim = kw['in_dim']
        model = NodePredictor(**kw)
    model.train()
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.empty(p.shape).uniform_(-0.3, 0.3, generator=g))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in sd.items()} == dr.expected_keys(kind, kw, op), name
    inputs = {k: torch.randn(rows, dim, generator=g).requires_grad_() for k in (('z_src', 'z_dst') if kind == 'link' else ('z',))}
    out = model(*inputs.values())
    dout = torch.randn(out.shape, generator=g)
    out.backward(dout)
    grads = {k: v.grad.detach().clone() for k, v in inputs.items()}
    grads.update({k: p.grad.detach().clone() for k, p in model.named_parameters()})
    assert set(grads) == set(sd) | set(inputs), name
    plain = {k: v.detach() for k, v in inputs.items()}
    for k, (ref, _) in br.head_grads(sd, kind, op, plain, dout).items():
        dr.close(grads[k], ref.float(), f'{name} {k}')
    meta = dict(kind=kind, kw=kw, op=op, rows=rows, keys=[f'p.{k}' for k in sd])
    path = os.path.join(HERE, f'g30_decoder_grad_{name}.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), dout=dout.numpy(),
                        **{f'p.{k}': v.numpy() for k, v in sd.items()}, **{k: v.numpy() for k, v in plain.items()},
                        **{f'g.{k}': v.numpy() for k, v in grads.items()})  # fmt: skip
    size = os.path.getsize(path)
    assert size < 500_000, (name, size)  # float32 parameters and their gradients: twice a g26 fixture
    print(f'g30_decoder_grad_{name}: {size} bytes, {len(grads)} gradients')


def main() -> None:
    for seed, name in enumerate(br.EXPECTED_GRAD_FIXTURES):
        fixture(name, 3000 + seed)


if __name__ == '__main__':
    torch.set_num_threads(1)
    main()
