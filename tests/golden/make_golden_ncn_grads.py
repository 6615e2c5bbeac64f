#!/usr/bin/env python
"""Generate the NCNPredictor gradient fixtures tests/golden/g31_ncn_grad_*.npz by running the REFERENCE's ``NCNPredictor``
(tgm/nn/decoder/ncnpred.py) under float32 autograd on the host.

Runs only where the reference checkout is (PyG is replaced by the names-only placeholder in tests/golden/_pyg_stub).  The inputs are
``make_golden_ncn.py``'s small ones (N = 12, E = 40, B = 9, C = 5, targets drawn from few ids, so duplicate targets, repeated edges and
pairs with i = j are everywhere); the weights are the reference's own initialisation under the case's seed, the upstream gradient is
standard normal.  Recorded as plain .npz data:

    meta                k, decay, variant, N, C, H, out, keys (the reference's state_dict keys, in its order, each prefixed 'p.')
    p.<state_dict key>  the parameters (float32)
    x, edge_index, tar_ei[, last_update, edge_time]   the inputs
    dout                the upstream gradient, the shape of the reference's output
    g.<name>            the reference's float32 gradient of x and of every xsmlp parameter (``out.backward(dout)``); xslin gets none

    python tests/golden/make_golden_ncn_grads.py

The float64 restatement of the gradients (tests/ncn_bwd_restate.py) must agree with every recorded one within 1e-5 of max(1, |ref|)
before anything is written.
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
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from tgm.nn.decoder.ncnpred import NCNPredictor  # noqa: E402

import ncn_bwd_restate as br  # noqa: E402
import ncn_restate as nr  # noqa: E402
from make_golden_ncn import small_inputs  # noqa: E402

# name -> (input variant, k, decay)
CASES = {'k2_plain': ('samepair', 2, False), 'k2_decay': ('rand', 2, True), 'k4_plain': ('bothways', 4, False), 'k4_decay': ('samepair', 4, True),
         'onevsmany': ('onevsmany', 4, True), 'selfloop': ('selfloop', 4, False)}  # fmt: skip
H, OUT = 8, 1


def fixture(name: str, seed: int) -> None:
    variant, k, decay = CASES[name]
    g = torch.Generator().manual_seed(seed)
    x, ei, tar, lu, et = small_inputs(variant, g)
    if not decay:
        lu = et = None
    torch.manual_seed(seed)
    model = NCNPredictor(x.shape[1], H, OUT, k=k, cn_time_decay=decay).train()
    sd = {n: v.detach().clone() for n, v in model.state_dict().items()}
    xg = x.clone().requires_grad_()
    out = model(xg, ei, tar, lu, et)
    dout = torch.randn(out.shape, generator=g)
    out.backward(dout)
    assert model.xslin.weight.grad is None and model.xslin.bias.grad is None, name
    grads = {'x': xg.grad.detach().clone()}
    grads.update({n: p.grad.detach().clone() for n, p in model.named_parameters() if n.startswith('xsmlp.')})
    assert set(grads) == {'x', *br.PARAMS}, name
    for n, (ref, _) in br.grads(sd, x, ei, tar, k, dout, lu, et).items():
        if not n.startswith('_'):
            err = nr.rel_err(grads[n], ref)
            assert err < 1e-5, (name, n, err)
    meta = dict(k=k, decay=decay, variant=variant, N=x.shape[0], C=x.shape[1], H=H, out=OUT, keys=[f'p.{n}' for n in sd])
    arrays = dict(x=x.numpy(), edge_index=ei.numpy(), tar_ei=tar.numpy(), dout=dout.numpy())
    if decay:
        arrays.update(last_update=lu.numpy(), edge_time=et.numpy())
    path = os.path.join(HERE, f'g31_ncn_grad_{name}.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays,
                        **{f'p.{n}': v.numpy() for n, v in sd.items()}, **{f'g.{n}': v.numpy() for n, v in grads.items()})  # fmt: skip
    size = os.path.getsize(path)
    assert size < 500_000, (name, size)
    print(f'g31_ncn_grad_{name}: {size} bytes, {len(grads)} gradients')


def main() -> None:
    assert sorted(CASES) == br.EXPECTED_GRAD_FIXTURES
    for seed, name in enumerate(sorted(CASES)):
        fixture(name, 3100 + seed)


if __name__ == '__main__':
    torch.set_num_threads(1)
    main()
