#!/usr/bin/env python
"""Generate the TPNet gradient fixtures tests/golden/g32_tpnet_grad_*.npz by running the REFERENCE's ``TPNet`` (tgm/nn/encoder/tpnet.py)
under float32 autograd on the host, after ``make_golden_ncn_grads.py``.

Runs only where the reference checkout is (PyG is replaced by the names-only placeholder in tests/golden/_pyg_stub).  The inputs and the
weights are those of ``g17_tpnet_enc_{small, small_norp, small_cross, single, padheavy}`` (stored arrays, or the recorded seed), the model
is in eval mode (no dropout), the upstream gradient is standard normal.  Recorded as plain .npz data:

    meta       the g17 fixture's name, the seed of dout
    dout       the upstream gradient [2B, E] (sources, then destinations)
    g.<name>   the reference's float32 gradient of every trainable parameter (``cat(z_src, z_dst).backward(dout)``)

and, alongside, ``g32_tpnet_grad_noise.json``: per case and parameter the distance of the recorded gradient from the float64 restatement
(tests/tpnet_bwd_restate.py under float64 autograd), max |got - ref| over the restated gradient's largest entry.  On ``padheavy`` the
reference's float32 run carries the constant-column noise of its plain token LayerNorm (an error d of a column's mean comes out as
d / sqrt(eps) = 316 d), so that distance is the largest there (1.7e-5 against 7e-7 .. 5e-6); it is recorded, not bounded.

    python tests/golden/make_golden_tpnet_grads.py
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
sys.path.insert(0, REPO)  # (the restatements import oracle/)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from tgm.nn import TPNet  # noqa: E402
from tgm.nn.encoder.tpnet import RandomProjectionModule  # noqa: E402

import tpnet_bwd_restate as br  # noqa: E402
from golden_util import load  # noqa: E402
from test_tpnet_cpu import encoder_inputs, fixture_state_dict, rp_dict, rp_kwargs  # noqa: E402

CASES = ('small', 'small_norp', 'small_cross', 'single', 'padheavy')


def trainable(name: str) -> bool:
    return name.split('.')[-1] in ('weight', 'bias')


def fixture(name: str, seed: int) -> dict:
    meta, a = load(f'g17_tpnet_enc_{name}')
    sd = fixture_state_dict(meta, a)
    rp = None if meta['cfg'] is None else RandomProjectionModule(**rp_kwargs(meta['cfg']))
    model = TPNet(**meta['dims'], random_projections=rp)
    model.load_state_dict(sd, strict=True)
    model.eval()
    i = encoder_inputs(a)
    zs, zd = model(i['node_x'], torch.stack([i['src'], i['dst']]), i['edge_time'], i['nbr_nids'], i['nbr_time'], i['nbr_edge_x'])
    out = torch.cat([zs, zd])
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed))
    out.backward(dout)
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad and p.grad is not None}
    assert sorted(grads) == sorted(n for n in sd if trainable(n)), name
    # the float64 restatement of the same gradients
    leaf = {n: (v.double().requires_grad_(True) if trainable(n) else (v.double() if v.is_floating_point() else v)) for n, v in sd.items()}
    r = torch.cat(br.forward(leaf, meta['dims']['num_layers'], rp_dict(meta['cfg']), i['node_x'], i['src'], i['dst'], i['edge_time'], i['nbr_nids'],
                             i['nbr_time'], i['nbr_edge_x']))  # fmt: skip
    (r * dout.double()).sum().backward()
    noise = {}
    for n, g in grads.items():
        ref = leaf[n].grad if leaf[n].grad is not None else torch.zeros_like(leaf[n])
        noise[n] = float((g.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)
    path = os.path.join(HERE, f'g32_tpnet_grad_{name}.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(dict(inputs=f'g17_tpnet_enc_{name}', dout_seed=seed)).encode(), dtype=np.uint8),
                        dout=dout.numpy(), **{f'g.{n}': v.numpy() for n, v in grads.items()})  # fmt: skip
    size = os.path.getsize(path)
    assert size < 500_000, (name, size)
    print(f'g32_tpnet_grad_{name}: {size} bytes, {len(grads)} gradients, worst distance from float64 {max(noise.values()):.3e}')
    return noise


def main() -> None:
    noise = {name: fixture(name, 3200 + k) for k, name in enumerate(CASES)}
    with open(os.path.join(HERE, 'g32_tpnet_grad_noise.json'), 'w') as f:
        json.dump(noise, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    torch.set_num_threads(1)
    main()
