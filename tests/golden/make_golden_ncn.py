#!/usr/bin/env python
"""Generate the NCNPredictor fixtures tests/golden/g18_ncn_*.npz by running the REFERENCE.

Runs only where the reference checkout is (PyG is replaced by the names-only placeholder in tests/golden/_pyg_stub).  It imports the
reference's ``NCNPredictor`` (tgm/nn/decoder/ncnpred.py), runs it on the CPU in float32 with ``eval()`` and fixed seeds, and writes plain
.npz data: the inputs, the ``state_dict`` arrays (for the example's shape the seeds of ``ncn_restate.hashed_state_dict`` / ``hashed_x``
instead), ``cn_emb`` and the logits.

    python tests/golden/make_golden_ncn.py

  g18_ncn_{variant}_k{2,4}_{plain,decay}   N = 12, E = 40, B = 9, C = 5; variants: ``rand``, ``onevsmany`` (tar_i constant), ``selfloop``,
                                          ``samepair`` (tar_i[r] == tar_j[r]), ``bothways`` (one edge in both directions); targets are
                                          drawn from few ids, so duplicates (the reference's last-write-wins row mapping) are everywhere
  g18_ncn_hub_k{2,4}                      N = 300, E = 900, C = 100, B = 33: one node of degree ~700; pairs (hub, hub), (hub, leaf),
                                          (leaf, isolated), (leaf, leaf)
  g18_ncn_width_c{C}_h{H}_o{out}          N = 40, E = 120, B = 7
  g18_ncn_decay_edges                     Unix-scale edge_time over last_update = 0 (the weight underflows to 0), gaps of 0, a negative gap
  g18_ncn_example_k{2,4}                  the example's shape: C = 100, H = 100, out 1, B = 200, a sampled-subgraph-sized edge list; x and the
                                          weights from seeds
  g18_ncn_self_noise.json                 for every fixture the distance of the reference's float32 cn_emb / logits from the float64
                                          restatement, max |a - b| / max(1, |b|)
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
from tgm.nn.decoder.ncnpred import NCNPredictor  # noqa: E402

import ncn_restate as nr  # noqa: E402

NOISE = {}


def save(name: str, meta: dict, **arrays) -> None:
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(f'{name}: {os.path.getsize(path)} bytes')


def case(name: str, x, ei, tar, k: int, H: int, out: int, seed: int, lu=None, et=None, hashed: bool = False, x_seed=None) -> None:
    torch.manual_seed(seed)
    C = x.shape[1]
    decay = lu is not None
    m = NCNPredictor(C, H, out, k=k, cn_time_decay=decay).eval()
    meta = dict(N=x.shape[0], C=C, H=H, out=out, k=k, decay=decay)
    with torch.no_grad():
        if hashed:
            shapes = {n: list(v.shape) for n, v in m.state_dict().items()}
            meta.update(weights_seed=seed, shapes=shapes)
            m.load_state_dict(nr.hashed_state_dict(shapes, seed), strict=True)
        cn = m.get_cn_emb(x, ei, tar, (lu, et))
        cn = cn.to_dense() if cn.is_sparse else cn
        logits = m(x, ei, tar, lu, et)
    sd = {n: v.clone() for n, v in m.state_dict().items()}
    NOISE[name] = dict(cn_emb=nr.rel_err(cn, nr.cn_emb(x, ei, tar, k, lu, et)), logits=nr.rel_err(logits, nr.forward(sd, x, ei, tar, k, lu, et)))
    meta.update(state_dict_keys=list(sd), shapes={n: list(v.shape) for n, v in sd.items()}, dtypes={n: str(v.dtype)[6:] for n, v in sd.items()})
    arrays = dict(edge_index=ei.numpy(), tar_ei=tar.numpy(), cn_emb=cn.numpy(), logits=logits.numpy())
    if x_seed is not None:
        meta.update(x_seed=x_seed)
    else:
        arrays.update(x=x.numpy())
    if decay:
        arrays.update(last_update=lu.numpy(), edge_time=et.numpy())
    if not hashed:
        arrays.update({f'p_{n}': v.numpy() for n, v in sd.items()})
    save(name, meta, **arrays)


def small_inputs(variant: str, g, N=12, E=40, B=9, C=5):
    x = torch.randn((N, C), generator=g)
    ei = torch.randint(0, N, (2, E), generator=g)
    tar = torch.randint(0, 5, (2, B), generator=g)  # few ids: duplicates on both sides
    tar[1] += 3
    if variant == 'onevsmany':
        tar[0] = 4
        tar[1] = torch.randint(0, N, (B,), generator=g)
    elif variant == 'selfloop':
        ei[:, 3] = tar[0, -1]
        ei[:, 17] = 7
        tar[1, 2] = 7
    elif variant == 'samepair':
        tar[1, 1], tar[1, -1] = tar[0, 1], tar[0, -1]
    elif variant == 'bothways':
        ei[0, 5], ei[1, 5] = ei[1, 4].item(), ei[0, 4].item()
        tar[0, -1], tar[1, -1] = ei[0, 4].item(), ei[1, 4].item()
    lu = torch.randint(0, 50_000, (N,), generator=g)
    et = torch.randint(40_000, 90_000, (B,), generator=g)
    return x, ei, tar, lu, et


SMALL_VARIANTS = ['rand', 'onevsmany', 'selfloop', 'samepair', 'bothways']


def hub_inputs(g, N=300, E=900, B=33, C=100):
    x = torch.randn((N, C), generator=g)
    ei = torch.randint(1, 250, (2, E), generator=g)  # nodes 250 .. 299 stay isolated
    hub_side = torch.rand(E, generator=g) < 0.75
    ei[0, hub_side] = 0  # node 0: degree ~700, with repeated neighbours
    ei[:, 11] = 0  # the hub's self-loop
    leaves = torch.randint(1, 250, (B,), generator=g)
    ti = leaves.clone()
    tj = torch.randint(1, 250, (B,), generator=g)
    ti[0], tj[0] = 0, 0  # (hub, hub)
    ti[1:9] = 0  # (hub, leaf)
    tj[9:12] = 0  # (leaf, hub)
    tj[12:16] = torch.arange(250, 254)  # (leaf, isolated)
    ti[32], tj[32] = 0, ei[1, 0]  # the hub's last occurrence on the source side
    return x, ei, torch.stack([ti, tj])


def example_inputs(g, x_seed: int, N=1500, E=4400, B=200, C=100):
    """A sampled-subgraph-shaped input: 600 seed rows of up to 10 neighbours over ~1500 local ids, B = 200 pairs among the first 600 ids."""
    x = nr.hashed_x(N, C, x_seed)
    other = torch.where(torch.rand(E, generator=g) < 0.8, torch.randint(600, 760, (E,), generator=g), torch.randint(0, N, (E,), generator=g))
    ei = torch.stack([torch.randint(0, 600, (E,), generator=g), other])  # most neighbours are a few popular ids: pairs do share some
    tar = torch.stack([torch.randint(0, 200, (B,), generator=g), torch.randint(200, 600, (B,), generator=g)])
    lu = torch.randint(2 * 10**6 - 60_000, 2 * 10**6, (N,), generator=g)
    et = torch.sort(torch.randint(2 * 10**6, 2 * 10**6 + 20_000, (B,), generator=g)).values
    return x, ei, tar, lu, et


if __name__ == '__main__':
    torch.set_num_threads(1)
    seed = 1800
    for v in SMALL_VARIANTS:
        for k in (2, 4):
            for decay in (False, True):
                seed += 1
                g = torch.Generator().manual_seed(seed)
                x, ei, tar, lu, et = small_inputs(v, g)
                case(f'g18_ncn_{v}_k{k}_{"decay" if decay else "plain"}', x, ei, tar, k, 8, 1, seed, *((lu, et) if decay else (None, None)))
    for k in (2, 4):
        seed += 1
        g = torch.Generator().manual_seed(seed)
        x, ei, tar = hub_inputs(g)
        case(f'g18_ncn_hub_k{k}', x, ei, tar, k, 16, 1, seed)
    for C, H, out in ((5, 8, 1), (64, 100, 1), (100, 100, 3), (172, 8, 1), (256, 100, 3)):
        seed += 1
        g = torch.Generator().manual_seed(seed)
        x = torch.randn((40, C), generator=g)
        ei, tar = torch.randint(0, 40, (2, 120), generator=g), torch.randperm(40, generator=g)[:14].reshape(2, 7)
        case(f'g18_ncn_width_c{C}_h{H}_o{out}', x, ei, tar, 4 if C in (5, 100, 256) else 2, H, out, seed)
    seed += 1
    g = torch.Generator().manual_seed(seed)
    x, ei, tar, lu, et = small_inputs('rand', g)
    lu[:4] = 0  # Unix-scale gaps: exp(-1.7e5) underflows to exactly 0
    et[:] = 1_700_000_000 + torch.arange(9)
    lu[4:8] = et[:4]  # gaps of 0 for the matching rows, a few seconds either way for the others (a negative gap: a weight above 1)
    lu[8:] = et[-1] + 25_000
    case('g18_ncn_decay_edges', x, ei, tar, 4, 8, 1, seed, lu, et)
    for k in (2, 4):
        seed += 1
        g = torch.Generator().manual_seed(seed)
        x, ei, tar, lu, et = example_inputs(g, seed)
        case(f'g18_ncn_example_k{k}', x, ei, tar, k, 100, 1, seed, lu, et, hashed=True, x_seed=seed)
    with open(os.path.join(HERE, 'g18_ncn_self_noise.json'), 'w') as f:
        json.dump(dict(fixtures=NOISE), f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(NOISE, indent=1))
