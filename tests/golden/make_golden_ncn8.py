#!/usr/bin/env python
"""Generate the k = 8 NCNPredictor fixtures tests/golden/g34_ncn8_*.npz by running the REFERENCE.

Runs only where the reference checkout is, exactly as make_golden_ncn.py does (whose input builders it reuses): the reference's
``NCNPredictor(k=8)`` on the CPU in float32, ``eval()``, fixed seeds; plain .npz data out.  Before it writes a fixture it asserts, on the float64
restatement's intermediates (tests/ncn8_restate.py), that every integer the reference forms stays below 2^24 (its float32 counts are exact),
that the decay weights are finite, and that the property the fixture is named after occurs.

    python tests/golden/make_golden_ncn8.py

  g34_ncn8_{variant}_{plain,decay}   N = 12, E = 40, B = 9, C = 5; make_golden_ncn.py's variants and ``triangle``: edges between the targets
                                    and triangles through them (u != 0, K3 diagonals, a negative c22 before the clamp, masked columns)
  g34_ncn8_hub                      N = 300, E = 900, C = 100, B = 33: a neighbour list longer than a wave, a two-hop row over most ids
  g34_ncn8_width_c{1,64,65,300}     N = 40, E = 120, B = 7
  g34_ncn8_wide_n{N}                N one past the kernel's LDS cap (7680), E = 120, B = 5, x from a seed
  g34_ncn8_decay_edges              gaps of 0, a negative finite gap, underflow to 0
  g34_ncn8_example                  the example's shape (make_golden_ncn.example_inputs), weights and x from seeds; cn_emb of 16 rows
  g34_ncn8_self_noise.json          per fixture: the reference's float32 distance from the float64 restatement
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden_ncn as g18  # noqa: E402  (sets the paths: the PyG placeholder, the reference, tests/)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from tgm.nn.decoder.ncnpred import NCNPredictor  # noqa: E402

import ncn8_restate as n8  # noqa: E402
import ncn_restate as nr  # noqa: E402

NOISE = {}
LDS_MAX_NODES = 7680  # csrc/ncn8.hip: kNcn8LdsMaxN
EXACT = float(1 << 24)


def largest_integer(co: dict) -> float:
    """The largest integer the reference forms in float32: the entries of A A and A A A, every product and sum on the way to the c blocks."""
    As = co['A'].to_sparse()
    A2 = torch.sparse.mm(As, As)
    K3 = torch.sparse.mm(A2, As)
    parts = [A2.coalesce().values(), K3.coalesce().values(), co['Si'] * co['Sj'], co['Ri'] * co['Sj'], co['Si'] * co['Rj'], co['Ri'] * co['Ri'] * co['u'], co['Rj'] * co['Rj'] * co['u'],
             (co['k3i'] + co['k3j'] + co['c11']) * co['u'], co['sp'], co['c12_raw'], co['c21_raw'], co['c22_raw']]  # fmt: skip
    return max(float(p.abs().max()) for p in parts)


def case(name: str, x, ei, tar, H: int, out: int, seed: int, lu=None, et=None, hashed: bool = False, x_seed=None, rows=None, check=None) -> None:
    torch.manual_seed(seed)
    N, C = x.shape
    decay = lu is not None
    co = n8.coefficients(N, ei, tar)
    big = largest_integer(co)
    assert big < EXACT, f'{name}: the reference forms {big:.0f} >= 2^24 in float32'
    if decay:
        assert torch.isfinite(nr.decay_weights(lu, et)).all(), f'{name}: a decay weight is not finite'
    if check is not None:
        check(co)
    m = NCNPredictor(C, H, out, k=8, cn_time_decay=decay).eval()
    meta = dict(N=N, C=C, H=H, out=out, k=8, decay=decay)
    with torch.no_grad():
        if hashed:
            shapes = {n: list(v.shape) for n, v in m.state_dict().items()}
            meta.update(weights_seed=seed, shapes=shapes)
            m.load_state_dict(nr.hashed_state_dict(shapes, seed), strict=True)
        cn = m.get_cn_emb(x, ei, tar, (lu, et))
        cn = cn.to_dense() if cn.is_sparse else cn
        logits = m(x, ei, tar, lu, et)
    sd = {n: v.clone() for n, v in m.state_dict().items()}
    ref_cn, ref_out = n8.cn_emb(x, ei, tar, lu, et), n8.forward(sd, x, ei, tar, lu, et)
    if rows is not None:
        rows = rows(cn)
        meta.update(cn_rows=[int(r) for r in rows])
        cn, ref_cn = cn[rows], ref_cn[rows]
    NOISE[name] = dict(cn_emb=nr.rel_err(cn, ref_cn), logits=nr.rel_err(logits, ref_out), largest_integer=big)
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
    g18.save(name, meta, **arrays)


def triangle_inputs(g):
    """Edges between the two targets of several pairs and a third node joined to both; the last pair is active whatever the duplicates."""
    x, ei, tar, lu, et = g18.small_inputs('rand', g)
    a, b = int(tar[0, -1]), int(tar[1, -1])
    c, d = 9, 10
    extra = [(a, b), (b, a), (a, c), (c, b), (a, d), (d, b), (c, d), (a, 11)]
    for s, (p, q) in enumerate(extra):
        ei[0, 2 * s], ei[1, 2 * s] = p, q
    a2, b2 = int(tar[0, -2]), int(tar[1, -2])
    ei[0, 30], ei[1, 30] = a2, b2
    ei[0, 31], ei[1, 31] = a2, c
    ei[0, 32], ei[1, 32] = c, b2
    return x, ei, tar, lu, et


def triangle_check(tar):
    ti, tj = tar[0], tar[1]
    ar = torch.arange(ti.numel())

    def check(co: dict) -> None:
        assert (co['u'] != 0).any(), 'triangle: no edge between the targets of an active pair'
        assert ((co['k3i'] != 0) & (co['u'] != 0)).any() and ((co['k3j'] != 0) & (co['u'] != 0)).any(), 'triangle: no K3 diagonal where u != 0'
        assert (co['c22_raw'] < 0).any(), 'triangle: the clamp has nothing to do'
        masked = sum(int((c[ar, t] != 0).sum()) for c in (co['c12_raw'], co['c21_raw'], co['c22_raw']) for t in (ti, tj))
        assert masked > 0, 'triangle: the column masks remove only zeros'

    return check


def hub_check(tar, N):
    def check(co: dict) -> None:
        deg = co['A'].sum(1)
        assert deg[0] > 64 and (co['A'][0] > 0).sum() > 64, 'hub: the hub row is no longer than a wave'
        assert ((co['A'][0] @ co['A']) > 0).sum() > N // 2, 'hub: the two-hop row does not touch most ids'
        ti, tj = tar[0], tar[1]
        assert ((ti == 0) & (tj == 0)).any() and ((ti == 0) & (tj != 0)).any() and (deg[tj] == 0).any() and ((ti != 0) & (tj != 0) & (deg[tj] > 0)).any()

    return check


def wide_inputs(g, N: int, E=120, B=5, C=5):
    """Few ids spread over the whole range, so that two-hop rows exist and the last id takes part."""
    ids = torch.cat([torch.tensor([0, 1, N - 1, N - 2, LDS_MAX_NODES - 1, LDS_MAX_NODES]), torch.randint(0, N, (18,), generator=g)])
    ei = ids[torch.randint(0, ids.numel(), (2, E), generator=g)]
    tar = torch.stack([ids[torch.randperm(6, generator=g)[:B]], ids[6 + torch.randperm(18, generator=g)[:B]]])
    tar[1, 0] = N - 1
    ei[:, 0] = torch.tensor([int(tar[0, 0]), N - 1])
    return ei, tar


if __name__ == '__main__':
    torch.set_num_threads(1)
    seed = 3400
    for v in g18.SMALL_VARIANTS + ['triangle']:
        for decay in (False, True):
            seed += 1
            g = torch.Generator().manual_seed(seed)
            x, ei, tar, lu, et = triangle_inputs(g) if v == 'triangle' else g18.small_inputs(v, g)
            case(f'g34_ncn8_{v}_{"decay" if decay else "plain"}', x, ei, tar, 8, 1, seed, *((lu, et) if decay else (None, None)),
                 check=triangle_check(tar) if v == 'triangle' else None)  # fmt: skip
    seed += 1
    share = 0.75
    # shrink the hub until the reference's float32 integers are exact AND the reference's own float32 sums stay a factor 4 inside the
    # project's bar for aggregated values (1e-5, absolute below 1): with 3 in 4 edges on the hub and x ~ N(0, 1) the two-hop blocks sum 240
    # terms of size 1e3 that cancel, and the reference itself is 2.6e-4 from float64 -- a fixture it does not meet says nothing.  x gets the
    # scale of an embedding layer's output (0.1), then the hub shrinks.
    while True:
        g = torch.Generator().manual_seed(seed)
        x, ei, tar = g18.hub_inputs(g)
        x = x * 0.1
        thin = torch.rand(ei.shape[1], generator=g) > share / 0.75  # hub_inputs puts 3 in 4 edges on the hub: move some of them off it
        thin[11] = False
        ei[0, thin & (ei[0] == 0)] = torch.randint(1, 250, (int((thin & (ei[0] == 0)).sum()),), generator=g)
        with torch.no_grad():
            ref_noise = nr.rel_err(NCNPredictor(100, 16, 1, k=8).eval().get_cn_emb(x, ei, tar, (None, None)), n8.cn_emb(x, ei, tar))
        if largest_integer(n8.coefficients(300, ei, tar)) < EXACT and ref_noise < 2.5e-6:
            break
        share -= 0.05
        assert share > 0.04, 'hub: no hub left'
    print(f'hub: {share:.2f} of the edges on node 0')
    case('g34_ncn8_hub', x, ei, tar, 16, 1, seed, check=hub_check(tar, 300))
    for C in (1, 64, 65, 300):
        seed += 1
        g = torch.Generator().manual_seed(seed)
        x = torch.randn((40, C), generator=g)
        ei, tar = torch.randint(0, 40, (2, 120), generator=g), torch.randperm(40, generator=g)[:14].reshape(2, 7)
        case(f'g34_ncn8_width_c{C}', x, ei, tar, 8, 1, seed)
    seed += 1
    g = torch.Generator().manual_seed(seed)
    N = LDS_MAX_NODES + 1
    ei, tar = wide_inputs(g, N)
    case(f'g34_ncn8_wide_n{N}', nr.hashed_x(N, 5, seed), ei, tar, 8, 1, seed, x_seed=seed)
    seed += 1
    g = torch.Generator().manual_seed(seed)
    x, ei, tar, lu, et = triangle_inputs(g)
    lu[:4] = 0  # Unix-scale gaps: exp(-1.7e5) underflows to exactly 0
    et[:] = 1_700_000_000 + torch.arange(9)
    lu[4:8] = et[:4]  # gaps of 0 for the matching rows, a few seconds either way for the others
    lu[8:] = et[-1] + 25_000  # a negative finite gap: a weight above 1
    case('g34_ncn8_decay_edges', x, ei, tar, 8, 1, seed, lu, et)
    seed += 1
    g = torch.Generator().manual_seed(seed)
    x, ei, tar, lu, et = g18.example_inputs(g, seed)

    def sixteen(cn):
        nz = torch.nonzero(cn.abs().sum(1) > 0).reshape(-1)
        assert nz.numel() >= 8, 'example: fewer than 8 pairs with a common-neighbour block'
        rest = [r for r in range(cn.shape[0]) if r not in set(nz[:12].tolist())]
        return sorted(nz[:12].tolist() + rest[: 16 - min(12, nz.numel())])

    case('g34_ncn8_example', x, ei, tar, 100, 1, seed, lu, et, hashed=True, x_seed=seed, rows=sixteen)
    with open(os.path.join(HERE, 'g34_ncn8_self_noise.json'), 'w') as f:
        json.dump(dict(fixtures=NOISE), f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(NOISE, indent=1))
