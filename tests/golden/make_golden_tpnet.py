#!/usr/bin/env python
"""Generate the TPNet fixtures tests/golden/g17_tpnet_*.npz by running the REFERENCE.

Runs only where the reference checkout is (PyG is replaced by the names-only placeholder in tests/golden/_pyg_stub).  It imports the
reference's ``RandomProjectionModule`` and ``TPNet``, runs them on the CPU in float32 with ``eval()`` and fixed seeds, and writes plain
.npz data: inputs, the ``state_dict`` arrays (for the example's dimensions the seed of ``tpnet_restate.hashed_state_dict`` instead: the
weights alone would pass the committed-file size limit) and the reference's outputs.

    python tests/golden/make_golden_tpnet.py

  g17_tpnet_update_{name}   the tables after a recorded stream of 32 batches: duplicate targets inside a batch, self-loops, nodes that are
                            source and destination in one batch, ties in time, a batch whose last time equals the previous one's
                            (``rand_l2``: dim 16, two layers; ``matrix_l3``: use_matrix, three layers; ``rand_l1``: dim 7, one layer)
  g17_tpnet_pair_{name}     ``RandomProjectionModule.forward`` after a few updates, ids with pads (-1: the last row): both
                            concat_src_dst settings, scale on and off, use_matrix, enforce_dim, dims 1, 7, 90, 120 and 300
  g17_tpnet_enc_{name}      the full encoder: small dims with / without random projections, concat off, a pad-heavy input with an
                            all-pad row, and the example's dims (k 32, node 128, edge 172, time 100, out 172, two mixer layers, dim 120)
  g17_tpnet_self_noise.json for every float fixture the distance of the reference's float32 output from the float64 restatement,
                            max |a - b| / max(1, |b|)
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
from tgm.nn.encoder.tpnet import RandomProjectionModule, TPNet  # noqa: E402

import tpnet_restate as tr  # noqa: E402

NOISE = {}


def save(name: str, meta: dict, **arrays) -> None:
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(f'{name}: {os.path.getsize(path)} bytes')


def stream(g, N, nb, bs, step):
    """[nb, bs] sources, destinations, times (sorted, with ties) carrying the corner cases the update has to get right."""
    src = torch.randint(0, N, (nb, bs), generator=g)
    dst = torch.randint(0, N, (nb, bs), generator=g)
    gaps = torch.randint(0, step, (nb * bs,), generator=g)
    gaps[torch.rand(nb * bs, generator=g) < 0.3] = 0  # ties in time
    t = (1000 + torch.cumsum(gaps, 0)).reshape(nb, bs)
    src[1, 3] = dst[1, 3]  # a self-loop
    src[2, :4] = src[2, 0]  # one target four times in a batch
    dst[2, 4:7] = src[2, 0]  # ... that is also a destination in it
    src[3, 1], dst[3, 1] = dst[3, 0].item(), src[3, 0].item()  # the same edge in both directions
    t[5] = t[4, -1]  # a whole batch at the previous batch's last time: next == now
    t[9, :] = t[9, -1]  # every edge of a batch at one time
    src[11] = dst[10]  # this batch's sources were the previous batch's destinations
    return src, dst, t


def rp_kwargs(cfg: dict) -> dict:
    return dict(num_nodes=cfg['num_nodes'], num_layer=cfg['num_layer'], time_decay_weight=cfg['lam'], beginning_time=cfg['beginning_time'],
                use_matrix=cfg['use_matrix'], scale_random_projection=cfg.get('scale', True), enforce_dim=cfg.get('enforce_dim'),
                num_edges=cfg.get('num_edges'), dim_factor=cfg.get('dim_factor'), concat_src_dst=cfg.get('concat', True))  # fmt: skip


def update_case(name: str, cfg: dict, nb: int, bs: int, seed: int) -> None:
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    m = RandomProjectionModule(**rp_kwargs(cfg))
    p0 = m.random_projections[0].detach().clone()
    src, dst, t = stream(g, cfg['num_nodes'], nb, bs, cfg['step'])
    tabs, now = [p.detach().clone() for p in m.random_projections], cfg['beginning_time']
    with torch.no_grad():
        for b in range(nb):
            m.update(src[b], dst[b], t[b])
            tabs, now = tr.rp_update(tabs, now, src[b], dst[b], t[b], cfg['lam'])
    NOISE[name] = max(tr.rel_err(m.random_projections[i], tabs[i]) for i in range(1, cfg['num_layer'] + 1))
    arrays = {f'table_{i}': m.random_projections[i].detach().numpy() for i in range(1, cfg['num_layer'] + 1)}
    save(name, dict(cfg=cfg, dim=m.dim, now=int(m.now_time.reshape(-1)[0])), p0=p0.numpy(), src=src.numpy().astype(np.int32),
         dst=dst.numpy().astype(np.int32), time=t.numpy(), **arrays)  # fmt: skip


def warmed_module(cfg: dict, seed: int, nb: int = 6, bs: int = 20):
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 1)
    m = RandomProjectionModule(**rp_kwargs(cfg)).eval()
    src, dst, t = stream(g, cfg['num_nodes'], max(nb, 12), bs, cfg['step'])
    with torch.no_grad():
        for p in m.mlp.parameters():
            p.add_(0.05 * torch.randn_like(p))
        for b in range(nb):
            m.update(src[b], dst[b], t[b])
    return m, g


def pair_case(name: str, cfg: dict, seed: int, P: int = 60) -> None:
    m, g = warmed_module(cfg, seed)
    N = cfg['num_nodes']
    a = torch.randint(0, N, (P,), generator=g)
    b = torch.randint(0, N, (P,), generator=g)
    a[::7] = -1  # pad ids: the last table row
    b[3], a[5], b[5] = a[3].item(), -1, -1
    with torch.no_grad():
        out = m(a, b)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    NOISE[name] = tr.rel_err(out, tr.rp_forward(sd, '', cfg['num_layer'], a, b, cfg.get('concat', True), cfg.get('scale', True)))
    save(name, dict(cfg=cfg, dim=m.dim, out_dim=m.out_dim, state_dict_keys=list(sd), dtypes={k: str(v.dtype)[6:] for k, v in sd.items()}),
         a=a.numpy().astype(np.int32), b=b.numpy().astype(np.int32), out=out.numpy(), **{f'p_{k}': v.numpy() for k, v in sd.items()})  # fmt: skip


def encoder_inputs(g, B, k, N, dN, dE, max_gap, pad_frac, all_pad_rows=()):
    src = torch.randint(0, N, (B,), generator=g)
    dst = torch.randint(0, N, (B,), generator=g)
    nids = torch.randint(0, N, (2 * B, k), generator=g)
    nids[torch.rand(2 * B, k, generator=g) < pad_frac] = -1
    for r in all_pad_rows:
        nids[r] = -1
    edge_time = torch.randint(max_gap, 2 * max_gap, (B,), generator=g)
    t2 = torch.cat([edge_time, edge_time])
    nbr_t = t2[:, None] - torch.randint(0, max_gap, (2 * B, k), generator=g)
    nbr_t[nids == -1] = 0  # what the sampler leaves in a padded slot
    ex = torch.rand((2 * B, k, dE), generator=g)
    ex[nids == -1] = 0.0
    pads = (nids == -1).nonzero()
    if len(pads):
        ex[pads[0, 0], pads[0, 1]] = 0.5  # edge features of a padded slot are taken as they come
    node_x = torch.randn((N, dN), generator=g)
    return dict(node_x=node_x, src=src, dst=dst, edge_time=edge_time, nbr_nids=nids, nbr_time=nbr_t, nbr_edge_x=ex)


def encoder_case(name: str, dims: dict, cfg, B: int, max_gap: int, pad_frac: float, seed: int, hashed: bool = False, all_pad_rows=()) -> None:
    rp = None
    if cfg is not None:
        rp, _ = warmed_module(cfg, seed + 7)
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    m = TPNet(**dims, random_projections=rp).eval()
    N = cfg['num_nodes'] if cfg is not None else 30
    inp = encoder_inputs(g, B, dims['num_neighbors'], N, dims['node_feat_dim'], dims['edge_x_dim'], max_gap, pad_frac, all_pad_rows)
    meta = dict(dims=dims, cfg=cfg, max_gap=max_gap)
    with torch.no_grad():
        if hashed:
            shapes = {k: list(v.shape) for k, v in m.state_dict().items()}
            dtypes = {k: str(v.dtype)[6:] for k, v in m.state_dict().items()}
            meta.update(weights_seed=seed, shapes=shapes)
            m.load_state_dict(tr.hashed_state_dict(shapes, dtypes, seed), strict=True)
        else:
            for n, p in m.named_parameters():
                if p.is_floating_point() and not n.startswith(('time_encoder.w.weight', 'random_projections.')):
                    p.add_(0.05 * torch.randn_like(p))
        zs, zd = m(inp['node_x'], torch.stack([inp['src'], inp['dst']]), inp['edge_time'], inp['nbr_nids'], inp['nbr_time'], inp['nbr_edge_x'])
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    rpd = None if cfg is None else dict(num_layer=cfg['num_layer'], concat=cfg.get('concat', True), scale=cfg.get('scale', True))
    rs, rd = tr.tpnet_forward(sd, dims['num_layers'], rpd, inp['node_x'], inp['src'], inp['dst'], inp['edge_time'], inp['nbr_nids'], inp['nbr_time'],
                              inp['nbr_edge_x'])  # fmt: skip
    NOISE[name] = max(tr.rel_err(zs, rs), tr.rel_err(zd, rd))
    meta.update(state_dict_keys=list(sd), dtypes={k: str(v.dtype)[6:] for k, v in sd.items()})
    arrays = dict(node_x=inp['node_x'].numpy(), src=inp['src'].numpy().astype(np.int32), dst=inp['dst'].numpy().astype(np.int32),
                  edge_time=inp['edge_time'].numpy(), nbr_nids=inp['nbr_nids'].numpy().astype(np.int32), nbr_time=inp['nbr_time'].numpy(),
                  nbr_edge_x=inp['nbr_edge_x'].numpy(), z_src=zs.numpy(), z_dst=zd.numpy())  # fmt: skip
    if not hashed:
        arrays.update({f'p_{k}': v.numpy() for k, v in sd.items()})
    save(name, meta, **arrays)


RAND = dict(num_nodes=40, num_layer=2, lam=1e-4, beginning_time=1000, use_matrix=False, enforce_dim=16, step=400)
UPDATE_CASES = {
    'rand_l2': RAND,
    'matrix_l3': dict(num_nodes=24, num_layer=3, lam=2e-4, beginning_time=1000, use_matrix=True, step=300),
    'rand_l1': dict(num_nodes=15, num_layer=1, lam=1e-3, beginning_time=990, use_matrix=False, enforce_dim=7, step=100),
}
PAIR_CASES = {
    'concat_scale': dict(RAND),
    'concat_raw': dict(RAND, scale=False),
    'cross_scale': dict(RAND, concat=False),
    'cross_raw': dict(RAND, concat=False, scale=False),
    'matrix': dict(num_nodes=24, num_layer=2, lam=2e-4, beginning_time=1000, use_matrix=True, step=300),
    'dim1': dict(RAND, enforce_dim=1),
    'dim7_l1': dict(RAND, enforce_dim=7, num_layer=1),
    'dim90_l3': dict(RAND, enforce_dim=90, num_layer=3, concat=False),
    'dim120_factor': dict(num_nodes=300, num_layer=2, lam=1e-4, beginning_time=1000, use_matrix=False, num_edges=100000, dim_factor=10, step=400),
    'dim300': dict(RAND, enforce_dim=300),
}
SMALL = dict(node_feat_dim=6, edge_x_dim=5, time_feat_dim=8, output_dim=12, num_neighbors=8, num_layers=2, dropout=0.1)
EXAMPLE = dict(node_feat_dim=128, edge_x_dim=172, time_feat_dim=100, output_dim=172, num_neighbors=32, num_layers=2, dropout=0.1)
EXAMPLE_RP = dict(num_nodes=130, num_layer=2, lam=1e-6, beginning_time=0, use_matrix=False, num_edges=100000, dim_factor=10, step=400)


if __name__ == '__main__':
    torch.set_num_threads(1)
    for i, (n, cfg) in enumerate(UPDATE_CASES.items()):
        update_case(f'g17_tpnet_update_{n}', cfg, 32, 12, 1700 + i)
    for i, (n, cfg) in enumerate(PAIR_CASES.items()):
        pair_case(f'g17_tpnet_pair_{n}', cfg, 1720 + i)
    encoder_case('g17_tpnet_enc_small', SMALL, dict(RAND), 7, 10**4, 0.35, 1740)
    encoder_case('g17_tpnet_enc_small_norp', SMALL, None, 7, 10**4, 0.35, 1741)
    encoder_case('g17_tpnet_enc_small_cross', dict(SMALL, num_layers=1), dict(RAND, concat=False, scale=False), 5, 10**4, 0.35, 1742)
    encoder_case('g17_tpnet_enc_padheavy', SMALL, dict(RAND), 6, 10**5, 0.8, 1743, all_pad_rows=(0, 7))
    encoder_case('g17_tpnet_enc_single', dict(SMALL, num_neighbors=3), dict(RAND, num_layer=1), 1, 10**4, 0.3, 1744)
    encoder_case('g17_tpnet_enc_example', EXAMPLE, EXAMPLE_RP, 6, 10**5, 0.3, 1745, hashed=True)
    with open(os.path.join(HERE, 'g17_tpnet_self_noise.json'), 'w') as f:
        json.dump(dict(fixtures=NOISE), f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(NOISE, indent=1))
