#!/usr/bin/env python
"""Generate the GraphMixer fixtures tests/golden/g15_graphmixer_*.npz by running the REFERENCE.

Runs only in the build container (needs the reference checkout; PyG is replaced by the names-only placeholder in
tests/golden/_pyg_stub).  It drives the reference's own ``MLPMixer``, ``Time2Vec``, ``DGraph`` / ``DGDataLoader`` and
``_storage.get_edges``; GraphMixer's hook and encoder live in the reference's example script, so they are written out here in
this file's own words (same arithmetic).  Outputs are plain .npz data: inputs + the reference's outputs.

    python tests/golden/make_golden_graphmixer.py

  g15_graphmixer_hook_{plain,nodes,split}  time-gap lists per batch and time_gap (ties, self loops, repeated seeds, node events,
                                           the last partial batch, a split's own timeline)
  g15_graphmixer_mixer_{i}                 MLPMixer forward over odd shapes (K, C, expansion factors)
  g15_graphmixer_encoder                   GraphMixer encoder forward (small dims, padded slots, empty and repeated time-gap runs)
"""
from __future__ import annotations

import json
import os
import sys
from dataclasses import replace

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('TGM_REFERENCE', os.path.join(os.path.dirname(REPO), 'reference'))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, '_pyg_stub'))
sys.path.insert(0, REFERENCE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
from tgm import DGraph  # noqa: E402
from tgm.data import DGData, DGDataLoader  # noqa: E402
from tgm.hooks import HookManager  # noqa: E402
from tgm.hooks.base import StatelessHook  # noqa: E402
from tgm.nn import MLPMixer, Time2Vec  # noqa: E402

GAPS = [0, 1, 2, 37, 2000]


def save(name: str, meta: dict, **arrays) -> None:
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(f'{name}: {os.path.getsize(path)} bytes')


class FixedNegatives(StatelessHook):
    """One pre-drawn negative per edge, looked up by the edge's position in the stream."""

    requires = {'edge_src', 'edge_dst', 'edge_time'}
    produces = {'neg', 'neg_time'}

    def __init__(self, neg_by_time_rank: torch.Tensor, all_times: torch.Tensor) -> None:
        self.neg, self.times = neg_by_time_rank, all_times
        self.cursor = 0

    def __call__(self, dg, batch):
        n = batch.edge_src.numel()
        batch.neg = self.neg[self.cursor : self.cursor + n].clone()
        batch.neg_time = batch.edge_time.clone()
        self.cursor += n
        return batch

    def reset_state(self) -> None:
        self.cursor = 0


class TimeGapLists(StatelessHook):
    """GraphMixer's time-gap hook: the edges of the last ``gap`` events before the batch (an event-index window that ends at the
    batch's nominal end and excludes the batch's first timestamp), each seen from both endpoints, collected per seed."""

    requires = {'neg'}
    produces = {'time_gap_nbrs'}

    def __init__(self, gap: int) -> None:
        self.gap = gap

    def __call__(self, dg, batch):
        window = replace(dg._slice)
        window.start_idx = max(dg._slice.end_idx - self.gap, 0)
        window.end_time = int(batch.edge_time.min()) - 1
        u, v, _ = dg._storage.get_edges(window)
        table = {}
        for a, b in zip(u.tolist(), v.tolist()):
            table.setdefault(a, []).append(b)
            table.setdefault(b, []).append(a)
        seeds = torch.cat([batch.edge_src, batch.edge_dst, batch.neg])
        batch.time_gap_nbrs = [list(table.get(s, [])) for s in seeds.tolist()]
        return batch


def make_data(seed: int, E: int, N: int, node_events: bool):
    g = torch.Generator().manual_seed(seed)
    ts = torch.sort(torch.randint(0, E // 3, (E,), generator=g)).values  # ~3 edges per timestamp: ties at batch starts
    src = torch.randint(0, N, (E,), generator=g, dtype=torch.int64)
    dst = torch.randint(0, N, (E,), generator=g, dtype=torch.int64)
    loops = torch.rand(E, generator=g) < 0.06
    dst[loops] = src[loops]
    x = torch.rand((E, 3), generator=g)
    neg = torch.randint(0, N, (E,), generator=g, dtype=torch.int32)
    kw = {}
    if node_events:
        M = E // 6
        kw = dict(node_x_time=torch.sort(torch.randint(0, E // 3, (M,), generator=g)).values,
                  node_x_nids=torch.randint(0, N, (M,), generator=g, dtype=torch.int64), node_x=torch.rand((M, 2), generator=g))  # fmt: skip
    return ts, torch.stack([src, dst], 1), x, neg, kw


def hook_case(name: str, seed: int, E: int, N: int, bs: int, node_events: bool, split: bool) -> None:
    ts, ei, x, neg, kw = make_data(seed, E, N, node_events)
    data = DGData.from_raw(ts, ei, x, **kw)
    if split:
        data = data.split()[1]  # the validation split: its own timeline (event indices start at 0 again)
    dg = DGraph(data)
    st = dg._storage._data
    times = st.time.numpy()
    edge_event = st.edge_mask.numpy()
    src = st.edge_index[:, 0].numpy().astype(np.int32)
    dst = st.edge_index[:, 1].numpy().astype(np.int32)
    ne = len(src)
    neg_e = neg[:ne]
    out = {}
    for gap in GAPS:
        hm = HookManager(keys=['k'])
        hm.register('k', FixedNegatives(neg_e, None))
        hm.register('k', TimeGapLists(gap))
        vals, offs, starts = [], [0], []
        with hm.activate('k'):
            for b in DGDataLoader(dg, batch_size=bs, hook_manager=hm):
                for lst in b.time_gap_nbrs:
                    vals += lst
                    offs.append(len(vals))
                starts.append(len(offs) - 1)
        out[f'gap{gap}_vals'] = np.array(vals, dtype=np.int32)
        out[f'gap{gap}_offs'] = np.array(offs, dtype=np.int64)
        out[f'gap{gap}_batch_seed0'] = np.array(starts, dtype=np.int64)
    # the stored (time-sorted) stream the windows index, and the raw input it was built from (argsort leaves ties in an order of its own)
    arrays = dict(times=times, edge_event=edge_event, src=src, dst=dst, neg=neg_e.numpy(), raw_ts=ts.numpy(), raw_ei=ei.numpy().astype(np.int32),
                  raw_x=x.numpy(), **out)  # fmt: skip
    if node_events:
        arrays.update(raw_node_t=kw['node_x_time'].numpy(), raw_node_nids=kw['node_x_nids'].numpy().astype(np.int32), raw_node_x=kw['node_x'].numpy())
    save(name, dict(batch_size=bs, gaps=GAPS, num_nodes=N, node_events=node_events, split=split), **arrays)


MIXER_SHAPES = [(2, 1, 0.5, 4.0), (5, 16, 0.5, 4.0), (20, 172, 0.5, 1.5), (30, 200, 1.3, 0.7), (20, 16, 0.9, 1.7), (30, 1, 0.2, 3.0)]


def mixer_cases() -> None:
    """One file per shape (the channel FFN of C = 172 / 200 at expansion 4 alone would pass the committed-file size limit)."""
    for i, (K, C, ft, fc) in enumerate(MIXER_SHAPES):
        torch.manual_seed(100 + i)
        m = MLPMixer(num_tokens=K, num_channels=C, token_dim_expansion_factor=ft, channel_dim_expansion_factor=fc).eval()
        with torch.no_grad():
            for p in m.parameters():  # non-trivial norms / biases
                p.add_(0.1 * torch.randn_like(p))
            x = torch.randn(3, K, C) * 2.0 + 0.5
            y = m(x)
        arrays = {'x': x.numpy(), 'y': y.numpy()}
        for k, v in m.state_dict().items():
            arrays[f'p_{k}'] = v.numpy()
        save(f'g15_graphmixer_mixer_{i}', dict(K=K, C=C, token_expansion=ft, channel_expansion=fc), **arrays)


class ExampleShapedEncoder(nn.Module):
    """The example's encoder layout (parameter names included), forward written out below."""

    def __init__(self, time_dim, embed_dim, num_tokens, node_dim, edge_dim, num_layers, token_dim_expansion, channel_dim_expansion) -> None:
        super().__init__()
        self.time_encoder = Time2Vec(time_dim=time_dim)
        self.projection_layer = nn.Linear(edge_dim + time_dim, edge_dim)
        self.mlp_mixers = nn.ModuleList([MLPMixer(num_tokens, edge_dim, token_dim_expansion, channel_dim_expansion, 0.0) for _ in range(num_layers)])
        self.output_layer = nn.Linear(edge_dim + node_dim, embed_dim)

    def forward(self, nbr_edge_x, seed_times, nbr_edge_time, nbr_nids, seeds, tg_lists, node_feat):
        z = self.projection_layer(torch.cat([nbr_edge_x, self.time_encoder(seed_times[:, None] - nbr_edge_time)], dim=-1))
        for m in self.mlp_mixers:
            z = m(z)
        valid = nbr_nids != -1
        z_link = (z * valid.unsqueeze(-1)).sum(dim=1) / valid.sum(dim=1, keepdim=True).clamp(min=1)
        tg = torch.zeros((len(tg_lists), node_feat.shape[1]))
        for i, lst in enumerate(tg_lists):
            if lst:
                tg[i] = node_feat[lst].mean(dim=0)
        return self.output_layer(torch.cat([z_link, tg + node_feat[seeds]], dim=1))


def encoder_case() -> None:
    torch.manual_seed(7)
    dims = dict(time_dim=8, embed_dim=10, num_tokens=5, node_dim=6, edge_dim=12, num_layers=2, token_dim_expansion=0.5, channel_dim_expansion=4.0)
    enc = ExampleShapedEncoder(**dims).eval()
    bs, N, K = 8, 20, dims['num_tokens']
    S = 3 * bs
    g = torch.Generator().manual_seed(8)
    seeds = torch.randint(0, N, (S,), generator=g)
    seeds[5] = seeds[2]  # a repeated seed
    seed_t = torch.randint(1000, 5000, (S,), generator=g)
    nbr_t = seed_t[:, None] - torch.randint(0, 900, (S, K), generator=g)
    nids = torch.randint(0, N, (S, K), generator=g)
    pad = torch.rand(S, K, generator=g) < 0.3
    pad[0] = True  # a seed without any neighbour
    nids[pad] = -1
    nbr_t[pad] = 0  # padded slots carry what a sampler writes there; they still take part in token mixing
    ex = torch.rand((S, K, dims['edge_dim']), generator=g)
    ex[pad] = 0.0
    node_feat = torch.randn((N, dims['node_dim']), generator=g)
    tg_lists = [torch.randint(0, N, (int(c),), generator=g).tolist() for c in torch.randint(0, 5, (S,), generator=g)]
    tg_lists[1] = []
    with torch.no_grad():
        z = enc(ex, seed_t, nbr_t, nids, seeds, tg_lists, node_feat)
    flat = [v for lst in tg_lists for v in lst]
    offs = np.cumsum([0] + [len(lst) for lst in tg_lists]).astype(np.int64)
    arrays = dict(nbr_edge_x=ex.numpy(), seed_times=seed_t.numpy(), nbr_edge_time=nbr_t.numpy(), nbr_nids=nids.numpy().astype(np.int32),
                  seeds=seeds.numpy().astype(np.int32), tg_vals=np.array(flat, dtype=np.int32), tg_offs=offs, node_feat=node_feat.numpy(),
                  z=z.numpy())  # fmt: skip
    for k, v in enc.state_dict().items():
        arrays[f'p_{k}'] = v.numpy()
    save('g15_graphmixer_encoder', dict(dims=dims, batch_size=bs, state_dict_keys=list(enc.state_dict())), **arrays)


if __name__ == '__main__':
    torch.set_num_threads(1)
    hook_case('g15_graphmixer_hook_plain', 11, 360, 25, 50, node_events=False, split=False)
    hook_case('g15_graphmixer_hook_nodes', 12, 330, 18, 40, node_events=True, split=False)
    hook_case('g15_graphmixer_hook_split', 13, 600, 30, 32, node_events=False, split=True)
    mixer_cases()
    encoder_case()
