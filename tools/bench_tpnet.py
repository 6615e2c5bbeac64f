#!/usr/bin/env python
"""TPNet at the example's shape (wiki-shaped stream, bs 200, k = [32], node 128, edge 172, time 100, embed 172, two mixer layers,
rp_num_layers 2, lambda 1e-6, use_matrix off so dim = 120), with concat_src_dst on and off.  Per batch, in microseconds:

  update                 ``RandomProjectionModule.update`` alone (the native call), and the reference's update composed from torch ops
                         (rescale, gather, two scatter_add_ per level) on the same device
  pair_features          the pair-feature kernel alone at the encoder's shape (4 B k items: neighbour x source, neighbour x destination),
                         by device events, with its algorithmic bytes (the gathered rows it must read + the output) against the HBM spec
  forward                the encoder, positive and negative call together as the example's step makes them: ``encode_pairs`` (hop 0 read in
                         place), ``forward`` on gathered tensors (the gathers timed with it), and composed from torch ops on the device

A timed window loops over the batch list until it lasts at least --window-s seconds; the variants of one figure take turns (one window
each, three rounds, after a warm-up window each) and each figure is the median of its three windows.  Prints one JSON line per setting.
    python tools/bench_tpnet.py [--edges E] [--batches B]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgm_amd import DGData, DGDataLoader, DGraph  # noqa: E402
from tgm_amd.hooks import HookManager, RandomNegativeEdgeSamplerHook, RecencyNeighborHook  # noqa: E402
from tgm_amd.nn import RandomProjectionModule, TPNet  # noqa: E402
from tgm_amd.synth import make_stream  # noqa: E402

HBM_TBS = 8.0  # MI355X HBM3E spec

ap = argparse.ArgumentParser()
ap.add_argument('--edges', type=int, default=60_000)
ap.add_argument('--batches', type=int, default=40, help='distinct batches a timed window loops over')
ap.add_argument('--window-s', type=float, default=0.5, help='least duration of a timed window')
args = ap.parse_args()

dev = torch.device('cuda', 0)
bs, K, dN, dT, E_, NL, RPL, LAM = 200, 32, 128, 100, 172, 2, 2, 1e-6
RP_EDGES = 110_000  # tgbl-wiki's training edges, whatever --edges is: dim = int(log(2 E)) * 10 = 120
s = make_stream('wiki', num_edges=args.edges)
N, dE = s.num_nodes, s.edge_x.shape[1]
dg = DGraph(DGData.from_raw(s.ts, torch.stack([s.src, s.dst], 1), s.edge_x), device=dev)
node_x = torch.randn(N, dN, device=dev)
hm = HookManager(keys=['k'])
hm.register('k', RandomNegativeEdgeSamplerHook(low=0, high=N))
hm.register('k', RecencyNeighborHook(N, [K], ['edge_src', 'edge_dst', 'neg'], ['edge_time', 'edge_time', 'neg_time']))
with hm.activate('k'):
    batches = list(DGDataLoader(dg, batch_size=bs, hook_manager=hm))
full = [b for b in batches if b.edge_src.numel() == bs]
work = full[-args.batches :]  # steady state: full neighbour windows
assert all(t.dtype == torch.int32 and t.is_contiguous() for b in work for t in (b.nbr_nids[0], b.edge_src, b.edge_dst, b.neg))  # passed to the kernel as they are
ar = torch.arange(bs, device=dev, dtype=torch.int32)
ROWS = {False: (ar, ar + bs), True: (ar, ar + 2 * bs)}


def window(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * len(work)) * 1e6


def alternating_medians(fns):
    """Warm each up (which also sizes its window), then one window each in turn, three rounds: drift of the device hits all alike."""
    for fn in fns:
        window(fn)  # warm-up (first-call costs would undersize the window below)
    reps = [max(1, math.ceil(args.window_s * 1.1e6 / (window(fn) * len(work)))) for fn in fns]
    seen = [[] for _ in fns]
    for _ in range(3):
        for i, fn in enumerate(fns):
            seen[i].append(window(fn, reps[i]))
    return [statistics.median(v) for v in seen], [[round(x, 1) for x in v] for v in seen]


def torch_update(tabs, now, src, dst, t):
    """The reference's update from torch ops on the device (float atomics inside scatter_add_)."""
    nxt = t[-1].unsqueeze(0)
    w = torch.exp(-LAM * (nxt - t))[:, None]
    for i in range(1, RPL + 1):
        tabs[i] = tabs[i] * torch.pow(torch.exp(-LAM * (nxt - now)), i)
    src, dst = src.long(), dst.long()
    for i in range(RPL, 0, -1):
        ms, md = tabs[i - 1][dst] * w, tabs[i - 1][src] * w
        tabs[i].scatter_add_(0, src[:, None].expand(-1, ms.shape[1]), ms)
        tabs[i].scatter_add_(0, dst[:, None].expand(-1, md.shape[1]), md)
    return nxt


def run(concat: bool) -> dict:
    torch.manual_seed(0)
    rp = RandomProjectionModule(N, RPL, LAM, int(s.ts[0]), use_matrix=False, num_edges=RP_EDGES, dim_factor=10, concat_src_dst=concat)
    enc = TPNet(node_feat_dim=dN, edge_x_dim=dE, time_feat_dim=dT, output_dim=E_, num_neighbors=K, num_layers=NL, dropout=0.1, random_projections=rp,
                device=dev).to(dev).eval()  # fmt: skip
    p0 = rp.random_projections[0]

    def warm_state():
        rp.reset_random_projections(reset_zero=False)
        for b in full:  # the whole stream: the tables the timed forwards read are the stream's
            rp.update(b.edge_src, b.edge_dst, b.edge_time)

    # -- update ------------------------------------------------------------------------------------------------------------------------
    def native_updates():
        rp.reset_random_projections(reset_zero=False)
        for b in work:
            rp.update(b.edge_src, b.edge_dst, b.edge_time)

    tt = {}

    def torch_updates():
        tt['tabs'] = [p0] + [torch.zeros_like(p0) for _ in range(RPL)]
        now = rp.beginning_time.data
        for b in work:
            now = torch_update(tt['tabs'], now, b.edge_src, b.edge_dst, b.edge_time)

    with torch.no_grad():
        (upd_us, upd_torch_us), upd_seen = alternating_medians([native_updates, torch_updates])
        native_updates()
        agree = max(float(((rp.random_projections[i] - tt['tabs'][i]).abs() / tt['tabs'][i].abs().clamp(min=1)).max()) for i in range(1, RPL + 1))
        warm_state()

    # -- the pair-feature kernel alone, at the encoder's shape ----------------------------------------------------------------------------
    od, ld, R = rp.out_dim, (rp.out_dim + 3) // 4 * 4, 2 * bs * K
    feat = torch.empty((2 * R, ld), dtype=torch.float32, device=dev)
    rows = [torch.cat(ROWS[neg]) for neg in (False, True)]

    def pair_kernel(b, neg):
        rp._pair_features(b.nbr_nids[0], rows[neg], b.nbr_nids[0].shape[0], K, b.edge_src, b.neg if neg else b.edge_dst, bs, R, feat, ld)

    def pair_event_us():
        for b in work:  # warm-up
            pair_kernel(b, False)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(5):
            for b in work:
                pair_kernel(b, False)
                pair_kernel(b, True)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / (5 * len(work))

    pair_seen = [pair_event_us() for _ in range(3)]
    pair_us = statistics.median(pair_seen)  # both calls of a batch
    pair_bytes = 2 * (2 * R * (2 * (RPL + 1) * rp.dim * 4 + od * 4))  # per batch: every item reads 2 (L + 1) rows and writes out_dim floats

    # -- forward -----------------------------------------------------------------------------------------------------------------------
    def each(fn):
        def go():
            for b in work:
                fn(b, False)
                fn(b, True)
        return go

    def pairs(b, neg):
        sr, dr = ROWS[neg]
        return enc.encode_pairs(node_x, b.edge_src, b.neg if neg else b.edge_dst, b.edge_time, b.nbr_nids[0], b.nbr_edge_time[0], b.nbr_edge_x[0], sr, dr)

    def gathered(b, neg):
        r = rows[neg].long()
        return enc(node_x, torch.stack([b.edge_src, b.neg if neg else b.edge_dst]), b.edge_time, b.nbr_nids[0][r], b.nbr_edge_time[0][r], b.nbr_edge_x[0][r])

    def composed(b, neg):
        sr, dr = ROWS[neg]
        return enc._torch_forward(enc._inputs(node_x, b.edge_src, b.neg if neg else b.edge_dst, b.edge_time, b.nbr_nids[0], b.nbr_edge_time[0],
                                              b.nbr_edge_x[0], sr, dr))  # fmt: skip

    with torch.no_grad():
        (pairs_us, gathered_us, torch_us), fwd_seen = alternating_medians([each(pairs), each(gathered), each(composed)])
        zn, zc = pairs(work[-1], True), composed(work[-1], True)
        fwd_agree = max(float(((a - c).abs() / c.abs().clamp(min=1)).max()) for a, c in zip(zn, zc))
    return {
        'bench': 'tpnet_example_shape', 'concat_src_dst': concat, 'device': torch.cuda.get_device_name(0), 'edges': args.edges, 'num_nodes': N,
        'batches_timed': len(work), 'bs': bs, 'k': K, 'rp_dim': rp.dim, 'rp_out_dim': od,
        'update_us_per_batch': round(upd_us, 1), 'torch_update_us_per_batch': round(upd_torch_us, 1), 'update_speedup_vs_torch': round(upd_torch_us / upd_us, 2),
        'update_windows_us': upd_seen, 'update_native_vs_torch_max_rel_diff': agree,
        'pair_kernel_us_per_batch': round(pair_us, 1), 'pair_kernel_runs_us': [round(x, 1) for x in pair_seen], 'pair_kernel_mbytes_per_batch': round(pair_bytes / 1e6, 1),
        'pair_kernel_fraction_of_hbm_spec': round(pair_bytes / (pair_us * 1e-6) / (HBM_TBS * 1e12), 3),
        'forward_encode_pairs_us_per_batch': round(pairs_us, 1), 'forward_gathered_us_per_batch': round(gathered_us, 1),
        'torch_composed_forward_us_per_batch': round(torch_us, 1), 'native_speedup_vs_torch': round(torch_us / pairs_us, 2),
        'forward_windows_us': fwd_seen, 'forward_native_vs_torch_max_rel_diff': fwd_agree,
    }  # fmt: skip


for concat in (True, False):
    print(json.dumps(run(concat)), flush=True)
