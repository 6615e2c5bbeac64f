#!/usr/bin/env python
"""Generate the DyGFormer fixtures tests/golden/g16_dygformer_*.npz by running the REFERENCE.

Runs only where the reference checkout is (PyG is replaced by the names-only placeholder in tests/golden/_pyg_stub).  It imports the
reference's ``DyGFormer``, ``NeighborCooccurrenceEncoder`` and ``TransformerEncoder``, runs them on the CPU in float32 with ``eval()`` and
fixed seeds, and writes plain .npz data: inputs, the ``state_dict`` arrays (for the example's dimensions the seed of
``dygformer_restate.hashed_state_dict`` instead: the weights alone would pass the committed-file size limit) and the reference's outputs.

    python tests/golden/make_golden_dygformer.py

  g16_dygformer_counts_{L}      co-occurrence counts: repeated neighbours, a seed inside its own and the other list, all-pad rows, src == dst
  g16_dygformer_cooc            the co-occurrence encoder
  g16_dygformer_layer_{i}       one TransformerEncoder layer (heads 1 / 2 / 4, head dimensions 8, 25, 100)
  g16_dygformer_small_p{ps}     the full encoder at small dims, patch sizes 1, 2, 4, padded slots (time gaps < 1e4: with only 8 time
                                channels the float32 rounding of w dt is not averaged down as it is over the example's 100)
  g16_dygformer_single          P = 1
  g16_dygformer_longgap         time gaps up to 1e6 (the one fixture outside the 1e5 range)
  g16_dygformer_example         the example's dims (L 32, C 50, two heads, two layers, node 128, edge 172, time 100, out 172)
  g16_dygformer_self_noise.json for every float fixture (co-occurrence encoder, layers, encoders) the distance of the reference's float32 output from the float64
                                restatement, max |a - b| / max(1, |b|); plus the study of that distance against the time-gap range
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
from tgm.nn.encoder.dygformer import DyGFormer, NeighborCooccurrenceEncoder, TransformerEncoder  # noqa: E402

import dygformer_restate as dr  # noqa: E402

NOISE = {}


def save(name: str, meta: dict, **arrays) -> None:
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(f'{name}: {os.path.getsize(path)} bytes')


def id_sequences(g, P, L, N, pad_frac):
    """[P, L] source / destination sequences (slot 0 = the seed) with heavy repetition and the corner cases."""
    s = torch.randint(0, N, (P, L), generator=g)
    d = torch.randint(0, N, (P, L), generator=g)
    for a in (s, d):
        a[:, 1:][torch.rand(P, L - 1, generator=g) < pad_frac] = -1
    if P >= 6 and L >= 2:
        s[0, 1:] = s[0, 0]  # the seed fills its own list
        d[0, L // 2] = s[0, 0]  # ... and sits in the other side's
        s[1, 1:] = -1  # all pads
        d[1, 1:] = -1
        d[2] = s[2]  # src == dst, same neighbours
        d[3, 0] = s[3, 0]  # src == dst, different neighbours
        s[4, 1:] = -1  # one side padded only
        s[5, L - 1] = d[5, 0]  # the destination seed among the source's neighbours
    return s, d


def counts_cases() -> None:
    for L in (2, 5, 32, 64):
        g = torch.Generator().manual_seed(1600 + L)
        s, d = id_sequences(g, 12, L, max(3, L // 3), 0.25)
        enc = NeighborCooccurrenceEncoder(4, 'cpu')
        fs, fd = enc._count_nodes_freq(s, d)
        save(f'g16_dygformer_counts_{L}', dict(L=L), src_seq=s.numpy().astype(np.int32), dst_seq=d.numpy().astype(np.int32),
             src_counts=fs.numpy().astype(np.int32), dst_counts=fd.numpy().astype(np.int32))  # fmt: skip


def cooc_case() -> None:
    torch.manual_seed(1610)
    g = torch.Generator().manual_seed(1611)
    enc = NeighborCooccurrenceEncoder(10, 'cpu').eval()
    s, d = id_sequences(g, 9, 16, 6, 0.3)
    with torch.no_grad():
        fs, fd = enc(s, d)
    cs, cd = dr.cooccurrence_counts(s.numpy(), d.numpy())
    r64 = [dr.cooccurrence_encode(enc.state_dict(), 'neighbor_co_occurrence_encoder.', torch.from_numpy(c)) for c in (cs, cd)]
    NOISE['g16_dygformer_cooc'] = max(dr.rel_err(fs, r64[0]), dr.rel_err(fd, r64[1]))
    arrays = {f'p_{k}': v.numpy() for k, v in enc.state_dict().items()}
    save('g16_dygformer_cooc', dict(feat_dim=10), src_seq=s.numpy().astype(np.int32), dst_seq=d.numpy().astype(np.int32), src_feat=fs.numpy(),
         dst_feat=fd.numpy(), **arrays)  # fmt: skip


LAYER_SHAPES = [(8, 1, 6, 5), (16, 2, 10, 3), (50, 2, 64, 3), (32, 4, 16, 4), (100, 4, 7, 2), (200, 2, 64, 2)]  # (d, heads, T, B)


def layer_cases() -> None:
    for i, (d, H, T, B) in enumerate(LAYER_SHAPES):
        torch.manual_seed(1620 + i)
        m = TransformerEncoder(d, H, dropout=0.1).eval()
        meta = dict(attention_dim=d, num_heads=H)
        with torch.no_grad():
            if d >= 100:  # too large to store: hashed weights, the seed recorded
                meta.update(weights_seed=1620 + i, shapes={k: list(v.shape) for k, v in m.state_dict().items()})
                m.load_state_dict(dr.hashed_state_dict(meta['shapes'], 1620 + i), strict=True)
            else:
                for p in m.parameters():
                    p.add_(0.05 * torch.randn_like(p))
            x = torch.randn(B, T, d) * 1.5 + 0.3
            y = m(x)
        sd = m.state_dict()
        meta['state_dict_keys'] = list(sd)
        NOISE[f'g16_dygformer_layer_{i}'] = dr.rel_err(y, dr.transformer_layer(sd, '', x.double(), H))
        arrays = {} if d >= 100 else {f'p_{k}': v.numpy() for k, v in sd.items()}
        save(f'g16_dygformer_layer_{i}', meta, x=x.numpy(), y=y.numpy(), **arrays)


def encoder_inputs(g, P, L, N, dN, dE, max_gap, pad_frac):
    s, d = id_sequences(g, P, L, N, pad_frac)
    ids = torch.cat([s, d])
    src, dst, nids = s[:, 0].clone(), d[:, 0].clone(), ids[:, 1:].clone()
    edge_time = torch.randint(max_gap, 2 * max_gap, (P,), generator=g)
    t2 = torch.cat([edge_time, edge_time])
    nbr_t = t2[:, None] - torch.randint(0, max_gap, (2 * P, L - 1), generator=g)
    nbr_t[nids == -1] = 0  # what the sampler leaves in a padded slot
    ex = torch.rand((2 * P, L - 1, dE), generator=g)
    ex[nids == -1] = 0.0
    ex[0, -1] = 0.5  # edge features of a padded slot are taken as they come
    node_x = torch.randn((N, dN), generator=g)
    return dict(node_x=node_x, src=src, dst=dst, edge_time=edge_time, nbr_nids=nids, nbr_time=nbr_t, nbr_edge_x=ex)


def run_encoder(dims, inp, sd=None, seed=0):
    torch.manual_seed(seed)
    m = DyGFormer(**dims).eval()
    with torch.no_grad():
        if sd is not None:
            m.load_state_dict(sd, strict=True)
        else:
            for n, p in m.named_parameters():
                if not n.startswith('time_encoder.w.weight'):
                    p.add_(0.05 * torch.randn_like(p))
        zs, zd = m(inp['node_x'], torch.stack([inp['src'], inp['dst']]), inp['edge_time'], inp['nbr_nids'], inp['nbr_time'], inp['nbr_edge_x'])
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    rs, rd = dr.dygformer_forward(sd, dims['patch_size'], dims['num_layers'], dims['num_heads'], inp['node_x'], inp['src'], inp['dst'], inp['edge_time'],
                                  inp['nbr_nids'], inp['nbr_time'], inp['nbr_edge_x'])  # fmt: skip
    return sd, zs, zd, max(dr.rel_err(zs, rs), dr.rel_err(zd, rd))


def encoder_case(name, dims, P, N, max_gap, pad_frac, seed, hashed=False) -> None:
    g = torch.Generator().manual_seed(seed)
    inp = encoder_inputs(g, P, dims['max_input_sequence_length'], N, dims['node_feat_dim'], dims['edge_x_dim'], max_gap, pad_frac)
    meta = dict(dims=dims, max_gap=max_gap)
    sd0 = None
    if hashed:
        torch.manual_seed(0)
        shapes = {k: list(v.shape) for k, v in DyGFormer(**dims).state_dict().items()}
        meta.update(weights_seed=seed, shapes=shapes)
        sd0 = dr.hashed_state_dict(shapes, seed)
    sd, zs, zd, noise = run_encoder(dims, inp, sd0, seed)
    NOISE[name] = noise
    meta['state_dict_keys'] = list(sd)
    arrays = dict(node_x=inp['node_x'].numpy(), src=inp['src'].numpy().astype(np.int32), dst=inp['dst'].numpy().astype(np.int32),
                  edge_time=inp['edge_time'].numpy(), nbr_nids=inp['nbr_nids'].numpy().astype(np.int32), nbr_time=inp['nbr_time'].numpy(),
                  nbr_edge_x=inp['nbr_edge_x'].numpy(), z_src=zs.numpy(), z_dst=zd.numpy())  # fmt: skip
    if not hashed:
        arrays.update({f'p_{k}': v.numpy() for k, v in sd.items()})
    save(name, meta, **arrays)


EXAMPLE = dict(node_feat_dim=128, edge_x_dim=172, time_feat_dim=100, channel_embedding_dim=50, output_dim=172, patch_size=1, num_layers=2,
               num_heads=2, dropout=0.1, max_input_sequence_length=32)  # fmt: skip
SMALL = dict(node_feat_dim=6, edge_x_dim=5, time_feat_dim=8, channel_embedding_dim=4, output_dim=7, num_layers=2, num_heads=2, dropout=0.1)


def noise_study() -> dict:
    """The reference's float32 forward against float64 as the time gaps grow (example dims, P 16, 30 % pads; zero and random Time2Vec
    bias), and one small case (L 64, patch 4, C 16, gaps < 1e6)."""
    out = {}
    shapes = None
    for max_gap in (10**3, 10**5, 10**6):
        for bias in ('zero', 'random'):
            vals = []
            for rep in range(3):
                g = torch.Generator().manual_seed(1700 + rep)
                inp = encoder_inputs(g, 16, 32, 60, 128, 172, max_gap, 0.3)
                if shapes is None:
                    shapes = {k: list(v.shape) for k, v in DyGFormer(**EXAMPLE).state_dict().items()}
                sd = dr.hashed_state_dict(shapes, 1700 + rep)
                if bias == 'zero':
                    sd['time_encoder.w.bias'] = torch.zeros_like(sd['time_encoder.w.bias'])
                vals.append(run_encoder(EXAMPLE, inp, sd)[3])
            out[f'example_dims_gap_lt_{max_gap:g}_bias_{bias}'] = [min(vals), max(vals)]
    dims = dict(SMALL, channel_embedding_dim=16, patch_size=4, max_input_sequence_length=64)
    g = torch.Generator().manual_seed(1710)
    out['small_L64_patch4_C16_gap_lt_1e+06'] = run_encoder(dims, encoder_inputs(g, 16, 64, 40, 6, 5, 10**6, 0.3), None, 1710)[3]
    return out


if __name__ == '__main__':
    torch.set_num_threads(1)
    counts_cases()
    cooc_case()
    layer_cases()
    for ps in (1, 2, 4):
        encoder_case(f'g16_dygformer_small_p{ps}', dict(SMALL, patch_size=ps, max_input_sequence_length=8), 7, 12, 10**4, 0.35, 1630 + ps)
    encoder_case('g16_dygformer_single', dict(SMALL, patch_size=2, max_input_sequence_length=6, num_heads=1), 1, 5, 10**4, 0.3, 1640)
    encoder_case('g16_dygformer_longgap', dict(SMALL, patch_size=4, max_input_sequence_length=64, channel_embedding_dim=16), 6, 40, 10**6, 0.3, 1650)
    encoder_case('g16_dygformer_example', EXAMPLE, 6, 60, 10**5, 0.3, 1660, hashed=True)
    with open(os.path.join(HERE, 'g16_dygformer_self_noise.json'), 'w') as f:
        json.dump(dict(fixtures=NOISE, study=noise_study()), f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(NOISE, indent=1))
