"""DyGFormer without a GPU: import paths, the CPU restatement against every reference fixture, the state_dict layout, constructor
validation, the sequence-length check and the no-CPU-fallback contract."""
import json
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR, load
import dygformer_restate as dr

COUNT_CASES = [f'g16_dygformer_counts_{L}' for L in (2, 5, 32, 64)]
LAYER_CASES = [f'g16_dygformer_layer_{i}' for i in range(6)]
ENCODER_CASES = ['g16_dygformer_small_p1', 'g16_dygformer_small_p2', 'g16_dygformer_small_p4', 'g16_dygformer_single', 'g16_dygformer_longgap',
                 'g16_dygformer_example']  # fmt: skip
NOISE = json.load(open(os.path.join(GOLDEN_DIR, 'g16_dygformer_self_noise.json')))


def fixture_state_dict(meta, a):
    """The fixture's weights: stored arrays, or regenerated from the recorded seed (models too large to store)."""
    if 'weights_seed' in meta:
        return dr.hashed_state_dict(meta['shapes'], meta['weights_seed'])
    return {k[2:]: torch.from_numpy(v) for k, v in a.items() if k.startswith('p_')}


def encoder_inputs(a):
    T = torch.from_numpy
    return dict(node_x=T(a['node_x']), src=T(a['src']), dst=T(a['dst']), edge_time=T(a['edge_time']), nbr_nids=T(a['nbr_nids']), nbr_time=T(a['nbr_time']),
                nbr_edge_x=T(a['nbr_edge_x']))  # fmt: skip


def restated(meta, a, sd, dtype=torch.float64):
    d, i = meta['dims'], encoder_inputs(a)
    return dr.dygformer_forward(sd, d['patch_size'], d['num_layers'], d['num_heads'], i['node_x'], i['src'], i['dst'], i['edge_time'], i['nbr_nids'],
                                i['nbr_time'], i['nbr_edge_x'], dtype=dtype)  # fmt: skip


def test_import_paths():
    from tgm_amd.nn import DyGFormer, NeighborCooccurrenceEncoder, TransformerEncoder
    from tgm_amd.nn.encoder import DyGFormer as D2
    from tgm_amd.nn.encoder.dygformer import DyGFormer as D3

    assert DyGFormer is D2 is D3 and DyGFormer.__module__ == 'tgm_amd.nn.dygformer'
    assert NeighborCooccurrenceEncoder.__module__ == TransformerEncoder.__module__ == 'tgm_amd.nn.dygformer'


@pytest.mark.parametrize('name', COUNT_CASES)
def test_restated_counts_match_the_reference(name):
    _, a = load(name)
    cs, cd = dr.cooccurrence_counts(a['src_seq'], a['dst_seq'])
    assert np.array_equal(cs, a['src_counts']) and np.array_equal(cd, a['dst_counts'])


def test_restated_cooccurrence_encoder_matches_the_reference():
    _, a = load('g16_dygformer_cooc')
    sd = {k[2:]: torch.from_numpy(v) for k, v in a.items() if k.startswith('p_')}
    cs, cd = dr.cooccurrence_counts(a['src_seq'], a['dst_seq'])
    for c, want in ((cs, a['src_feat']), (cd, a['dst_feat'])):
        assert dr.rel_err(torch.from_numpy(want), dr.cooccurrence_encode(sd, 'neighbor_co_occurrence_encoder.', torch.from_numpy(c))) < 1e-5
    pad = a['src_seq'] == -1
    assert pad.any()  # a padded slot is not zero: both counts are 0 and still go through the encoder
    w = lambda n: sd[f'neighbor_co_occurrence_encoder.{n}'].double()
    e0 = 2 * (w('2.weight') @ torch.relu(w('0.bias')) + w('2.bias'))
    assert dr.rel_err(torch.from_numpy(a['src_feat'][pad]), e0.expand(int(pad.sum()), -1)) < 1e-5


@pytest.mark.parametrize('name', LAYER_CASES)
def test_restated_layer_matches_the_reference(name):
    from tgm_amd.nn import TransformerEncoder

    meta, a = load(name)
    sd = fixture_state_dict(meta, a)
    m = TransformerEncoder(meta['attention_dim'], meta['num_heads'])
    assert list(m.state_dict()) == meta['state_dict_keys']
    m.load_state_dict(sd, strict=True)
    err = dr.rel_err(torch.from_numpy(a['y']), dr.transformer_layer(sd, '', torch.from_numpy(a['x']).double(), meta['num_heads']))
    assert err < 1e-5 and abs(err - NOISE['fixtures'][name]) < 1e-12


@pytest.mark.parametrize('name', ENCODER_CASES)
def test_restated_encoder_matches_the_reference_and_the_layout(name):
    from tgm_amd.nn import DyGFormer

    meta, a = load(name)
    sd = fixture_state_dict(meta, a)
    m = DyGFormer(**meta['dims'])
    assert list(m.state_dict()) == meta['state_dict_keys'] == list(sd)
    m.load_state_dict(sd, strict=True)
    zs, zd = restated(meta, a, sd)
    err = max(dr.rel_err(torch.from_numpy(a['z_src']), zs), dr.rel_err(torch.from_numpy(a['z_dst']), zd))
    noise = NOISE['fixtures'][name]
    print(f'{name}: reference float32 vs float64 restatement {err:.3e} (recorded {noise:.3e})')
    assert abs(err - noise) <= 1e-9 + 1e-3 * noise  # the recorded self-noise is this distance
    assert err < (1e-4 if meta['max_gap'] <= 10**5 else 2e-3)
    # The float32 restatement is the reference's stand-in where the reference is not installed (the end-to-end GPU case).  It takes the same
    # float32 Time2Vec argument, so it must land on the reference's own float32 output up to summation order (~ sqrt(K) 2^-24 over the
    # K <= 800-term contractions of O(1) values: 2e-6), and its distance from float64 must be the reference's, not a multiple of it.
    z32 = restated(meta, a, sd, dtype=torch.float32)
    e32 = max(dr.rel_err(z32[0], zs), dr.rel_err(z32[1], zd))
    efix = max(dr.rel_err(z32[0], torch.from_numpy(a['z_src'])), dr.rel_err(z32[1], torch.from_numpy(a['z_dst'])))
    print(f'{name}: float32 restatement vs float64 {e32:.3e}, vs the reference float32 output {efix:.3e}')
    assert efix < 2e-6
    assert abs(e32 - noise) <= 0.1 * noise + 2e-6


def test_state_dict_key_families():
    from tgm_amd.nn import DyGFormer

    keys = set(DyGFormer(4, 3, 6, 5, output_dim=7, patch_size=2, num_layers=1, max_input_sequence_length=8).state_dict())
    want = {'time_encoder.w.weight', 'time_encoder.w.bias', 'output_layer.weight', 'output_layer.bias'}
    want |= {f'co_occurrence_encoder.neighbor_co_occurrence_encoder.{i}.{p}' for i in (0, 2) for p in ('weight', 'bias')}
    want |= {f'projection_layer.{c}.{p}' for c in ('node', 'edge', 'time', 'neighbor_co_occurrence') for p in ('weight', 'bias')}
    want |= {f'transformers.0.multi_head_attention.{p}' for p in ('in_proj_weight', 'in_proj_bias', 'out_proj.weight', 'out_proj.bias')}
    want |= {f'transformers.0.{m}.{i}.{p}' for m in ('linear_layers', 'norm_layers') for i in (0, 1) for p in ('weight', 'bias')}
    assert keys == want


def test_constructor_errors():
    from tgm_amd.nn import DyGFormer

    with pytest.raises(ValueError, match='multiple'):
        DyGFormer(4, 3, 6, 5, patch_size=3, max_input_sequence_length=8)
    with pytest.raises(NotImplementedError):
        DyGFormer(4, 3, 6, 5, num_channels=3)
    m = DyGFormer(4, 3, 6, 5)  # the reference's defaults
    assert (m.patch_size, m.max_input_sequence_length, m.num_patches, m.num_channels, m.output_layer.out_features) == (1, 512, 512, 4, 172)
    assert len(m.transformers) == 2 and m.transformers[0].num_heads == 2 and m.transformers[0].dropout_rate == 0.1


def test_sequence_length_must_equal_max_input_sequence_length_and_cpu_tensors_raise():
    from tgm_amd.exceptions import NativeLibraryError
    from tgm_amd.nn import DyGFormer, NeighborCooccurrenceEncoder, TransformerEncoder

    m = DyGFormer(4, 3, 6, 5, max_input_sequence_length=8).eval()
    P = 2
    args = lambda k: (torch.zeros(9, 4), torch.zeros(2, P, dtype=torch.int64), torch.zeros(P, dtype=torch.int64), torch.zeros(2 * P, k, dtype=torch.int64),
                      torch.zeros(2 * P, k, dtype=torch.int64), torch.zeros(2 * P, k, 3))  # fmt: skip
    with pytest.raises(NativeLibraryError):
        m(*args(7))
    with pytest.raises(NativeLibraryError):
        NeighborCooccurrenceEncoder(4, 'cpu')(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(NativeLibraryError):
        TransformerEncoder(8, 2).eval()(torch.zeros(1, 4, 8))
    for k in (5, 8):  # shapes are validated before anything touches the device
        with pytest.raises(ValueError, match='max_input_sequence_length'):
            m(*args(k))
