"""TPNet without a GPU: import paths, the float64 restatement against every reference fixture (and the recorded self-noise), the
constructor and ``dim`` rule, the state_dict layout and dtypes, ``reload_random_projections``' errors and the no-CPU-fallback contract."""
import json
import os

import pytest
import torch

from golden_util import GOLDEN_DIR, load
import tpnet_restate as tr

UPDATE_CASES = [f'g17_tpnet_update_{n}' for n in ('rand_l2', 'matrix_l3', 'rand_l1')]
PAIR_CASES = [f'g17_tpnet_pair_{n}' for n in ('concat_scale', 'concat_raw', 'cross_scale', 'cross_raw', 'matrix', 'dim1', 'dim7_l1', 'dim90_l3',
                                              'dim120_factor', 'dim300')]  # fmt: skip
ENCODER_CASES = [f'g17_tpnet_enc_{n}' for n in ('small', 'small_norp', 'small_cross', 'padheavy', 'single', 'example')]
NOISE = json.load(open(os.path.join(GOLDEN_DIR, 'g17_tpnet_self_noise.json')))


def rp_kwargs(cfg: dict) -> dict:
    return dict(num_nodes=cfg['num_nodes'], num_layer=cfg['num_layer'], time_decay_weight=cfg['lam'], beginning_time=cfg['beginning_time'],
                use_matrix=cfg['use_matrix'], scale_random_projection=cfg.get('scale', True), enforce_dim=cfg.get('enforce_dim'),
                num_edges=cfg.get('num_edges'), dim_factor=cfg.get('dim_factor'), concat_src_dst=cfg.get('concat', True))  # fmt: skip


def fixture_state_dict(meta, a):
    """The fixture's weights: stored arrays, or regenerated from the recorded seed (models too large to store)."""
    if 'weights_seed' in meta:
        return tr.hashed_state_dict(meta['shapes'], meta['dtypes'], meta['weights_seed'])
    return {k[2:]: torch.from_numpy(v) for k, v in a.items() if k.startswith('p_')}


def encoder_inputs(a):
    T = torch.from_numpy
    return dict(node_x=T(a['node_x']), src=T(a['src']), dst=T(a['dst']), edge_time=T(a['edge_time']), nbr_nids=T(a['nbr_nids']), nbr_time=T(a['nbr_time']),
                nbr_edge_x=T(a['nbr_edge_x']))  # fmt: skip


def rp_dict(cfg):
    return None if cfg is None else dict(num_layer=cfg['num_layer'], concat=cfg.get('concat', True), scale=cfg.get('scale', True))


def restated(meta, a, sd, dtype=torch.float64):
    i = encoder_inputs(a)
    return tr.tpnet_forward(sd, meta['dims']['num_layers'], rp_dict(meta['cfg']), i['node_x'], i['src'], i['dst'], i['edge_time'], i['nbr_nids'],
                            i['nbr_time'], i['nbr_edge_x'], dtype=dtype)  # fmt: skip


def restated_stream(meta, a, upto=None):
    """The float64 tables after the fixture's batches [0, upto)."""
    cfg = meta['cfg']
    p0 = torch.from_numpy(a['p0'])
    tabs, now = [p0.double()] + [torch.zeros_like(p0, dtype=torch.float64) for _ in range(cfg['num_layer'])], cfg['beginning_time']
    for b in range(a['src'].shape[0] if upto is None else upto):
        tabs, now = tr.rp_update(tabs, now, a['src'][b], a['dst'][b], a['time'][b], cfg['lam'])
    return tabs, now


def build_model(meta):
    from tgm_amd.nn import TPNet, RandomProjectionModule

    rp = None if meta['cfg'] is None else RandomProjectionModule(**rp_kwargs(meta['cfg']))
    return TPNet(**meta['dims'], random_projections=rp)


def test_import_paths():
    from tgm_amd.nn import RandomProjectionModule, TPNet
    from tgm_amd.nn.encoder import TPNet as T2
    from tgm_amd.nn.encoder.tpnet import RandomProjectionModule as R3, TPNet as T3

    assert TPNet is T2 is T3 and RandomProjectionModule is R3 and TPNet.__module__ == 'tgm_amd.nn.tpnet'


@pytest.mark.parametrize('name', UPDATE_CASES)
def test_restated_update_matches_the_reference(name):
    meta, a = load(name)
    tabs, now = restated_stream(meta, a)
    assert a['src'].shape[0] >= 30 and now == meta['now']
    err = max(tr.rel_err(torch.from_numpy(a[f'table_{i}']), tabs[i]) for i in range(1, meta['cfg']['num_layer'] + 1))
    noise = NOISE['fixtures'][name]
    print(f'{name}: reference float32 vs float64 restatement {err:.3e} (recorded {noise:.3e})')
    assert err < 1e-5 and abs(err - noise) <= 1e-9 + 1e-3 * noise
    # the stream holds what it promises: duplicate targets, a self-loop, a node on both sides, ties, a batch with next == now
    s, d, t = a['src'], a['dst'], a['time']
    assert (s[1] == d[1]).any() and len(set(s[2].tolist())) < s.shape[1] and set(s[2].tolist()) & set(d[2].tolist())
    assert (t[:, 1:] == t[:, :-1]).any() and t[5, -1] == t[4, -1] and (t.reshape(-1)[1:] >= t.reshape(-1)[:-1]).all()


@pytest.mark.parametrize('name', PAIR_CASES)
def test_restated_pair_features_match_the_reference(name):
    from tgm_amd.nn import RandomProjectionModule

    meta, a = load(name)
    cfg = meta['cfg']
    sd = fixture_state_dict(meta, a)
    m = RandomProjectionModule(**rp_kwargs(cfg))
    assert (m.dim, m.out_dim) == (meta['dim'], meta['out_dim']) and list(m.state_dict()) == meta['state_dict_keys']
    assert {k: str(v.dtype)[6:] for k, v in m.state_dict().items()} == meta['dtypes']
    m.load_state_dict(sd, strict=True)  # (the reference's now_time has shape [1] after an update)
    assert (a['a'] == -1).any() and (a['b'] == -1).any()
    err = tr.rel_err(torch.from_numpy(a['out']), tr.rp_forward(sd, '', cfg['num_layer'], a['a'], a['b'], cfg.get('concat', True), cfg.get('scale', True)))
    noise = NOISE['fixtures'][name]
    print(f'{name}: reference float32 vs float64 restatement {err:.3e} (recorded {noise:.3e})')
    assert err < 1e-5 and abs(err - noise) <= 1e-9 + 1e-3 * noise


@pytest.mark.parametrize('name', ENCODER_CASES)
def test_restated_encoder_matches_the_reference_and_the_layout(name):
    meta, a = load(name)
    sd = fixture_state_dict(meta, a)
    m = build_model(meta)
    assert list(m.state_dict()) == meta['state_dict_keys'] == list(sd)
    assert {k: str(v.dtype)[6:] for k, v in m.state_dict().items()} == meta['dtypes']
    m.load_state_dict(sd, strict=True)
    zs, zd = restated(meta, a, sd)
    err = max(tr.rel_err(torch.from_numpy(a['z_src']), zs), tr.rel_err(torch.from_numpy(a['z_dst']), zd))
    noise = NOISE['fixtures'][name]
    print(f'{name}: reference float32 vs float64 restatement {err:.3e} (recorded {noise:.3e})')
    assert err < 1e-5 and abs(err - noise) <= 1e-9 + 1e-3 * noise


def test_the_two_reference_quirks_are_in_the_fixture():
    """Pad tokens are not zeroed after the projection, and pad slots carry the pair features of the last node."""
    meta, a = load('g17_tpnet_enc_padheavy')
    sd = fixture_state_dict(meta, a)
    i = encoder_inputs(a)
    want = torch.from_numpy(a['z_src'])
    assert (i['nbr_nids'][0] == -1).all()  # an all-pad row
    # zeroing the pad tokens after the projection would give another answer ...
    tok = tr.tpnet_tokens(sd, rp_dict(meta['cfg']), **i)
    g = lambda n: sd[n].double()
    F = torch.nn.functional
    z = F.linear(F.relu(F.linear(tok, g('projection_layer.0.weight'), g('projection_layer.0.bias'))), g('projection_layer.2.weight'), g('projection_layer.2.bias'))
    z = z.masked_fill((i['nbr_nids'] == -1).unsqueeze(-1), 0.0)
    for l in range(meta['dims']['num_layers']):
        z = tr.mixer_forward(sd, f'mlp_mixers.{l}.', z)
    assert tr.rel_err(want, z.mean(dim=1)[: want.shape[0]]) > 1e-3
    # ... and so would pair features of another row for the pads
    moved = dict(sd)
    for l in range(meta['cfg']['num_layer'] + 1):
        t = sd[f'random_projections.random_projections.{l}'].clone()
        t[-1] = t[0]
        moved[f'random_projections.random_projections.{l}'] = t
    last = meta['cfg']['num_nodes'] - 1
    assert not (i['nbr_nids'] == last).any() and not (i['src'] == last).any() and not (i['dst'] == last).any()
    zs, _ = tr.tpnet_forward(moved, meta['dims']['num_layers'], rp_dict(meta['cfg']), **i)
    assert tr.rel_err(want, zs) > 1e-4


def test_constructor_dim_rule_and_errors():
    import math

    from tgm_amd.nn import RandomProjectionModule, TPNet

    with pytest.raises(ValueError, match='enforce_dim'):
        RandomProjectionModule(10, 2, 1e-6, 0, use_matrix=False)
    m = RandomProjectionModule(10, 2, 1e-6, 0)
    assert m.dim == 10 and m.out_dim == 36 and torch.equal(m.random_projections[0], torch.eye(10)) and not m.random_projections[1].any()
    m = RandomProjectionModule(9228, 2, 1e-6, 0, use_matrix=False, num_edges=110_000, dim_factor=10, concat_src_dst=False)
    assert m.dim == int(math.log(220_000)) * 10 == 120 and m.out_dim == 9
    assert RandomProjectionModule(50, 1, 1e-6, 0, use_matrix=False, num_edges=110_000, dim_factor=10).dim == 50  # capped by num_nodes
    assert RandomProjectionModule(50, 1, 1e-6, 0, use_matrix=False, enforce_dim=7, num_edges=5, dim_factor=3).dim == 7  # enforce_dim wins
    assert [p.requires_grad for p in m.random_projections] == [False] * 3 and not m.now_time.requires_grad
    assert m.now_time.dtype == m.beginning_time.dtype == torch.int64  # an integer beginning_time stays int64, as the reference's does
    assert RandomProjectionModule(5, 1, 1e-6, 0.5).now_time.dtype == torch.float32
    enc = TPNet(4, 3, 6, 8, 5, random_projections=m)
    assert enc.random_feature_dim == 18 and enc.projection_layer[0].in_features == 4 + 3 + 6 + 18 and enc.projection_layer[2].out_features == 8
    assert len(enc.mlp_mixers) == 2 and enc.mlp_mixers[0].num_tokens == 5 and enc.mlp_mixers[0].token_feedforward.ffn[0].out_features == 2
    assert TPNet(4, 3, 6, 8, 5).projection_layer[0].in_features == 13


def test_backup_reset_reload_on_the_host():
    from tgm_amd.nn import RandomProjectionModule

    m = RandomProjectionModule(6, 2, 1e-6, 3, use_matrix=False, enforce_dim=4)
    with torch.no_grad():
        m.random_projections[1].fill_(2.0)
        m.now_time.data = torch.tensor(9)
    p0 = m.random_projections[0].clone()
    now, tabs = m.backup_random_projections()
    assert int(now) == 9 and len(tabs) == 2 and torch.equal(tabs[0], torch.full((6, 4), 2.0))
    m.reset_random_projections(reset_zero=False)
    assert int(m.now_time) == 3 and not m.random_projections[1].any() and torch.equal(m.random_projections[0], p0)
    m.reset_random_projections()
    assert not torch.equal(m.random_projections[0], p0)  # redrawn
    m.reload_random_projections((now, tabs))
    assert int(m.now_time) == 9 and torch.equal(m.random_projections[1], tabs[0])
    with pytest.raises(ValueError, match='Expected a tuple'):
        m.reload_random_projections((now,))
    with pytest.raises(ValueError, match='now time must be'):
        m.reload_random_projections((9, tabs))
    with pytest.raises(ValueError, match='num_layer'):
        m.reload_random_projections((now, tabs[:1]))
    with pytest.raises(ValueError, match=r'random_projections\[1\] must be'):
        m.reload_random_projections((now, [tabs[0], None]))


def test_cpu_tensors_raise():
    from tgm_amd.exceptions import NativeLibraryError
    from tgm_amd.nn import RandomProjectionModule, TPNet

    rp = RandomProjectionModule(9, 2, 1e-6, 0, use_matrix=False, enforce_dim=4).eval()
    ids = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(NativeLibraryError):
        rp(ids, ids)
    with pytest.raises(NativeLibraryError):
        rp.update(ids, ids, ids)
    m = TPNet(4, 3, 6, 8, 5, random_projections=rp).eval()
    B = 2
    args = lambda k: (torch.zeros(9, 4), torch.zeros(2, B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64), torch.zeros(2 * B, k, dtype=torch.int64),
                      torch.zeros(2 * B, k, dtype=torch.int64), torch.zeros(2 * B, k, 3))  # fmt: skip
    with pytest.raises(NativeLibraryError):
        m(*args(5))
    with pytest.raises(NativeLibraryError):
        m.train()(*args(5))
    with pytest.raises(ValueError, match='num_neighbors'):  # shapes are validated before anything touches the device
        m(*args(4))
