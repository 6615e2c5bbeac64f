"""NCNPredictor at k = 8 without a device: the float64 restatement (tests/ncn8_restate.py) against every fixture recorded from the reference,
the steps that only k = 8 has (column masks, clamp, u) shown to matter, 'all' against 'last', and the workspace arithmetic of the native stage."""
import glob
import json
import os

import pytest
import torch

from golden_util import GOLDEN_DIR, load
import ncn8_restate as n8
import ncn_restate as nr
from test_ncn_cpu import CN_BAR, LOGIT_BAR, build_model, fixture_inputs

CASES8 = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, 'g34_ncn8_*.npz')))
with open(os.path.join(GOLDEN_DIR, 'g34_ncn8_self_noise.json')) as f:
    NOISE8 = json.load(f)['fixtures']


def recorded_rows(meta, cn):
    """The example's fixture stores cn_emb for 16 of its 200 pairs."""
    return cn[meta['cn_rows']] if 'cn_rows' in meta else cn


def test_fixture_set_is_complete():
    assert len(CASES8) == 12 + 1 + 4 + 1 + 1 + 1 and set(CASES8) == set(NOISE8)
    biggest = max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN_DIR, 'g18_ncn_*.npz')))
    assert all(os.path.getsize(os.path.join(GOLDEN_DIR, c + '.npz')) <= biggest for c in CASES8)


@pytest.mark.parametrize('name', CASES8)
def test_restatement_reproduces_the_reference_fixture(name):
    meta, a = load(name)
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    sd = nr.fixture_state_dict(meta, a)
    cn = n8.cn_emb(x, ei, tar, lu, et)
    out = n8.forward(sd, x, ei, tar, lu, et)
    assert meta['k'] == 8 and cn.shape == (tar.shape[1], 7 * meta['C']) and out.shape == (tar.shape[1] * meta['out'],)
    e_cn, e_out = nr.rel_err(torch.from_numpy(a['cn_emb']), recorded_rows(meta, cn)), nr.rel_err(torch.from_numpy(a['logits']), out)
    assert e_cn < CN_BAR and e_out < LOGIT_BAR
    assert abs(e_cn - NOISE8[name]['cn_emb']) < 1e-12 and abs(e_out - NOISE8[name]['logits']) < 1e-12  # the recorded self-noise is this distance
    assert NOISE8[name]['largest_integer'] < 2**24  # the reference's float32 counts are exact
    if meta['decay']:
        assert torch.isfinite(nr.decay_weights(lu, et)).all()


@pytest.mark.parametrize('name', ['g34_ncn8_triangle_plain', 'g34_ncn8_triangle_decay'])
@pytest.mark.parametrize('step', ['masks', 'clamp', 'u'])
def test_masks_clamp_and_u_matter_in_triangle(name, step):
    meta, a = load(name)
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    ref = torch.from_numpy(a['cn_emb'])
    assert nr.rel_err(n8.cn_emb(x, ei, tar, lu, et), ref) < CN_BAR
    assert nr.rel_err(n8.cn_emb(x, ei, tar, lu, et, drop=step), ref) > 1e-3


def test_triangle_has_what_it_is_named_after():
    meta, a = load('g34_ncn8_triangle_plain')
    _, ei, tar, _, _ = fixture_inputs(meta, a)
    co = n8.coefficients(meta['N'], ei, tar)
    ar = torch.arange(tar.shape[1])
    assert (co['u'] != 0).any() and ((co['k3i'] != 0) & (co['u'] != 0)).any() and (co['c22_raw'] < 0).any()
    assert sum(int((c[ar, t] != 0).sum()) for c in (co['c12_raw'], co['c21_raw'], co['c22_raw']) for t in (tar[0], tar[1])) > 0


def test_all_differs_from_last_on_onevsmany():
    meta, a = load('g34_ncn8_onevsmany_plain')
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    ref = torch.from_numpy(a['cn_emb'])
    assert not ref[:-1].any() and ref[-1].any()  # one source repeated: only the last candidate keeps its rows
    assert nr.rel_err(ref, n8.cn_emb(x, ei, tar, duplicate_targets='all')) > 1e-2


def test_hub_and_wide_fixtures_have_their_shapes():
    from tgm_amd import _native

    meta, a = load('g34_ncn8_hub')
    co = n8.coefficients(meta['N'], a['edge_index'], a['tar_ei'])
    assert (co['A'][0] > 0).sum() > 64 and ((co['A'][0] @ co['A']) > 0).sum() > meta['N'] // 2  # a row longer than a wave, a two-hop row over most ids
    cap = _native.load().tgmx_ncn8_lds_max_nodes()
    wide = [c for c in CASES8 if 'wide_n' in c]
    assert wide == [f'g34_ncn8_wide_n{cap + 1}'] and load(wide[0])[0]['N'] == cap + 1  # one past the LDS cap: the workspace storage


def test_workspace_bytes_is_host_arithmetic():
    from tgm_amd import _native

    lib = _native.load()
    cap = lib.tgmx_ncn8_lds_max_nodes()
    assert 5 * 4 * cap + 8272 <= 160 * 1024  # five int32 rows beside the 8 272 bytes of static chunk list, in one CU's LDS
    f = lib.tgmx_ncn8_workspace_bytes
    sizes = [f(n, 200) for n in (1, 12, cap, cap + 1, cap + 2, 10**5, 10**6, 2**31 - 1)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[2] < sizes[3] <= sizes[4] < sizes[5]  # monotone in N (a region is a multiple of 64 int32)
    assert f(cap + 1, 200) >= 200 * 5 * 4 * (cap + 1) and f(cap + 1, 5) >= 5 * 5 * 4 * (cap + 1)
    assert f(cap + 1, 10**6) == f(cap + 1, 256)  # one region per resident workgroup, not per pair
    assert f(cap + 1, 0) > 0
    for n, b in ((0, 5), (-1, 5), (2**31, 5), (12, -1), (12, 2**31)):
        assert f(n, b) == 0


@pytest.mark.parametrize('name', ['g34_ncn8_triangle_decay', 'g34_ncn8_selfloop_plain', 'g34_ncn8_onevsmany_decay', 'g34_ncn8_decay_edges'])
@pytest.mark.parametrize('dup', ['last', 'all'])
def test_composed_path_arithmetic(name, dup):
    """``_torch_xs`` launches nothing: handed the checked inputs directly it runs on host tensors, [B, N] rows and index_add_ over the half-edges."""
    meta, a = load(name)
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    m = build_model(meta, duplicate_targets=dup)
    xs = m._torch_xs(dict(x=x, N=meta['N'], B=tar.shape[1], tar=tar, lu=lu, et=et, adj=None, ei=ei))
    ref = torch.cat([x[tar[0]].double() * x[tar[1]].double(), n8.cn_emb(x, ei, tar, lu, et, duplicate_targets=dup)], dim=-1)
    assert xs.shape == (tar.shape[1], 8 * meta['C']) and xs[:, meta['C'] :].any() and nr.rel_err(xs, ref) < CN_BAR


def test_forward_refuses_what_it_cannot_run():
    """Checked before anything is launched: another k, and a hidden layer wider than the float64 MLP keeps in LDS (no quiet other path)."""
    import ctypes

    from tgm_amd import _native

    lib = _native.load()
    blk = _native.NCNFwd()
    blk.C, blk.k, blk.H, blk.out_ch, blk.ldxs, blk.ldh = 4, 8, 8193, 1, 32, 8196
    assert lib.tgmx_ncn8_forward(ctypes.byref(blk), None, 0, None) != 0 and b'8192' in lib.tgmx_last_error()
    blk.k, blk.H, blk.ldh = 4, 8, 8
    assert lib.tgmx_ncn8_forward(ctypes.byref(blk), None, 0, None) != 0 and b'k must be 8' in lib.tgmx_last_error()


def test_k8_stays_out_of_the_native_backward():
    from tgm_amd.nn import NCNPredictor, _ncn_train

    m8, m4 = NCNPredictor(4, 8, 1, k=8), NCNPredictor(4, 8, 1, k=4)
    x = torch.zeros(3, 4)
    assert not _ncn_train.in_envelope(m8, x) and _ncn_train.in_envelope(m4, x)
    with pytest.raises(NotImplementedError, match='k = 8 runs on device tensors only'):
        m8.get_cn_emb(x, torch.zeros((2, 3), dtype=torch.long), torch.zeros((2, 2), dtype=torch.long), (None, None))
