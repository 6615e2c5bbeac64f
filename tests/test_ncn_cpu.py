"""NCNPredictor without a device: the constructor's contract (state_dict layout, errors), the float64 restatement against every fixture
recorded from the reference, the ABI mirror, and the refusal of CPU tensors."""
import ctypes
import glob
import json
import os

import pytest
import torch

from golden_util import GOLDEN_DIR, load
import ncn_restate as nr

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, 'g18_ncn_*.npz')))
SMALL_CASES = [c for c in CASES if c.endswith(('_plain', '_decay'))]
with open(os.path.join(GOLDEN_DIR, 'g18_ncn_self_noise.json')) as f:
    NOISE = json.load(f)['fixtures']
CN_BAR = 1e-5  # the project's bar for aggregated values
LOGIT_BAR = 1e-4  # the ceiling tests/test_dygformer_gpu.py and tests/test_tpnet_gpu.py use


def build_model(meta, **kw):
    from tgm_amd.nn import NCNPredictor

    return NCNPredictor(meta['C'], meta['H'], meta['out'], k=meta['k'], cn_time_decay=meta['decay'], **kw)


def fixture_inputs(meta, a):
    lu, et = nr.fixture_times(meta, a)
    return nr.fixture_x(meta, a), torch.from_numpy(a['edge_index']), torch.from_numpy(a['tar_ei']), lu, et


def test_fixture_set_is_complete():
    assert len(CASES) == 20 + 2 + 5 + 1 + 2 and set(CASES) == set(NOISE)


@pytest.mark.parametrize('name', ['g18_ncn_rand_k2_plain', 'g18_ncn_rand_k4_decay', 'g18_ncn_width_c100_h100_o3'])
def test_state_dict_layout_is_the_reference_s(name):
    meta, a = load(name)
    sd = build_model(meta).state_dict()
    assert list(sd) == meta['state_dict_keys'] == ['xslin.weight', 'xslin.bias', 'xsmlp.0.weight', 'xsmlp.0.bias', 'xsmlp.2.weight', 'xsmlp.2.bias']
    assert {k: list(v.shape) for k, v in sd.items()} == meta['shapes']
    assert {k: str(v.dtype)[6:] for k, v in sd.items()} == meta['dtypes']
    m = build_model(meta)
    m.load_state_dict(nr.fixture_state_dict(meta, a), strict=True)


def test_initialisation_order_is_the_reference_s():
    """Same seed, same draws: xslin first, then xsmlp.0, then xsmlp.2 (the fixture stores the reference's freshly initialised weights)."""
    meta, a = load('g18_ncn_rand_k2_plain')
    torch.manual_seed(1801)
    sd = build_model(meta).state_dict()
    ref = nr.fixture_state_dict(meta, a)
    assert all(torch.equal(sd[k], ref[k]) for k in ref)


def test_constructor_errors_and_the_extra_argument():
    from tgm_amd.nn import NCNPredictor
    from tgm_amd.nn.decoder.ncnpred import NCNPredictor as by_reference_path

    assert by_reference_path is NCNPredictor
    with pytest.raises(ValueError, match=r'Please choose k from \[2,4,8\]'):
        NCNPredictor(4, 8, 1, k=3)
    with pytest.raises(ValueError, match='duplicate_targets'):
        NCNPredictor(4, 8, 1, duplicate_targets='first')
    with pytest.raises(TypeError):
        NCNPredictor(4, 8, 1, 2, False, 'all')  # keyword-only
    a, b = NCNPredictor(4, 8, 1, duplicate_targets='all'), NCNPredictor(4, 8, 1)
    assert list(a.state_dict()) == list(b.state_dict()) and not any('duplicate' in k for k in a.state_dict())
    b.load_state_dict(a.state_dict(), strict=True)
    assert b.duplicate_targets == 'last' and a.duplicate_targets == 'all'
    assert NCNPredictor(4, 8, 1, k=8).xsmlp[0].in_features == 32  # accepted; forward is not implemented


def test_missing_time_information_raises_the_reference_s_error():
    from tgm_amd.nn import NCNPredictor

    m = NCNPredictor(4, 8, 1, cn_time_decay=True)
    x, ei, tar = torch.randn(5, 4), torch.zeros((2, 3), dtype=torch.long), torch.zeros((2, 2), dtype=torch.long)
    with pytest.raises(RuntimeError, match='Please provide time_information to perform time decay'):
        m(x, ei, tar)
    with pytest.raises(RuntimeError, match='Please provide time_information to perform time decay'):
        m(x, ei, tar, last_update=torch.zeros(5, dtype=torch.long))
    with pytest.raises(RuntimeError, match='Please provide time_information to perform time decay'):
        m.get_cn_emb(x, ei, tar, (None, None))


def test_k8_forward_is_not_implemented():
    from tgm_amd.nn import NCNPredictor

    with pytest.raises(NotImplementedError, match='k = 8'):
        NCNPredictor(4, 8, 1, k=8)(torch.randn(5, 4), torch.zeros((2, 3), dtype=torch.long), torch.zeros((2, 2), dtype=torch.long))


def test_cpu_tensors_are_refused():
    from tgm_amd.exceptions import NativeLibraryError
    from tgm_amd.nn import NCNPredictor
    from tgm_amd.nn.ncn import adjacency

    m = NCNPredictor(4, 8, 1).eval()
    x, ei, tar = torch.randn(5, 4), torch.zeros((2, 3), dtype=torch.long), torch.zeros((2, 2), dtype=torch.long)
    with pytest.raises(NativeLibraryError):
        m(x, ei, tar)
    with torch.no_grad(), pytest.raises(NativeLibraryError):
        m(x, ei, tar)
    with pytest.raises(NativeLibraryError):
        adjacency(5, ei)


def test_abi_mirror_size():
    from tgm_amd import _native

    assert _native.load().tgmx_abi_sizeof(19) == ctypes.sizeof(_native.NCNFwd)


@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_the_reference_fixture(name):
    meta, a = load(name)
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    sd = nr.fixture_state_dict(meta, a)
    cn = nr.cn_emb(x, ei, tar, meta['k'], lu, et)
    out = nr.forward(sd, x, ei, tar, meta['k'], lu, et)
    e_cn, e_out = nr.rel_err(torch.from_numpy(a['cn_emb']), cn), nr.rel_err(torch.from_numpy(a['logits']), out)
    assert cn.shape == (tar.shape[1], (meta['k'] - 1) * meta['C']) and out.shape == (tar.shape[1] * meta['out'],)
    assert e_cn < CN_BAR and e_out < LOGIT_BAR
    assert abs(e_cn - NOISE[name]['cn_emb']) < 1e-12 and abs(e_out - NOISE[name]['logits']) < 1e-12  # the recorded self-noise is this distance


def test_the_duplicate_target_rule_and_the_discarded_relu_matter_in_the_fixtures():
    meta, a = load('g18_ncn_onevsmany_k4_plain')
    x, ei, tar, lu, et = fixture_inputs(meta, a)
    ref = torch.from_numpy(a['cn_emb'])
    assert not ref[:-1].any() and ref[-1].any()  # one source repeated: only the last candidate keeps its rows
    assert nr.rel_err(ref, nr.cn_emb(x, ei, tar, 4, duplicate_targets='all')) > 1e-2
    sd = nr.fixture_state_dict(meta, a)
    assert (x[tar[0]] * x[tar[1]] < 0).any()
    assert nr.rel_err(torch.from_numpy(a['logits']), nr.forward(sd, x, ei, tar, 4, relu_xs=True)) > 1e-3
