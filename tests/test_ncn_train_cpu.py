"""NCNPredictor training without a device: the hand-written float64 gradients (tests/ncn_bwd_restate.py) against float64 autograd of the
forward's restatement and against the gradients recorded from the reference, the wrong variants the bound must tell apart, the share of
ambiguous ReLU entries in every case the GPU tests use, the ABI mirror and the workspace arithmetic."""
import ctypes

import pytest
import torch

import ncn_bwd_restate as br
import ncn_restate as nr
import ncn_train_cases as tc

FIXTURES = br.grad_fixture_names()


def test_fixture_set_is_complete():
    assert FIXTURES == br.EXPECTED_GRAD_FIXTURES


def _fixture(name):
    meta, sd, inp, dout, ref = br.load_grad_fixture(name)
    args = (sd, inp['x'], inp['edge_index'], inp['tar_ei'], meta['k'], dout, inp['last_update'], inp['edge_time'])
    return meta, args, ref


@pytest.mark.parametrize('name', br.EXPECTED_GRAD_FIXTURES)
def test_restatement_against_autograd_and_the_recorded_gradients(name):
    meta, args, ref = _fixture(name)
    got = br.grads(*args)
    auto = br.autograd_grads(*args)
    assert set(ref) == {'x', *br.PARAMS}
    for n in ref:
        assert nr.rel_err(got[n][0], auto[n]) < 1e-12, n
        assert nr.rel_err(ref[n], got[n][0]) < 1e-5, n  # the generator's own gate
        assert bool((got[n][1] >= 0).all()) and float(got[n][1].max()) < 1e-3 * max(1.0, float(got[n][0].abs().max())), n


@pytest.mark.parametrize('seed', range(6))
@pytest.mark.parametrize('dup', ['all', 'last'])
def test_restatement_against_autograd_on_random_cases(seed, dup):
    c = tc.random_case(seed, k=2 + 2 * (seed % 2), decay=seed % 3 != 0, out_of_range=seed >= 4)
    got = br.grads(c.sd, c.x, c.ei, c.tar, c.k, c.dout, c.lu, c.et, dup)
    auto = br.autograd_grads(c.sd, c.x, c.ei, c.tar, c.k, c.dout, c.lu, c.et, dup)
    for n in ('x', *br.PARAMS):
        assert nr.rel_err(got[n][0], auto[n]) < 1e-12, n


@pytest.mark.parametrize('variant', br.VARIANTS)
def test_every_wrong_variant_leaves_the_bound_on_some_fixture(variant):
    worst = 0.0
    for name in FIXTURES:
        meta, args, _ = _fixture(name)
        right, wrong = br.grads(*args), br.grads(*args, variant=variant)
        worst = max(worst, br.worst_ratio(wrong['x'][0], right['x'][0], right['x'][1]))
    assert worst > 100.0, (variant, worst)  # not a near miss: the wrong gradient is far outside what float32 rounding allows


@pytest.mark.parametrize('name', sorted(tc.GPU_CASES))
def test_ambiguous_relu_entries_are_rare_in_every_gpu_case(name):
    """A loosened bound must not hide a failure: at most 1 % of h may have a mask the device could read differently."""
    c = tc.GPU_CASES[name]()
    g = br.grads(c.sd, c.x, c.ei, c.tar, c.k, c.dout, c.lu, c.et, c.dup)
    assert br.ambiguous_relu_fraction(g) <= 0.01, name


def test_dx_cases_cross_the_kernel_s_thresholds():
    deg = lambda c: int(nr.dense_adjacency(c.N, c.ei).sum(1).max())
    assert deg(tc.DX_CASES['past_threshold_c257_k2']()) == br.LONG_ROW + 1  # one entry past the split threshold
    assert deg(tc.DX_CASES['hub_c64_k2_decay']()) > br.LONG_ROW + br.CHUNK // 2  # a hub over three chunks or more
    assert nr.dense_adjacency(*tc.rows_graph()[:2]).sum(1)[:5].tolist() == [0, 1, 63, 64, 65]
    assert {c for n in tc.DX_CASES for c in (1, 7, 64, 257) if f'_c{c}_' in n} == {1, 7, 64, 257}


def test_abi_mirror_and_version():
    from tgm_amd import _native

    lib = _native.load()
    assert lib.tgmx_abi_sizeof(33) == ctypes.sizeof(_native.NcnBwd) > ctypes.sizeof(_native.NCNFwd) > 0
    assert lib.tgmx_abi_sizeof(19) == ctypes.sizeof(_native.NCNFwd) and lib.tgmx_version() == 7 and lib.tgmx_abi_sizeof(34) == 0


def _block(N, E, B, C=100, k=4, H=100, out=1):
    from tgm_amd import _native

    t = _native.NcnBwd()
    a = t.fwd
    a.N, a.E, a.B, a.C, a.k, a.H, a.out_ch, a.ldxs, a.ldh, a.tar_stride = N, E, B, C, k, H, out, k * C, H, max(B, 1)
    t.d_x = t.d_w1 = t.d_b1 = t.d_w2 = t.d_b2 = 256  # (only compared against NULL)
    return t


def test_workspace_bytes_is_host_arithmetic_monotone_in_b_and_e():
    from tgm_amd import _native

    lib = _native.load()
    need = lambda *a, **kw: int(lib.tgmx_ncn_backward_workspace_bytes(ctypes.byref(_block(*a, **kw))))
    # (without a device rocPRIM answers the size query of its radix sort only for a single block's worth of keys: B stays small here, and
    # tests/test_ncn_train_gpu.py asks again at large B)
    sizes_b = [need(1250, 2300, B) for B in (0, 1, 9, 200, 201, 400)]
    sizes_e = [need(1250, E, 200) for E in (0, 1, 256, 257, 2300, 10**6)]
    assert all(s > 0 for s in sizes_b + sizes_e)
    assert sizes_b == sorted(sizes_b) and sizes_b[0] < sizes_b[-1]
    assert sizes_e == sorted(sizes_e) and sizes_e[0] < sizes_e[-1]
    assert need(1250, 2**30, 200) == 0 and need(1250, 2**30 - 1, 200) > 0  # 2 E >= 2^31
    assert need(2**30, 10, 200) == 0 and need(10, 10, 2**30) == 0 and need(10, 10, -1) == 0 and need(10, 10, 5, k=8) == 0 and need(10, 10, 5, C=0) == 0
    assert int(lib.tgmx_ncn_dx_workspace_bytes(1250, 2**30, 200, 100)) == 0 < int(lib.tgmx_ncn_dx_workspace_bytes(1250, 2300, 200, 100))
    # a gradient that is not asked for is not paid for
    t = _block(1250, 2300, 200)
    t.d_x = None
    assert 0 < int(lib.tgmx_ncn_backward_workspace_bytes(ctypes.byref(t))) < need(1250, 2300, 200)


def test_the_training_module_is_importable_without_a_device():
    from tgm_amd.nn import _ncn_train

    assert _ncn_train.mode() in ('native', 'py', 'torch') and _ncn_train._tail_route(1, 100) and not _ncn_train._tail_route(17, 100)
