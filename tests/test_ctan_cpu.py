"""CTAN without a GPU: the restatement against the reference's recorded memory states (tests/golden/g22_ctanmem_*.npz), the Python surface
(constructors, state_dict, import paths), the struct mirror and the refusal to compute off the GPU."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import ctan_restate as cr

GOLDEN = cr.GOLDEN
FIXTURES = sorted(os.path.basename(p)[len('g22_ctanmem_'):-4] for p in glob.glob(os.path.join(GOLDEN, 'g22_ctanmem_*.npz')))
EXPECTED = ['basic', 'dup_in_batch', 'f32_tie', 'init_time_reset', 'ooo', 'rows_mismatch', 'wiki_small']


load_fixture, replay = cr.load_fixture, cr.replay


def test_fixture_set_is_complete():
    assert FIXTURES == EXPECTED


@pytest.mark.parametrize('name', EXPECTED)
def test_restatement_reproduces_the_reference_memory(name):
    z, meta = load_fixture(name)
    replay(z, meta, cr.CTANMemoryRestated, lambda m, *a: m.update_state(*a), lambda m: m.reset_state(), lambda m: (m.memory, m.last_update))


def test_f32_tie_is_what_the_issue_says():
    z, meta = load_fixture('f32_tie')
    assert z['src'].tolist() == [1, 2, 1, 4] and z['dst'].tolist() == [2, 3, 5, 1]
    assert z['t'].tolist() == [1000000001, 1000000002, 1000000003, 1000000002]
    assert np.array_equal(z['memory'][0][1], z['src_emb0'][0]) and int(z['last_update'][0][1]) == 1000000003
    m = cr.CTANMemoryRestated(8, 4)
    assert m.winners(z['src'], z['dst'], z['t'])[1] == (0, 1000000003)


def test_import_paths():
    import tgm_amd.nn.encoder.ctan as mod
    from tgm_amd.nn import CTAN as A
    from tgm_amd.nn import CTANMemory as B
    from tgm_amd.nn.encoder import CTAN, CTANMemory

    assert mod.CTAN is CTAN is A and mod.CTANMemory is CTANMemory is B
    import tgm_amd.nn.ctan

    assert mod is tgm_amd.nn.ctan


@pytest.mark.parametrize('dims', [dict(edge_dim=7, memory_dim=5, time_dim=2, node_dim=1), dict(edge_dim=172, memory_dim=32, time_dim=16, node_dim=3)])
def test_state_dict_keys_and_shapes(dims):
    from tgm_amd.nn.encoder import CTAN

    enc = CTAN(**dims, num_iters=3, mean_delta_t=2.0, std_delta_t=3.0, epsilon=0.5, gamma=0.2)
    want = cr.expected_shapes(**dims)
    sd = enc.state_dict()
    assert sorted(sd) == sorted(want)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert sorted(n for n, _ in enc.named_parameters()) == sorted(cr.PARAMS) and [n for n, _ in enc.named_buffers()] == ['aconv.eye']
    assert torch.equal(sd['aconv.eye'], torch.eye(dims['memory_dim'])) and not sd['aconv.bias'].any()
    assert (enc.mean_delta_t, enc.std_delta_t, enc.aconv.num_iters, enc.aconv.epsilon, enc.aconv.gamma) == (2.0, 3.0, 3, 0.5, 0.2)
    # strict loading from a dict with exactly the reference's keys
    g = torch.Generator().manual_seed(0)
    other = {k: torch.randn(s, generator=g) for k, s in want.items()}
    enc.load_state_dict(other, strict=True)
    assert all(torch.equal(enc.state_dict()[k], other[k]) for k in want)
    with pytest.raises(RuntimeError):
        enc.load_state_dict({**other, 'aconv.phi.lin_skip.weight': torch.zeros(1)}, strict=True)


def test_defaults_match_the_reference_signature():
    import inspect

    from tgm_amd.nn.encoder import CTAN, CTANMemory

    sig = inspect.signature(CTAN.__init__)
    assert list(sig.parameters)[1:] == ['edge_dim', 'memory_dim', 'time_dim', 'node_dim', 'num_iters', 'mean_delta_t', 'std_delta_t', 'epsilon', 'gamma']
    assert [sig.parameters[k].default for k in ('num_iters', 'mean_delta_t', 'std_delta_t', 'epsilon', 'gamma')] == [1, 0.0, 1.0, 0.1, 0.1]
    sig = inspect.signature(CTANMemory.__init__)
    assert list(sig.parameters)[1:] == ['num_nodes', 'memory_dim', 'aggr_module', 'init_time'] and sig.parameters['init_time'].default == 0
    assert list(inspect.signature(CTAN.forward).parameters)[1:] == ['node_x', 'last_update', 'edge_index', 't', 'msg']
    assert list(inspect.signature(CTANMemory.update_state).parameters)[1:] == ['src', 'pos_dst', 't', 'src_emb', 'pos_dst_emb']


def test_memory_buffers_and_reset():
    from tgm_amd.nn.encoder import CTANMemory, LastAggregator, MeanAggregator

    mem = CTANMemory(9, 4, aggr_module=LastAggregator(), init_time=77)
    sd = mem.state_dict()
    assert sorted(sd) == ['_assoc', 'last_update', 'memory']
    assert sd['memory'].shape == (9, 4) and sd['memory'].dtype == torch.float32 and not sd['memory'].any()
    assert sd['last_update'].dtype == torch.int64 and sd['last_update'].tolist() == [77] * 9
    assert sd['_assoc'].shape == (9,) and sd['_assoc'].dtype == torch.int64
    mem.memory += 1
    mem.last_update += 5
    mem.reset_parameters()
    assert not mem.memory.any() and mem.last_update.tolist() == [77] * 9
    mem.detach()
    other = CTANMemory(9, 4, aggr_module=MeanAggregator())
    other.load_state_dict(sd, strict=True)
    assert other.last_update.tolist() == [77] * 9

    class Other(torch.nn.Module):
        pass

    with pytest.raises(NotImplementedError, match='Other'):
        CTANMemory(9, 4, aggr_module=Other())


def test_no_cpu_fallback():
    from tgm_amd.exceptions import NativeLibraryError
    from tgm_amd.nn.encoder import CTAN, CTANMemory, LastAggregator

    enc = CTAN(edge_dim=7, memory_dim=5, time_dim=2, node_dim=1).eval()
    ei = torch.randint(0, 10, (2, 10))
    args = (torch.rand(10, 6), torch.zeros(10, dtype=torch.long), ei, torch.arange(10), torch.randint(0, 10, (10, 7)))
    with pytest.raises(NativeLibraryError):
        enc(*args)
    with torch.no_grad(), pytest.raises(NativeLibraryError):
        enc(*args)
    mem = CTANMemory(10, 5, aggr_module=LastAggregator())
    with pytest.raises(NativeLibraryError):
        mem(torch.arange(3))
    with pytest.raises(NativeLibraryError):
        mem.update_state(ei[0], ei[1], torch.arange(10), torch.rand(10, 5), torch.rand(10, 5))


def test_struct_mirror_and_signatures():
    from tgm_amd import _native

    lib = _native.load()
    assert lib.tgmx_abi_sizeof(22) == ctypes.sizeof(_native.CtanFwd) > 0
    assert lib.tgmx_abi_sizeof(23) == 0
    for name in ('tgmx_ctan_forward', 'tgmx_ctan_attend', 'tgmx_ctan_memory_update'):
        assert name in _native.SIGNATURES and hasattr(lib, name)


def test_composed_forward_is_the_restated_arithmetic():
    """The torch-op composition the training path runs (CTAN.forward_composed, device-agnostic) against the restatement, float32 on the CPU."""
    from tgm_amd.nn.encoder import CTAN

    torch.manual_seed(3)
    U, E, D, M, T = 12, 40, 3, 6, 4
    enc = CTAN(edge_dim=D, memory_dim=M, time_dim=T, node_dim=2, num_iters=2, mean_delta_t=3.0, std_delta_t=7.0, epsilon=0.4, gamma=0.3)
    with torch.no_grad():
        enc.aconv.bias.uniform_(-0.5, 0.5)
    node_x, lu = torch.randn(U, M + 2), torch.randint(0, 60, (U,))
    ei, t, msg = torch.randint(0, U - 2, (2, E)), torch.randint(0, 60, (E,)), torch.randint(0, 5, (E, D))
    with torch.no_grad():
        got = enc.forward_composed(node_x, lu, ei, t, msg)
    kw = dict(num_iters=2, mean_delta_t=3.0, std_delta_t=7.0, epsilon=0.4, gamma=0.3)
    ref = cr.ctan_forward(enc.state_dict(), node_x, lu, ei, t, msg, **kw)
    assert got.shape == (U, M) and cr.rel_err(got, ref) < 5e-6
    assert cr.rel_err(cr.ctan_forward(enc.state_dict(), node_x, lu, ei, t, msg, use_abs=False, **kw), ref) > 1e-3
    assert cr.rel_err(cr.ctan_forward(enc.state_dict(), node_x, lu, ei, t, msg, swap_edge_blocks=True, **kw), ref) > 1e-3
