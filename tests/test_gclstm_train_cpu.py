"""GCLSTM training without a GPU: the hand-derived backward (tests/gclstm_bwd_restate.py) against float64 autograd through the restated
forward (tests/gclstm_restate.py) on the g23 fixtures and a random K = 4 cell, its float32 evaluation against the rounding bound with every
wrong variant outside it, the ABI additions, the argument checks of the new entry points, and ``TGMX_GCLSTM_BWD``."""
import ctypes
import functools

import pytest
import torch

import gclstm_bwd_restate as br
import gclstm_restate as gr
from oracle.tgat_bwd_ref import EPS, F64, worst_ratio


def _random_case():
    """K = 4, weighted, directed with self loops and duplicates, no normalisation with lambda_max (the diagonal is a degree)."""
    g = torch.Generator().manual_seed(404)
    N, cin, Co, K, E = 23, 5, 6, 4, 120
    sd = {k: torch.empty(s).uniform_(-0.5, 0.5, generator=g) for k, s in gr.expected_shapes(cin, Co, K).items()}
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[:, 10:20] = ei[:, 20:30]
    snap = dict(x=torch.randn(N, cin, generator=g), edge_index=ei, edge_weight=torch.rand(E, generator=g) + 0.5)
    meta = dict(normalization=None, lambda_max=12.0)
    return meta, sd, [snap], torch.randn(N, Co, generator=g) * 0.5, torch.randn(N, Co, generator=g) * 0.5


@functools.lru_cache(maxsize=None)
def _case(name):
    """(sd, the last snapshot's inputs with the states before it, normalisation, lambda_max) -- once per name."""
    if name == 'random_k4':
        meta, sd, snaps, H, C = _random_case()
    else:
        meta, sd, snaps = gr.load_fixture(name)
        H = C = None
        for snap in snaps[:-1]:
            H, C = gr.gclstm_forward(sd, snap['x'], snap['edge_index'], snap['edge_weight'], H, C, meta['lambda_max'], meta['normalization'])
        H, C = (None if H is None else H.float()), (None if C is None else C.float())
    snap = snaps[-1]
    N, Co = snap['x'].shape[0], sd['W_i'].shape[1]
    g = torch.Generator().manual_seed(len(name))
    H = torch.randn(N, Co, generator=g) * 0.5 if H is None else H  # (a one-snapshot fixture: states that are not zero)
    C = torch.randn(N, Co, generator=g) * 0.5 if C is None else C
    dH, dC = torch.randn(N, Co, generator=g).double(), torch.randn(N, Co, generator=g).double()
    return sd, snap, H, C, meta['normalization'], meta['lambda_max'], dH, dC


CASES = gr.EXPECTED_FIXTURES + ['random_k4']


@pytest.mark.parametrize('name', CASES)
def test_restatement_equals_float64_autograd(name):
    sd, snap, H, C, norm, lm, dH, dC = _case(name)
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    x64, H64, C64 = (t.double().requires_grad_() for t in (snap['x'], H, C))
    Ho, Co_ = gr.gclstm_forward(sd64, x64, snap['edge_index'], snap['edge_weight'], H64, C64, lm, norm)
    ((Ho * dH).sum() + (Co_ * dC).sum()).backward()
    want = {**{k: v.grad for k, v in sd64.items()}, 'node_x': x64.grad, 'H': H64.grad, 'C': C64.grad}
    saved = br.forward_saved(sd, snap['x'], snap['edge_index'], snap['edge_weight'], H, C, lm, norm)
    got = br.cell_backward(sd, saved, dH, dC)
    assert set(got) == set(want)
    for k, (val, mag) in got.items():
        assert val.shape == want[k].shape and gr.rel_err(val, want[k]) <= 1e-12, (name, k)
        assert (mag >= 0).all() and torch.isfinite(mag).all() and (mag >= val.abs() * (1 - 1e-12)).all(), (name, k)
    # one upstream gradient alone
    for only in ('H', 'C'):
        for t in (*sd64.values(), x64, H64, C64):
            t.grad = None
        Ho, Co_ = gr.gclstm_forward(sd64, x64, snap['edge_index'], snap['edge_weight'], H64, C64, lm, norm)
        ((Ho * dH).sum() if only == 'H' else (Co_ * dC).sum()).backward()
        got = br.cell_backward(sd, saved, dH if only == 'H' else None, dC if only == 'C' else None)
        for k, t in (('H', H64), ('C', C64), ('W_f', sd64['W_f']), ('conv_i.lins.0.weight', sd64['conv_i.lins.0.weight'])):
            assert gr.rel_err(got[k][0], t.grad) <= 1e-12, (name, only, k)
        if only == 'C':  # the output gate takes no part in C'
            assert sd64['W_o'].grad is None and not got['W_o'][0].any() and not got['conv_o.lins.0.weight'][0].any()


@pytest.mark.parametrize('name', CASES)
def test_float32_evaluation_stays_inside_the_bound_and_mutants_fall_outside(name):
    sd, snap, H, C, norm, lm, dH, dC = _case(name)
    saved = br.forward_saved(sd, snap['x'], snap['edge_index'], snap['edge_weight'], H, C, lm, norm, rounded=True)
    dH, dC = dH.float().double(), dC.float().double()
    want = br.cell_backward(sd, saved, dH, dC)
    f32 = br.cell_backward(sd, saved, dH, dC, dtype=torch.float32)
    n = br.cell_chain(saved)
    for k, (val, mag) in want.items():
        assert f32[k][0].dtype == torch.float32
        assert worst_ratio(f32[k][0], val, n * EPS * mag) <= 1.0, (name, k)
    K = saved['K']
    for mutation, (_, shows) in br.MUTATIONS.items():
        wrong = br.cell_backward(sd, saved, dH, dC, mutate=mutation)
        worst = max(worst_ratio(wrong[k][0].float(), val, n * EPS * mag) for k, (val, mag) in want.items())
        directed = bool(saved['lap'][0].numel()) and mutation == 'L_for_LT' and _asymmetric(saved['lap'], saved['N'])
        if shows(K=K) and (mutation != 'L_for_LT' or directed):
            assert worst > 1.0, (name, mutation, worst)
        elif mutation != 'L_for_LT':
            assert worst <= 1.0, (name, mutation, worst)  # the variant cannot show here: it IS the formula


def _asymmetric(lap, N):
    row, col, m, _ = lap
    L = torch.zeros(N, N, dtype=F64)
    L.index_put_((col, row), m, accumulate=True)
    return not torch.allclose(L, L.t(), atol=1e-9)


def test_mutations_show_somewhere():
    """Every wrong variant is caught by at least one case (the Clenshaw ones need K >= 3 / a directed graph)."""
    caught = set()
    for name in ('k3_directed', 'k4_loops_dups', 'random_k4'):
        sd, snap, H, C, norm, lm, dH, dC = _case(name)
        saved = br.forward_saved(sd, snap['x'], snap['edge_index'], snap['edge_weight'], H, C, lm, norm, rounded=True)
        want, n = br.cell_backward(sd, saved, dH, dC), br.cell_chain(saved)
        for mutation in br.MUTATIONS:
            wrong = br.cell_backward(sd, saved, dH, dC, mutate=mutation)
            if max(worst_ratio(wrong[k][0].float(), val, n * EPS * mag) for k, (val, mag) in want.items()) > 1.0:
                caught.add(mutation)
    assert caught == set(br.MUTATIONS)


@pytest.mark.parametrize('N,C', br.GATE_CASES)
def test_gate_backward_float32_against_its_bound(N, C):
    for saturate_all in (False, True):
        c = br.gate_case(N, C, saturate_all=saturate_all)
        for dH, dC in ((True, True), (False, True), (True, False)):
            (dpre, dcp), (bp, bc) = br.gate_bounds(c, dH, dC)
            got = br.gate_backward(c['pre'], c['Cprev'], c['dH'] if dH else None, c['dC'] if dC else None, dtype=torch.float32)
            assert worst_ratio(got[0], dpre, bp) <= 1.0 and worst_ratio(got[1], dcp, bc) <= 1.0
            assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    assert br.gate_chain() == 28
    N, C = br.GATE_BIG_CASE
    assert N * C == 16384 * 256 + 96


def test_clenshaw_is_the_transpose_of_the_recurrence():
    """<w, T_k(L) h> summed over k equals <Clenshaw(w), h> for any h: the reverse pass is the adjoint of the basis."""
    g = torch.Generator().manual_seed(3)
    N, C, E = 17, 3, 60
    ei = torch.randint(0, N, (2, E), generator=g)
    lap = gr.scaled_laplacian(ei, torch.rand(E, generator=g) + 0.5, N, 'rw', 2.5)
    for K in (1, 2, 3, 4, 5):
        h, w = torch.randn(N, C, generator=g, dtype=F64), torch.randn(N, K * C, generator=g, dtype=F64)
        lhs = sum((w[:, k * C:(k + 1) * C] * t).sum() for k, t in enumerate(gr.cheb_basis(lap, h, K)))
        dH, mag = br.clenshaw(lap, w, K)
        assert abs(float(lhs - (dH * h).sum())) <= 1e-10 * float(mag.abs().sum()) and (mag >= dH.abs() - 1e-12).all()
    assert br.clenshaw_chain(1, 5, 9) == 9 + 8 and br.clenshaw_chain(4, 5, 9) == 9 + 2 * 13 + 8


def test_abi_additions():
    from tgm_amd import _native

    lib = _native.load()
    for name in ('tgmx_gclstm_gate_backward', 'tgmx_cheb_laplacian_t', 'tgmx_cheb_propagate2', 'tgmx_cheb_clenshaw', 'tgmx_gclstm_backward',
                 'tgmx_gclstm_backward_workspace_bytes'):  # fmt: skip
        assert name in _native.SIGNATURES and hasattr(lib, name)
    assert lib.tgmx_abi_sizeof(32) == ctypes.sizeof(_native.GclstmBwd) > 0 and lib.tgmx_version() == 7
    assert lib.tgmx_abi_sizeof(24) == ctypes.sizeof(_native.GclstmFwd)  # tgmx_gclstm_fwd_t is unchanged


def test_new_entry_points_reject_null_pointers_and_bad_sizes():
    """Every check below fails before anything is launched: no device is needed."""
    from tgm_amd import _native

    lib = _native.load()
    x = 0x1000  # (never dereferenced: the calls return before any launch)
    E_INVALID = lib.tgmx_gclstm_backward(None, None)
    assert E_INVALID != 0 and lib.tgmx_gclstm_backward_workspace_bytes(None) == 0
    assert lib.tgmx_gclstm_gate_backward(None, x, 4, 3, x, 3, x, 3, x, x, None) == E_INVALID
    assert lib.tgmx_gclstm_gate_backward(x, x, 4, 3, x, 2, x, 3, x, x, None) == E_INVALID  # lddh < C
    assert lib.tgmx_gclstm_gate_backward(x, x, 0, 3, x, 3, x, 3, x, x, None) == 0  # N = 0: nothing to do
    assert lib.tgmx_cheb_propagate2(x, x, x, x, 4, 3, x, 3, x, 3, None, 0, 1.0, 1.0, -1.0, x + 64, 3, 5, None, 0, None) == E_INVALID  # gamma without prev2
    assert lib.tgmx_cheb_propagate2(x, x, x, x, 4, 3, x, 3, x, 3, None, 0, 1.0, 1.0, 0.0, x, 3, 5, None, 0, None) == E_INVALID  # t is out
    assert lib.tgmx_cheb_clenshaw(x, x, x, x, 4, 3, 1, x, 3, x, 3, 5, None, 0, None) == E_INVALID  # K = 1 reads no graph
    assert lib.tgmx_cheb_clenshaw(x, x, x, x, 4, 3, 3, x, 8, x, 3, 5, None, 0, None) == E_INVALID  # ldg < K C
    assert lib.tgmx_cheb_laplacian_t(x, x, 0, None, 5, 0, 1, 2.0, None, x, x, x, x, x, 1 << 20, None, None) == E_INVALID  # N = 0
    assert b'cheb_laplacian_t' in lib.tgmx_last_error()
    t = _native.GclstmBwd()
    assert lib.tgmx_gclstm_backward(ctypes.byref(t), None) == E_INVALID and b'bad sizes' in lib.tgmx_last_error()
    t.N, t.in_ch, t.C, t.K, t.ldop, t.E = 10, 4, 3, 2, 8, 7
    assert lib.tgmx_gclstm_backward(ctypes.byref(t), None) == E_INVALID and b'narrower' in lib.tgmx_last_error()
    t.ldop = 12
    small = lib.tgmx_gclstm_backward_workspace_bytes(ctypes.byref(t))
    assert small > 0
    assert lib.tgmx_gclstm_backward(ctypes.byref(t), None) == E_INVALID and b'saved' in lib.tgmx_last_error()
    t.op = t.pre = t.Cprev = x
    t.d_H = x
    assert lib.tgmx_gclstm_backward(ctypes.byref(t), None) == E_INVALID and b'transposed' in lib.tgmx_last_error()
    t.WT, t.ldwt = x, 12
    assert lib.tgmx_gclstm_backward(ctypes.byref(t), None) == E_INVALID and b'edge list' in lib.tgmx_last_error()
    t.src = t.dst = x
    assert lib.tgmx_gclstm_backward_workspace_bytes(ctypes.byref(t)) > small  # the Clenshaw pass brings the transpose and its basis
    assert lib.tgmx_gclstm_backward(ctypes.byref(t), None) == E_INVALID and b'workspace too small' in lib.tgmx_last_error()


def test_mode_parsing_and_the_host_path(monkeypatch):
    from tgm_amd.nn import GCLSTM, _gclstm_train

    monkeypatch.delenv('TGMX_GCLSTM_BWD', raising=False)
    assert _gclstm_train.mode() == 'native'
    for value, want in (('py', 'py'), ('torch', 'torch'), ('', 'native'), ('native', 'native'), ('PY', 'native'), ('1', 'native')):
        monkeypatch.setenv('TGMX_GCLSTM_BWD', value)
        assert _gclstm_train.mode() == want == br.parse_mode(value)
    monkeypatch.delenv('TGMX_GCLSTM_BWD')
    # the composed path is still what host tensors get: the hand-derived gradients agree with it
    sd, snap, H, C, norm, lm, dH, dC = _case('k2_weighted')
    meta, _, _ = gr.load_fixture('k2_weighted')
    cell = GCLSTM(meta['in_channels'], meta['out_channels'], meta['K'], normalization=norm, bias=meta['bias'])
    cell.load_state_dict(sd, strict=True)
    Hh, Ch = H.clone().requires_grad_(), C.clone().requires_grad_()
    Ho, Co_ = cell.forward_composed(snap['x'], snap['edge_index'], snap['edge_weight'], Hh, Ch, lm)
    assert 'Gclstm' not in type(Ho.grad_fn).__name__
    ((Ho * dH.float()).sum() + (Co_ * dC.float()).sum()).backward()
    saved = br.forward_saved(sd, snap['x'], snap['edge_index'], snap['edge_weight'], H, C, lm, norm)
    want = br.cell_backward(sd, saved, dH, dC)
    for k, p in cell.named_parameters():
        gr.close(p.grad, want[k][0].float(), f'composed {k}')
    gr.close(Hh.grad, want['H'][0].float(), 'composed H')
    gr.close(Ch.grad, want['C'][0].float(), 'composed C')
