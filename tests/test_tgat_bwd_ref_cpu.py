"""Keeps ``oracle/tgat_bwd_ref.py`` honest without a GPU: the float64 restatements that ``tests/test_tgat_bwd_blocks_gpu.py`` holds the
kernels of ``csrc/tgat_bwd.hip`` against

* equal torch float64 autograd through a plain forward (1e-10 relative),
* come with bars that an honest float32 evaluation of the same formulas meets with a factor two to spare, on every shape of the
  GPU file, and
* lose to every listed mutation (a dropped slot, the other head's weights, a forgotten mask, a neighbouring slot's time, a skipped
  column, a missing accumulation, a dropped or doubled row): each breaks the bar on at least one element, at every shape.
"""
import pytest
import torch

from oracle import tgat_bwd_ref as ref

F64 = torch.float64


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp(min=1e-300))


def _keep(case, H, k, drop):
    """The dropout keep mask times 1 / (1 - p) (p = 0.25: a visible share of dropped elements in k + 8 rows), or ones."""
    if not drop:
        return torch.ones(case['R'], H, k)
    g = torch.Generator().manual_seed(5)
    return (torch.rand(case['R'], H, k, generator=g) >= 0.25).float() / 0.75


# ---------------------------------------------------------------------------------------------------------------------------
# the restatements equal autograd
# ---------------------------------------------------------------------------------------------------------------------------
def test_sgemm_tn_colsum_equal_autograd():
    g = torch.Generator().manual_seed(0)
    A, B = torch.randn(2, 37, 5, generator=g), torch.randn(2, 37, 9, generator=g)
    W = torch.zeros(2, 5, 9, dtype=F64, requires_grad=True)  # Y = A W: dW = A^T dY
    ((A.double() @ W) * B.double()).sum().backward()
    assert _rel(ref.sgemm_tn(A, B)[0], W.grad) <= 1e-10
    b = torch.zeros(9, dtype=F64, requires_grad=True)
    ((b + torch.zeros(37, 9, dtype=F64)) * B[0].double()).sum().backward()
    assert _rel(ref.colsum(B[0])[0], b.grad) <= 1e-10


def test_relu_mask_add_cols_equal_autograd():
    h = torch.tensor([[0.0, -0.0, 1e-45, -1e-45, 2.0, -3.0]])
    gr = torch.arange(1.0, 7.0)[None]
    x = h.double().clone().requires_grad_(True)
    (torch.relu(x) * gr.double()).sum().backward()
    want = x.grad.clone()
    want[0, 0] = 0.0  # torch's relu has subgradient 0 at 0 too; spelled out: the kernel's test is h > 0
    assert torch.equal(ref.relu_mask(gr, h)[0], want)
    assert torch.equal(ref.add_cols(gr, h, 1)[0], gr.double() + h.double()) and torch.equal(ref.add_cols(gr, h, 0)[0], h.double())


@pytest.mark.parametrize('R,O', [(5, 1), (5, 2), (37, 65), (3, 300)])
def test_ln_backward_equals_autograd(R, O):
    dout, y, res, gamma = ref.ln_case(R, O)
    eps = 1e-5
    u = (y.double() + res.double()).requires_grad_(True)
    gm = gamma.double().clone().requires_grad_(True)
    (torch.nn.functional.layer_norm(u, (O,), gm, torch.zeros(O, dtype=F64), eps) * dout.double()).sum().backward()
    du, dgx, _, _ = ref.ln_backward(dout, y, res, gamma, eps)
    if O == 1:
        assert torch.equal(du, torch.zeros_like(du))
    else:
        assert _rel(du, u.grad) <= 1e-10
    assert float((dgx.sum(0) - gm.grad).abs().max()) <= 1e-10 * float(gm.grad.abs().max().clamp(min=1.0))


@pytest.mark.parametrize('drop', [False, True], ids=['keep1', 'keep_random'])
@pytest.mark.parametrize('shape', [(2, 5, 3, 4, 6), (1, 4, 2, 0, 5), (4, 7, 5, 3, 9)], ids=str)
def test_attn_backward_equals_autograd(shape, drop):
    """Row kinds of attn_case: fully valid, left-padded, an interior hole, all-pad with identical and with differing slot features.
    The restatement differentiates cos at the argument ROUNDED to float32, like the kernels; autograd cannot see a rounding.  So the
    arguments here are ones float32 holds exactly (integer dt < 2^13, tw a power of two, tb a multiple of 1/8): the rounding is the
    identity and d tw, d tb must agree as well."""
    H, k, d, D, T = shape
    c = ref.attn_case(H, k, d, D, T)
    seed_t, nbr_t = c['seed_t'] % 4096 + 4096, c['nbr_t'] % 4096
    nbr_t[k + 3] = nbr_t[k + 3, 0]  # the identical all-pad row stays identical
    tw = torch.tensor([2.0 ** -i for i in range(T)])
    tb = torch.arange(T).float() / 8 - 0.5
    keep = _keep(c, H, k, drop)
    A, grads = ref.attn_forward_autograd(c['qf'], c['dzbar'], c['nbrf'], c['ex'], seed_t, nbr_t, tw, tb, c['scale'], keep, c['mask'])
    nv = c['no_valid']
    assert bool(nv[k + 3]) and bool(nv[k + 4]) and int(nv.sum()) == 2
    assert float((A[nv] - 1.0 / k).abs().max()) <= 1e-15 and float(A[~nv].masked_select(~c['mask'][~nv][:, None, :].expand_as(A[~nv])).max()) == 0.0
    out = ref.attn_backward(c['qf'], A, c['dzbar'], c['nbrf'], c['ex'], seed_t, nbr_t, tw, tb, c['scale'], keep, nv)
    for name, got, want in (('dqf', out['dqf'], grads['dqf']), ('dnbr', out['dnbr'], grads['dnbr']), ('dtw', out['dtime'][:, :T].sum(0), grads['dtw']),
                            ('dtb', out['dtime'][:, T:].sum(0), grads['dtb'])):
        assert _rel(got, want) <= 1e-10, name
    assert torch.equal(out['dqf'][nv], torch.zeros_like(out['dqf'][nv]))  # all-pad rows: nothing flows through the scores


# ---------------------------------------------------------------------------------------------------------------------------
# the bars leave room for float32: the same formulas in float32 stay within half of each
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ref.SGEMM_TN_CASES, ids=str)
def test_sgemm_tn_float32_within_half_the_bar(case):
    R, M, N, batch = case
    g = torch.Generator().manual_seed(R + M)
    A, B = torch.randn(batch, R, M, generator=g), torch.randn(batch, R, N, generator=g)
    err = float((ref.sgemm_tn(A, B, torch.float32)[0].double() - ref.sgemm_tn(A, B)[0]).abs().max()) if R else 0.0
    assert err <= 0.5 * ref.gemm_bar(R), f'{err:.3e} vs {ref.gemm_bar(R):.3e}'


@pytest.mark.parametrize('case', ref.COLSUM_CASES, ids=str)
def test_colsum_float32_within_half_the_bar(case):
    R, C = case
    x = torch.randn(R, C, generator=torch.Generator().manual_seed(R + C))
    err = float((ref.colsum(x, torch.float32)[0].double() - ref.colsum(x)[0]).abs().max())
    assert err <= 0.5 * ref.gemm_bar(R), f'{err:.3e} vs {ref.gemm_bar(R):.3e}'


@pytest.mark.parametrize('O', ref.LN_WIDTHS)
def test_ln_backward_float32_within_half_the_bound(O):
    for R in ref.LN_ROWS:
        dout, y, res, gamma = ref.ln_case(R, O)
        du, dgx, du_mag, dgx_mag = ref.ln_backward(dout, y, res, gamma, 1e-5)
        du32, dgx32, _, _ = ref.ln_backward(dout, y, res, gamma, 1e-5, torch.float32)
        n = ref.ln_chain(O)
        w = max(ref.worst_ratio(du32, du, n * ref.EPS * du_mag), ref.worst_ratio(dgx32, dgx, n * ref.EPS * dgx_mag))
        assert w <= 0.5, f'O={O} R={R}: float32 at {w:.3f} of the bound'


def _attn_ratios(got, want, H, k, C):
    return {name: ref.worst_ratio(got[name], want[name], ref.attn_chain(C, H, k, name == 'dtime') * ref.EPS * want[name + '_mag'])
            for name in ('dqf', 'dnbr', 'dtime')}


@pytest.mark.parametrize('drop', [False, True], ids=['keep1', 'keep_random'])
@pytest.mark.parametrize('shape', ref.ATTN_SHAPES, ids=str)
def test_attn_backward_float32_within_half_the_bound(shape, drop):
    H, k, d, D, T = shape
    c = ref.attn_case(H, k, d, D, T)
    keep = _keep(c, H, k, drop)
    dn0 = torch.randn(c['R'], k, d, generator=torch.Generator().manual_seed(3))
    args = (c['qf'], c['probs'], c['dzbar'], c['nbrf'], c['ex'], c['seed_t'], c['nbr_t'], c['tw'], c['tb'], c['scale'], keep, c['no_valid'], dn0)
    want = ref.attn_backward(*args)
    got = ref.attn_backward(*args, dtype=torch.float32)
    ratios = _attn_ratios(got, want, H, k, c['C'])
    print(f'[float32] {shape} drop={drop}: ' + ', '.join(f'{n} {v:.3f}' for n, v in ratios.items()))
    assert max(ratios.values()) <= 0.5, ratios


# ---------------------------------------------------------------------------------------------------------------------------
# the bars notice what they must
# ---------------------------------------------------------------------------------------------------------------------------
# (a mutation that cannot change anything at a shape -- the other head of one, the neighbour of a single slot -- is not a case)
@pytest.mark.parametrize('shape,mutation', [(s, m) for s in ref.ATTN_SHAPES for m, applies in ref.MUTATIONS.items() if applies(s[0], s[1], True)], ids=str)
def test_attn_backward_mutations_break_the_bound(shape, mutation):
    H, k, d, D, T = shape
    drop = True
    c = ref.attn_case(H, k, d, D, T)
    keep = _keep(c, H, k, drop)
    dn0 = torch.randn(c['R'], k, d, generator=torch.Generator().manual_seed(3))
    args = (c['qf'], c['probs'], c['dzbar'], c['nbrf'], c['ex'], c['seed_t'], c['nbr_t'], c['tw'], c['tb'], c['scale'], keep, c['no_valid'], dn0)
    want = ref.attn_backward(*args)
    got = ref.attn_backward(*args, mutate=mutation)
    ratios = _attn_ratios(got, want, H, k, c['C'])
    assert max(ratios.values()) > 1.0, f'{mutation} passes at {shape}: {ratios}'


@pytest.mark.parametrize('mutation', ['drop_row_R-1', 'count_one_row_twice'])
def test_row_mutations_break_the_gemm_bar(mutation):
    for R, M, N, batch in ref.SGEMM_TN_CASES:
        if R == 0:
            continue  # no row to drop or double
        g = torch.Generator().manual_seed(R + M)
        A, B = torch.randn(batch, R, M, generator=g), torch.randn(batch, R, N, generator=g)
        A2, B2 = (A[:, :-1], B[:, :-1]) if mutation == 'drop_row_R-1' else (torch.cat([A, A[:, R // 2:R // 2 + 1]], 1), torch.cat([B, B[:, R // 2:R // 2 + 1]], 1))
        assert float((ref.sgemm_tn(A2, B2)[0] - ref.sgemm_tn(A, B)[0]).abs().max()) > ref.gemm_bar(R), (mutation, R, M, N)
    for R, C in ref.COLSUM_CASES:
        if R == 0:
            continue
        x = torch.randn(R, C, generator=torch.Generator().manual_seed(R + C))
        x2 = x[:-1] if mutation == 'drop_row_R-1' else torch.cat([x, x[R // 2:R // 2 + 1]])
        assert float((ref.colsum(x2)[0] - ref.colsum(x)[0]).abs().max()) > ref.gemm_bar(R), (mutation, R, C)


def test_all_pad_forward_needs_every_slot_once_the_slots_differ():
    """The forward's shortcut for a row without a valid slot reads ONE slot: zbar = (sum_s keep[s] / k) * z[0].  That is the uniform
    average sum_s (keep[s] / k) z[s] exactly when the k slots coincide (the leaf layer; any layer without dropout).  In train mode the
    k slots of such a row of a layer above the leaves are k rows of the layer below with equal inputs and their OWN dropout masks:
    they differ, and so does the average -- by the order of the values themselves.  (Hence the slot comparison in csrc/tgat.hip.)"""
    g = torch.Generator().manual_seed(2)
    k, C = 5, 7
    keep = (torch.rand(k, generator=g, dtype=F64) >= 0.25).double() / 0.75
    z_same = torch.randn(1, C, generator=g, dtype=F64).expand(k, C)
    lower_keep = (torch.rand(k, C, generator=g, dtype=F64) >= 0.1).double() / 0.9  # the layer below: one mask per row
    z_diff = z_same * lower_keep
    shortcut = lambda z: keep.sum() / k * z[0]
    full = lambda z: (keep[:, None] / k * z).sum(0)
    assert float((shortcut(z_same) - full(z_same)).abs().max()) <= 1e-15
    assert float((shortcut(z_diff) - full(z_diff)).abs().max()) > 1e-2
