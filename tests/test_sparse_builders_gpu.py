"""What the three sorted-key CSR builders share (csrc/edge_csr.h: the key scheme, the sort's bit range, the row pointers by binary search,
the columns from the keys): on one edge list without self loops ``tgmx_cheb_laplacian``, ``tgmx_gcn_norm_csr`` without self loops and
``tgmx_ncn_adj_build`` produce the same keys, and equal keys carry equal columns, so their ``indptr`` and ``cols`` agree word for word.

The list: a hub row of 2049 entries (longer than the propagate's very-long-row threshold, several blocks of the rows kernel), duplicates,
endpoints -1 and N (dropped: they sort behind every row), N = 65 and N = 64 (the key's column field is 7 and 6 bits wide).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HUB = 2049


def edge_list(N, dtype):
    g = torch.Generator().manual_seed(N)
    hub = 7
    hub_src = torch.randint(0, N - 1, (HUB,), generator=g)
    hub_src[hub_src >= hub] += 1  # every id but the hub's own: no self loop
    src = torch.randint(0, N, (240,), generator=g)
    dst = (src + torch.randint(1, N, (240,), generator=g)) % N  # never src itself
    src, dst = torch.where(dst == hub, dst, src), torch.where(dst == hub, src, dst)  # turned round: the hub row keeps exactly HUB entries
    src[:40], dst[:40] = src[40:80].clone(), dst[40:80].clone()  # duplicates
    src[200:205], dst[205:210] = -1, -1
    src[210:215], dst[215:220] = N, N
    src, dst = torch.cat([hub_src, src]), torch.cat([torch.full((HUB,), hub), dst])
    p = torch.randperm(src.numel(), generator=g)
    ei = torch.stack([src[p], dst[p]]).to(dtype)
    inside = (ei >= 0).all(0) & (ei < N).all(0)
    assert not (ei[0] == ei[1]).any() and int((inside & (ei[1] == hub)).sum()) == HUB
    return ei, int(inside.sum())


def rows(indptr, cols, N):
    indptr = indptr[: N + 1].cpu()
    return indptr, cols[: int(indptr[N])].cpu()


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64], ids=['int32', 'int64'])
@pytest.mark.parametrize('N', [65, 64])
def test_builders_agree_on_rows_and_columns(N, dtype):
    from tgm_amd.nn._snapshot import gcn_norm_csr, scaled_laplacian
    from tgm_amd.nn.ncn import adjacency

    ei, kept = edge_list(N, dtype)
    ei = ei.to(DEV)
    gcn_ip, gcn_cols = rows(*gcn_norm_csr(ei, None, N, 1.0, False)[:2], N)
    assert int(gcn_ip[N]) == kept and int(gcn_ip[8] - gcn_ip[7]) == HUB
    cheb_ip, cheb_cols = rows(*scaled_laplacian(ei, None, N, 'sym', 2.0, None)[:2], N)
    assert torch.equal(cheb_ip, gcn_ip) and torch.equal(cheb_cols, gcn_cols)

    doubled = torch.stack([torch.cat([ei[0], ei[1]]), torch.cat([ei[1], ei[0]])])
    both_ip, both_cols = rows(*gcn_norm_csr(doubled, None, N, 1.0, False)[:2], N)
    adj = adjacency(N, ei)
    ncn_ip, ncn_cols = rows(adj.indptr, adj.cols, N)
    assert int(ncn_ip[N]) == 2 * kept
    assert torch.equal(ncn_ip, both_ip) and torch.equal(ncn_cols, both_cols)
