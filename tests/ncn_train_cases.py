"""The inputs the NCNPredictor training tests share (tests/test_ncn_train_cpu.py asserts on the CPU what tests/test_ncn_train_gpu.py relies on):
everything is drawn from seeds, nothing from a device result.

    DX_CASES    name -> builder of one ``tgmx_ncn_dx`` case: graph shapes (one node, no edge, rows of 0 / 1 / 63 / 64 / 65 entries, the hub of the
                g18 fixtures, a row one entry past the kernel's long-row threshold) x pair sets (none, one, one-vs-many, i = j, a self-loop,
                an edge in both directions, ids outside [0, N)) x C in {1, 7, 64, 257} x k x decay x the dtype of the targets
    GPU_CASES   name -> builder of one end-to-end case (the g31 fixtures, two g18 fixtures' inputs, small random ones)
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Callable, Dict

import torch

import ncn_bwd_restate as br
import ncn_restate as nr
from golden_util import load

LONG_ROW = br.LONG_ROW


def _shapes(C: int, k: int, H: int, out: int) -> dict:
    return {'xslin.weight': [out, k * C], 'xslin.bias': [out], 'xsmlp.0.weight': [H, k * C], 'xsmlp.0.bias': [H], 'xsmlp.2.weight': [out, H],
            'xsmlp.2.bias': [out]}  # fmt: skip


def _times(N: int, B: int, g) -> tuple:
    return torch.randint(0, 50_000, (N,), generator=g), torch.randint(40_000, 90_000, (B,), generator=g)


def make(x, ei, tar, k: int, seed: int, decay: bool = False, dup: str = 'last', H: int = 8, out: int = 1, sd=None, dout=None, lu=None, et=None):
    N, C = x.shape
    B = tar.shape[1]
    g = torch.Generator().manual_seed(seed + 77)
    if decay and lu is None:
        lu, et = _times(N, B, g)
    if not decay:
        lu = et = None
    if sd is None:
        sd = nr.hashed_state_dict(_shapes(C, k, H, out), seed)
    H, out = sd['xsmlp.0.weight'].shape[0], sd['xsmlp.2.weight'].shape[0]
    if dout is None:
        dout = torch.from_numpy(nr.hashed_uniform(B * out, seed * 1000 + 500).copy())
    dxs = torch.from_numpy(nr.hashed_uniform(B * k * C, seed * 1000 + 501).reshape(B, k * C).copy())
    return SimpleNamespace(x=x, ei=ei, tar=tar, k=k, lu=lu, et=et, dup=dup, sd=sd, dout=dout, dxs=dxs, N=N, C=C, H=H, out=out, B=B, decay=decay)


# ---- graphs ---------------------------------------------------------------------------------------------------------------------------------
def small_graph(seed: int, N: int = 12, E: int = 40, B: int = 9):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N, (2, E), generator=g)
    tar = torch.randint(0, 5, (2, B), generator=g)  # few ids: duplicates on both sides, and pairs with i = j
    tar[1, B // 2 :] += 3
    return N, ei, tar


def rows_graph():
    """rows of 0 (node 0), 1 (node 1), 63, 64 and 65 (nodes 2, 3, 4) entries; the leaves of nodes 2, 3, 4 overlap: common neighbours exist"""
    src, dst, leaf = [], [], 10
    for node, deg in ((1, 1), (2, 63), (3, 64), (4, 65)):
        src += [node] * deg
        dst += list(range(leaf, leaf + deg))
        leaf += 40  # the leaves overlap between the nodes: common neighbours exist
    N = max(dst) + 1
    tar = torch.tensor([[2, 3, 4, 4, 1, 0, 2, 20, 60], [3, 4, 2, 4, 2, 3, 50, 95, 60]])
    return N, torch.tensor([src, dst]), tar


def past_threshold_graph():
    """node 5's row has LONG_ROW + 1 entries (neighbours repeated about 13 times each) and does not start on a chunk boundary"""
    src = [5] * (LONG_ROW + 1) + [0, 1, 2, 3, 0]
    dst = [6 + e % 39 for e in range(LONG_ROW + 1)] + [1, 2, 3, 4, 4]
    tar = torch.tensor([[5, 7, 5, 6, 1, 5], [9, 5, 5, 8, 3, 0]])
    return 45, torch.tensor([src, dst]), tar


# ---- tgmx_ncn_dx alone ----------------------------------------------------------------------------------------------------------------------
def _dx(graph: Callable, C: int, k: int, decay: bool, seed: int, dup: str = 'last', tar64: bool = True, edit: Callable = None) -> Callable:
    def build():
        N, ei, tar = graph()
        if edit is not None:
            N, ei, tar = edit(N, ei.clone(), tar.clone())
        c = make(nr.hashed_x(N, C, seed), ei, tar, k, seed, decay, dup)
        c.tar64 = tar64
        return c

    return build


def _one_vs_many(N, ei, tar):
    g = torch.Generator().manual_seed(5)
    return N, ei, torch.stack([torch.full((65,), 4), torch.randint(0, N, (65,), generator=g)])


def _same_pair(N, ei, tar):
    tar[1, 1], tar[1, -1] = tar[0, 1], tar[0, -1]
    return N, ei, tar


def _self_loop(N, ei, tar):
    ei[:, 3] = tar[0, -1]
    ei[:, 17] = 7
    tar[1, 2] = 7
    return N, ei, tar


def _both_ways(N, ei, tar):
    ei[0, 5], ei[1, 5] = ei[1, 4].item(), ei[0, 4].item()
    tar[0, -1], tar[1, -1] = ei[0, 4].item(), ei[1, 4].item()
    return N, ei, tar


def _outside(N, ei, tar):
    tar[0, 0], tar[1, 2], tar[0, 4], tar[1, 4] = -1, N, N + 5, -3  # one side, the other, both; the rest stay (and stay 'last' among themselves)
    ei[0, 1], ei[1, 6], ei[0, 9] = -2, N, 2**31 - 1
    return N, ei, tar


def _hub(k: int):
    def graph():
        meta, a = load(f'g18_ncn_hub_k{k}')
        return meta['N'], torch.from_numpy(a['edge_index']), torch.from_numpy(a['tar_ei'])

    return graph


_small = lambda seed: (lambda: small_graph(seed))
DX_CASES: Dict[str, Callable] = {
    'one_node_c7_k2': _dx(lambda: (1, torch.zeros((2, 3), dtype=torch.long), torch.zeros((2, 2), dtype=torch.long)), 7, 2, False, 11),
    'one_node_c1_k4_decay': _dx(lambda: (1, torch.zeros((2, 3), dtype=torch.long), torch.zeros((2, 2), dtype=torch.long)), 1, 4, True, 12),
    'no_edge_c64_k4': _dx(lambda: (12, torch.zeros((2, 0), dtype=torch.long), small_graph(13)[2]), 64, 4, False, 13),
    'no_edge_c1_k2_decay_i32': _dx(lambda: (12, torch.zeros((2, 0), dtype=torch.long), small_graph(14)[2]), 1, 2, True, 14, tar64=False),
    'rows_c7_k4_decay_all': _dx(rows_graph, 7, 4, True, 15, dup='all'),
    'rows_c257_k2': _dx(rows_graph, 257, 2, False, 16),
    'rows_c64_k4_i32': _dx(rows_graph, 64, 4, False, 17, tar64=False),
    'hub_c64_k2_decay': _dx(_hub(2), 64, 2, True, 18),
    'hub_c257_k4_all': _dx(_hub(4), 257, 4, False, 19, dup='all'),
    'hub_c1_k4_decay_i32': _dx(_hub(4), 1, 4, True, 20, tar64=False),
    'past_threshold_c7_k4_decay_all': _dx(past_threshold_graph, 7, 4, True, 21, dup='all'),
    'past_threshold_c257_k2': _dx(past_threshold_graph, 257, 2, False, 22),
    'no_pair_c7_k4': _dx(_small(23), 7, 4, False, 23, edit=lambda N, ei, tar: (N, ei, tar[:, :0])),
    'one_pair_c64_k2_decay': _dx(_small(24), 64, 2, True, 24, edit=lambda N, ei, tar: (N, ei, tar[:, :1])),
    'one_pair_c1_k4': _dx(_small(25), 1, 4, False, 25, edit=lambda N, ei, tar: (N, ei, tar[:, 3:4])),
    'one_vs_many_all_c7_k4_decay': _dx(_small(26), 7, 4, True, 26, dup='all', edit=_one_vs_many),
    'one_vs_many_last_c7_k4_decay': _dx(_small(26), 7, 4, True, 26, dup='last', edit=_one_vs_many),
    'one_vs_many_all_c257_k2_i32': _dx(_small(27), 257, 2, False, 27, dup='all', tar64=False, edit=_one_vs_many),
    'same_pair_c7_k4_decay': _dx(_small(28), 7, 4, True, 28, edit=_same_pair),
    'same_pair_c64_k2_all': _dx(_small(29), 64, 2, False, 29, dup='all', edit=_same_pair),
    'self_loop_c7_k4': _dx(_small(30), 7, 4, False, 30, edit=_self_loop),
    'self_loop_c1_k2_decay_all': _dx(_small(31), 1, 2, True, 31, dup='all', edit=_self_loop),
    'both_ways_c64_k4_decay': _dx(_small(32), 64, 4, True, 32, edit=_both_ways),
    'outside_c7_k4_decay': _dx(_small(33), 7, 4, True, 33, edit=_outside),
    'outside_c64_k2_all_i32': _dx(_small(34), 64, 2, False, 34, dup='all', tar64=False, edit=_outside),
}


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def _g31(name: str) -> Callable:
    def build():
        meta, sd, inp, dout, ref = br.load_grad_fixture(name)
        c = make(inp['x'], inp['edge_index'], inp['tar_ei'], meta['k'], 0, meta['decay'], sd=sd, dout=dout, lu=inp['last_update'], et=inp['edge_time'])
        c.ref = ref
        return c

    return build


def _g18(name: str, seed: int) -> Callable:
    def build():
        meta, a = load(name)
        return make(nr.fixture_x(meta, a), torch.from_numpy(a['edge_index']), torch.from_numpy(a['tar_ei']), meta['k'], seed,
                    sd=nr.fixture_state_dict(meta, a))  # fmt: skip

    return build


def random_case(seed: int, k: int = 4, decay: bool = True, out_of_range: bool = False, dup: str = 'last', H: int = 8, out: int = 1, C: int = 5):
    N, ei, tar = small_graph(100 + seed)
    if out_of_range:
        N, ei, tar = _outside(N, ei, tar)
    return make(nr.hashed_x(N, C, 100 + seed), ei, tar, k, 100 + seed, decay, dup, H=H, out=out)


GPU_CASES: Dict[str, Callable] = {f'g31_{n}': _g31(n) for n in br.EXPECTED_GRAD_FIXTURES}
GPU_CASES.update({
    'hub_k4': _g18('g18_ncn_hub_k4', 41),
    'width_c256_h100_o3': _g18('g18_ncn_width_c256_h100_o3', 42),
    'rand_k4_decay': lambda: random_case(1),
    'rand_k2_all': lambda: random_case(2, k=2, decay=False, dup='all'),
    'rand_outside': lambda: random_case(3, out_of_range=True),
    'rand_out3': lambda: random_case(4, out=3),
    'rand_out17': lambda: random_case(5, out=17),  # above the tail route: the generic last layer
    'pos': lambda: random_case(6),
    'neg': lambda: _negatives(random_case(6)),
})  # fmt: skip


def _negatives(c):
    """the same step's second call: the same x, edges, times and weights, other destinations"""
    g = torch.Generator().manual_seed(606)
    tar = torch.stack([c.tar[0], torch.randint(0, c.N, (c.B,), generator=g)])
    n = make(c.x, c.ei, tar, c.k, 606, c.decay, c.dup, sd=c.sd, lu=c.lu, et=c.et)
    return n


def tensors(c, device, tar64: bool = True):
    """(x, edge_index, tar_ei, last_update, edge_time) on the device"""
    mv = lambda t: None if t is None else t.to(device)
    tar = c.tar if tar64 else c.tar.to(torch.int32)
    return mv(c.x), mv(c.ei), mv(tar), mv(c.lu), mv(c.et)


__all__ = ['DX_CASES', 'GPU_CASES', 'make', 'random_case', 'tensors']
