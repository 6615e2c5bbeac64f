"""HistoricalNegativeEdgeSamplerHook on host tensors: the g25 fixtures recorded from the reference, the reference's own test file run in place,
and the draw as defined -- history[umulhi32(counter_u32(seed, call, source), n)] -- for uniformity and reproducibility."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import histneg_cases as hc
from tgm_amd.hooks import HistoricalNegativeEdgeSamplerHook
from tgm_amd.hooks.negatives import counter_u32, historical_draw, pool_words_bound
from tgm_amd.hooks.registry import list_hooks

REPLAY = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'replay_reference_histneg.py')


def test_every_scenario_has_its_fixture():
    assert hc.FIXTURES == sorted(f'g25_histneg_{n}' for n in hc.EXPECTED)


@pytest.mark.parametrize('name', hc.FIXTURES)
def test_host_path_against_fixture(name):
    hc.replay(name, 'cpu')


def test_reference_test_file_in_place():
    """test/unit/test_hooks/test_negative_edge_sampler_hook.py of the reference, unedited, with ``tgm`` aliased to ``tgm_amd``"""
    r = subprocess.run([sys.executable, REPLAY], capture_output=True, text=True)
    if r.returncode == 77:
        pytest.skip('no reference checkout')
    print(r.stdout, r.stderr)
    assert r.returncode == 0


def test_surface():
    h = HistoricalNegativeEdgeSamplerHook()
    assert h.has_state and h.requires == {'edge_src', 'edge_dst', 'edge_time'} and h.produces == {'neg', 'neg_time', 'valid_neg_mask'}
    assert HistoricalNegativeEdgeSamplerHook(id='foo').produces == {'neg_foo', 'neg_time_foo', 'valid_neg_mask_foo'}
    assert HistoricalNegativeEdgeSamplerHook in list_hooks()
    import tgm_amd.hooks.negatives as m  # the reference's path is tgm.hooks.negatives

    assert m.HistoricalNegativeEdgeSamplerHook is HistoricalNegativeEdgeSamplerHook
    h.check()  # nothing to report on the host path


def test_counter_restatement():
    """counter_u32 in Python integers against the arithmetic of csrc/common.h done in uint64"""
    def in_u64(seed, stream, i):
        with np.errstate(over='ignore'):
            u = np.uint64
            x = u(seed) ^ (u(stream) * u(0x9E3779B97F4A7C15)) ^ (u(i) * u(0xD1B54A32D192ED03))
            x = x + u(0x9E3779B97F4A7C15)
            x = (x ^ (x >> u(30))) * u(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> u(27))) * u(0x94D049BB133111EB)
            x = x ^ (x >> u(31))
            return int(x >> u(32))

    for seed, stream, i in [(0, 1, 0), (12345, 4096, 1_000_003), ((1 << 63) + 7, 17, 3), ((1 << 64) - 1, (1 << 40) + 1, (1 << 31) - 1)]:
        assert counter_u32(seed, stream, i) == in_u64(seed, stream, i)
    assert all(0 <= historical_draw(5, c, 9, 7) < 7 for c in range(1, 200))


HISTORY = [10] * 1 + [11] * 2 + [12] * 4 + [13] * 9


@pytest.mark.parametrize('seed', [0, 12345, (1 << 63) + 7])
@pytest.mark.parametrize('source', [3, 0, 1_000_003])
def test_draw_is_uniform_over_events(seed, source):
    """Pearson's statistic of 4096 calls over the four destinations (seen 1, 2, 4 and 9 times) against the 0.999 quantile of chi^2 with 3
    degrees of freedom.  Measured: 0.18 to 4.42 over these nine cases."""
    n = len(HISTORY)
    got = np.bincount([HISTORY[historical_draw(seed, c, source, n)] for c in range(1, 4097)], minlength=14)[10:]
    expect = 4096 * np.array([1, 2, 4, 9]) / n
    stat = float(((got - expect) ** 2 / expect).sum())
    print(f'seed {seed} source {source}: counts {got.tolist()}, statistic {stat:.2f}')
    assert stat <= 16.27


def test_hook_draws_what_the_definition_says():
    """the host path end to end: call c draws history[historical_draw(seed, c, s, n)] of the events offered before call c"""
    rng = np.random.default_rng(2511)
    calls = [(rng.integers(0, 6, 20), rng.integers(100, 200, 20), np.arange(c * 20, c * 20 + 20)) for c in range(8)]
    _, out = hc.run_stream(calls, 'cpu', seed=99)
    past = {}
    for c, ((s, d, _), (neg, _, _, _)) in enumerate(zip(calls, out), start=1):
        if c > 1:
            want = [past[v][historical_draw(99, c, v, len(past[v]))] if v in past else -1 for v in s.tolist()]
            assert neg.tolist() == want
        for a, b in zip(s.tolist(), d.tolist()):
            past.setdefault(a, []).append(b)


def test_draws_are_reproducible():
    rng = np.random.default_rng(2512)
    calls = [(rng.integers(0, 5, 30), rng.integers(0, 1000, 30), np.arange(c * 30, c * 30 + 30)) for c in range(6)]
    negs = lambda out: torch.cat([o[0] for o in out[1:]])
    (_, a), (_, b), (_, other) = hc.run_stream(calls, 'cpu', seed=1), hc.run_stream(calls, 'cpu', seed=1), hc.run_stream(calls, 'cpu', seed=2)
    assert torch.equal(negs(a), negs(b)) and not torch.equal(negs(a), negs(other))
    torch.manual_seed(1)  # without a seed: torch.initial_seed(), read at the first draw
    _, unseeded = hc.run_stream(calls, 'cpu', seed=None)
    assert torch.equal(negs(unseeded), negs(a))
    # a second epoch after reset_state(): the call count runs on, so the draws differ
    dg = hc.stream_graph(calls, 'cpu')
    hook = HistoricalNegativeEdgeSamplerHook(seed=1)
    epochs = []
    for _ in range(2):
        hook.reset_state()
        epochs.append(torch.cat([hook(dg, hc.batch_of(s, d, t, dg.device)).neg for s, d, t in calls][1:]))
    assert torch.equal(epochs[0], negs(a)) and not torch.equal(epochs[0], epochs[1])
    assert torch.equal(epochs[0] != -1, epochs[1] != -1)


def test_empty_batch_changes_nothing():
    calls = [([1, 2], [3, 4], [0, 1]), ([1], [5], [2])]
    dg = hc.stream_graph(calls, 'cpu')
    hook = HistoricalNegativeEdgeSamplerHook(seed=3)
    empty = lambda: hc.batch_of([], [], [], dg.device)
    b = hook(dg, empty())
    assert b.neg.shape == (0,) and b.neg_time.shape == (0,) and b.valid_neg_mask.shape == (0,) and hook._memory is None and hook._calls == 0
    hook(dg, hc.batch_of(*calls[0], dg.device))
    mem, calls_before = hook._memory.clone(), hook._calls
    b = hook(dg, empty())
    assert b.neg.dtype == torch.int32 and b.valid_neg_mask.dtype == torch.bool and hook._count == 2 and hook._calls == calls_before
    assert torch.equal(hook._memory, mem)
    assert hook(dg, hc.batch_of(*calls[1], dg.device)).neg.tolist() == [3]


def test_pool_bound_covers_every_layout():
    """the segments a source with n events owns (1 header + 4 2^k slots each) against the bound the host sizes the pool from"""
    def words(n):
        k_last = ((n - 1) // 4 + 1).bit_length() - 1
        return sum(1 + (4 << k) for k in range(k_last + 1))

    for n in list(range(1, 300)) + [4 * (2 ** k - 1) + j for k in range(3, 20) for j in (0, 1, 2)]:
        assert words(n) <= pool_words_bound(n, 1) - 1
        assert 7 * words(n) + 3 * words(1) <= pool_words_bound(7 * n + 3, 10) - 1
    assert 50 * words(1) <= pool_words_bound(50, 1000) - 1
