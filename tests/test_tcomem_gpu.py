"""tCoMemPredictor on the device: every g20 fixture replayed (window, rings, len, pos, popularity and pair counts after every call, every
query by the project's score criterion, integer queries as the base score alone, one-against-many against the per-positive calls), update
and constructor sizes across the wave edges and the 1024-event launch boundary with ring lengths around the wave width, contention on one
source / one pair / self-loops, growth through rehashes, a probe that wraps past the end of the table, determinism, id widths, every status
bit, the integer-query switch, and that a batch reads nothing back.

Every score check prints HIP's distance from float64 (max |got - ref| / max(1, |ref|)) next to the reference's own float32 distance and
their ratio; the measured figures are in DESIGN.md 3.9.
"""
import numpy as np
import pytest
import torch

import tcomem_restate as tr
from golden_util import load
from test_tcomem_cpu import BAR, EXPECTED, calls_of, check_scores, nested_of, queries_of, state_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TORCH = {'int64': torch.int64, 'int32': torch.int32, 'float32': torch.float32, 'float64': torch.float64}
FAR = 1 << 30  # a destination no stream here holds (and float32 holds exactly): its pair count is 0


def dev(a, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a, dtype=np.int64)).to(dtype).to(DEV)


def new_model(*args, **kw):
    from tgm_amd.nn import tCoMemPredictor

    return tCoMemPredictor(*args, **kw)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def nested(model):
    return {a: dict(row) for a, row in model.node_to_co_occurrence.items()}


def assert_state(model, restated):
    """window, rings, len, pos, popularity and pair counts against the restatement, exactly"""
    assert (model.window_start, model.window_end, model.window_size) == (restated.window_start, restated.window_end, restated.window_size)
    assert np.array_equal(model.recent_ts.numpy(), restated.recent_ts) and np.array_equal(model.recent_dst.numpy(), restated.recent_dst)
    assert np.array_equal(model.recent_len.numpy(), restated.len) and np.array_equal(model.recent_pos.numpy(), restated.pos)
    assert np.array_equal(model.popularity.numpy(), restated.pop)
    assert nested(model) == restated.nested_counts()
    model.check()


def assert_scores(model, restated, pairs, what):
    qs, qd = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    for dtype in ('int64', 'float32'):
        got = model(dev(qs, TORCH[dtype]), dev(qd, TORCH[dtype]))
        assert got.dtype == torch.float32
        e = tr.rel_err(got.cpu().numpy(), restated.scores64(qs, qd, dtype))
        print(f'{what} ({dtype}): HIP vs float64 {e:.3e}')
        assert e < BAR


@pytest.mark.parametrize('name', ['g20_tcomem_' + n for n in EXPECTED])
def test_fixture_replayed(name):
    meta, a = load(name)
    sd = TORCH[meta['stream_dtype']]
    model = None
    for c, (s, d, t) in enumerate(calls_of(meta, a)):
        if model is None:
            model = new_model(dev(s, sd), dev(d, sd), dev(t, sd), meta['num_nodes'], meta['k'], meta['window_ratio'], meta['co_occurrence_weight'])
        else:
            model.update(dev(s, sd), dev(d, sd), dev(t, sd))
        assert (model.window_start, model.window_end, model.window_size) == (a['window_start'][c], a['window_end'][c], a['window_size'][c])
        assert isinstance(model.window_start, float) and isinstance(model.window_size, int) and model.window_ratio == meta['window_ratio']
        ts, dst, ln, pos, pop = state_of(a, c)
        for got, want in ((model.recent_ts, ts), (model.recent_dst, dst), (model.recent_len, ln), (model.recent_pos, pos), (model.popularity, pop)):
            assert got.device.type == 'cpu' and got.numpy().dtype == want.dtype and np.array_equal(got.numpy(), want)
        assert nested(model) == nested_of(a, c)
        for j, (qs, qd, pred, pred64, dtype, rows) in enumerate(queries_of(meta, a, c)):
            qs_d, qd_d = dev(qs, TORCH[dtype]), dev(qd, TORCH[dtype])
            got = model(qs_d, qd_d)
            assert got.dtype == torch.float32 and got.device == qs_d.device and got.shape == qs_d.shape
            check_scores(name, f'call {c} query {j} ({dtype}), HIP', got.cpu().numpy(), pred64)
            if dtype in tr.INTEGER_QUERIES:  # the base score alone: what a pair that was never counted answers
                assert torch.equal(got, model(qs_d, torch.full_like(qd_d, FAR)))
                assert torch.equal(got, model(qs_d.float(), torch.full_like(qd_d, FAR).float()))
            if rows:  # recorded in the one-against-many form
                src, dst_, neg = qs_d[::rows], qd_d[::rows], qd_d.view(-1, rows)[:, 1:]
            else:  # made into one: every query's source against its destination and three other destinations
                src, dst_, neg = qs_d, qd_d, torch.stack([qd_d.roll(1), qd_d.roll(2), qd_d.roll(5)], 1)
            many = model.query_one_vs_many(src, dst_, neg)
            assert many.shape == (len(src), neg.shape[1] + 1) and many.dtype == torch.float32
            if rows:
                assert torch.equal(many.view(-1), got)
            ragged = [neg[b, : (b * 7) % (neg.shape[1] + 1)] for b in range(len(src))]  # lengths 0 .. M, row 0 empty
            take = range(0, len(src), max(1, len(src) // 40))  # the per-positive loop over a spread of rows
            each = {b: model(src[b].repeat(len(ragged[b]) + 1), torch.cat([dst_[b].unsqueeze(0), ragged[b]])) for b in take}
            as_list = model.query_one_vs_many(src, dst_, ragged)
            assert len(as_list) == len(src)
            for b in range(len(src)):
                assert same(as_list[b], many[b, : len(ragged[b]) + 1])
            for b in take:
                assert same(as_list[b], each[b])
        model.check()


def test_empty_query_answers_an_empty_float32_tensor():
    model = new_model(dev([1]), dev([2]), dev([1]), 10, 5)
    for dtype in TORCH.values():
        got = model(dev([], dtype), dev([], dtype))
        assert got.dtype == torch.float32 and got.shape == (0,)
    assert model.query_one_vs_many(dev([]), dev([]), []) == []
    assert model.query_one_vs_many(dev([]), dev([]), dev([]).view(0, 4)).shape == (0, 5)


N_NODES, SOURCES = 80, 8


def random_events(rng, n, t_lo, t_hi):
    """8 sources, so that a call of more than 8 k events puts more than k on one source; timestamps in no order"""
    return rng.integers(0, SOURCES, n), rng.integers(SOURCES - 2, N_NODES, n), rng.integers(t_lo, t_hi, n)


SOME_PAIRS = [(s, d) for s in range(SOURCES + 1) for d in range(SOURCES - 2, N_NODES, 3)]


@pytest.mark.parametrize('k', [1, 2, 50, 63, 64, 65])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 1024, 1025, 5000])
def test_update_sizes_against_the_restatement(n, k):
    rng = np.random.default_rng(1000 * k + n)
    s0, d0, t0 = random_events(rng, 100, 0, 1000)
    s1, d1, t1 = random_events(rng, n, 600, 1300)
    s2, d2, t2 = random_events(rng, 40, 1000, 1500)
    model, restated = new_model(dev(s0), dev(d0), dev(t0), N_NODES, k), tr.TCoMemRestated(s0, d0, t0, N_NODES, k)
    assert_state(model, restated)
    for s, d, t in ((s1, d1, t1), (s2, d2, t2)):
        model.update(dev(s), dev(d), dev(t))
        restated.update(s, d, t)
        assert_state(model, restated)
    if n > SOURCES * k:
        assert np.bincount(s1, minlength=SOURCES).max() > k
    assert_scores(model, restated, SOME_PAIRS, f'n={n} k={k}')


@pytest.mark.parametrize('k', [3, 64, 65])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 1024, 1025, 5000])
def test_constructor_sizes_against_the_restatement(n, k):
    rng = np.random.default_rng(n + k)
    s, d, t = random_events(rng, n, 0, 100_000)
    model, restated = new_model(dev(s), dev(d), dev(t), N_NODES, k), tr.TCoMemRestated(s, d, t, N_NODES, k)
    assert model.rehashes == 0
    assert_state(model, restated)
    assert_scores(model, restated, SOME_PAIRS, f'constructor n={n} k={k}')


@pytest.mark.parametrize('n', [1024, 1025])
@pytest.mark.parametrize('case', ['one_source', 'one_pair', 'self_loops'])
def test_contention(case, n):
    """every event on one ring, on one counter, or on one counter twice"""
    ts = np.random.default_rng(7).permutation(n) + 10
    src = np.full(n, 3)
    dst = {'one_source': np.arange(n) % 60 + 4, 'one_pair': np.full(n, 4), 'self_loops': np.full(n, 3)}[case]
    first = ([1, 5], [2, 6], [0, 5000])
    model, restated = new_model(*(dev(v) for v in first), 70, 50), tr.TCoMemRestated(*first, 70, 50)
    model.update(dev(src), dev(dst), dev(ts))
    restated.update(src, dst, ts)
    assert_state(model, restated)
    counts = nested(model)
    if case == 'one_pair':
        assert counts[3] == {4: n} and counts[4] == {3: n}
    if case == 'self_loops':
        assert counts[3] == {3: 2 * n}
    assert model.recent_len[3] == 50 and model.recent_pos[3] == n % 50 and model.popularity.sum() == n + 2


def test_growth_through_rehashes_keeps_the_counts():
    from tgm_amd.nn.edgebank import grow_capacity

    s0, d0, t0 = [0, 1, 2], [100, 101, 102], [0, 5, 10]
    model, restated = new_model(dev(s0), dev(d0), dev(t0), 400, 4, capacity=8), tr.TCoMemRestated(s0, d0, t0, 400, 4)
    assert model.capacity == 8
    capacity, offered, kept, rehashes, nxt = 8, 3, 0, 0, 3
    for step in range(12):
        n = 2 + step
        s = np.arange(nxt, nxt + n) % 200
        d = 399 - s  # new pairs, and pairs counted again once the sources come round
        pairs_before = len(restated.counts)
        want = grow_capacity(capacity, offered, kept, n)
        model.update(dev(s), dev(d), dev(np.full(n, 10 + step)))
        restated.update(s, d, np.full(n, 10 + step))
        if want != capacity:
            assert model.capacity == want and model._kept == pairs_before  # every pair moved
            capacity, offered, kept, rehashes = want, 0, pairs_before, rehashes + 1
        offered += n
        assert model.capacity == capacity and model.rehashes == rehashes
        assert_state(model, restated)
        nxt += n
    assert rehashes >= 2
    model.update(dev(np.arange(3, 60)), dev(399 - np.arange(3, 60)), dev(np.full(57, 30)))
    restated.update(np.arange(3, 60), 399 - np.arange(3, 60), np.full(57, 30))
    assert_state(model, restated)
    assert max(restated.counts.values()) == 2


def test_probe_wraps_past_the_end_of_the_table():
    """forty counted and forty absent pairs whose probes all start in the last two slots of a 128-slot table"""
    found = []
    for s in range(2000):
        for d in range(s, s + 5):
            if tr.home_slot(s, d, 128) >= 126:
                found.append((s, d))
    assert len(found) >= 80
    stored, absent = found[:80:2], found[1:80:2]
    s, d = [p[0] for p in stored], [p[1] for p in stored]
    ts = np.arange(40) + 5
    model = new_model(dev(s), dev(d), dev(ts), 2100, 2, capacity=128)
    assert model.capacity == 128 and model.rehashes == 0
    slots = model._buf[:256].view(128, 2)[:, 0].cpu().numpy()
    assert (slots[:38] != -1).all() and (slots[126:] != -1).all() and (slots[38:126] == -1).all()  # the run wraps: 126, 127, 0 .. 37
    model.update(dev(d[:5]), dev(s[:5]), dev(ts[:5] + 100))  # found again through the wrap, from the other side: no second copy
    restated = tr.TCoMemRestated(s, d, ts, 2100, 2)
    restated.update(d[:5], s[:5], ts[:5] + 100)
    assert_state(model, restated)
    both = stored + absent
    qs, qd = np.array([p[0] for p in both]), np.array([p[1] for p in both])
    got = model(dev(qs, torch.float32), dev(qd, torch.float32)).cpu().numpy()
    assert tr.rel_err(got, restated.scores64(qs, qd, 'float32')) < BAR
    base = model(dev(qs), dev(qd)).cpu().numpy()
    assert ((got > base) == np.array([restated.count(*p) > 0 for p in both])).all()


def test_two_runs_leave_the_same_state_and_answers():
    rng = np.random.default_rng(13)
    batches = [random_events(rng, n, 100 * i, 100 * i + 400) for i, n in enumerate((3000, 200, 200, 1500, 200))]
    qs, qd = dev([p[0] for p in SOME_PAIRS], torch.float32), dev([p[1] for p in SOME_PAIRS], torch.float32)

    def run():
        model = new_model(*(dev(v) for v in batches[0]), N_NODES, 50, capacity=64)
        for b in batches[1:]:
            model.update(*(dev(v) for v in b))
        state = [model.recent_ts, model.recent_dst, model.recent_len, model.recent_pos, model.popularity]
        return state, nested(model), model(qs, qd).cpu(), model(qs.long(), qd.long()).cpu()

    (s0, c0, f0, i0), (s1, c1, f1, i1) = run(), run()
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(s0, s1))  # fmt: skip
    assert c0 == c1 and len(c0) > 50 and torch.equal(f0.view(torch.int32), f1.view(torch.int32)) and torch.equal(i0.view(torch.int32), i1.view(torch.int32))


def test_id_widths_give_the_same_state_and_answers():
    rng = np.random.default_rng(11)
    s, d, t = random_events(rng, 700, 0, 5000)
    models = [new_model(dev(s, w), dev(d, w), dev(t, tw), N_NODES, 20) for w, tw in
              ((torch.int64, torch.int64), (torch.int32, torch.int32), (torch.int32, torch.int64), (torch.float32, torch.float32))]  # fmt: skip
    restated = tr.TCoMemRestated(s, d, t, N_NODES, 20)
    qs, qd = np.array([p[0] for p in SOME_PAIRS]), np.array([p[1] for p in SOME_PAIRS])
    first = None
    for model in models:
        assert_state(model, restated)
        answers = {name: model(dev(qs, dt), dev(qd, dt)) for name, dt in TORCH.items()}
        assert all(v.dtype == torch.float32 for v in answers.values())
        assert torch.equal(answers['int32'], answers['int64'])
        assert torch.equal(model(dev(qs, torch.int32), dev(qd, torch.int64)), answers['int64'])  # the widths are read per argument
        for name, got in answers.items():
            assert tr.rel_err(got.cpu().numpy(), restated.scores64(qs, qd, name)) < BAR
        first = first or answers
        assert all(torch.equal(answers[name], first[name]) for name in TORCH)


def test_every_status_bit_is_raised_once_and_cleared():
    model = new_model(dev([1, 2]), dev([2, 3]), dev([5, 6]), 10, 3, capacity=4)
    restated = tr.TCoMemRestated([1, 2], [2, 3], [5, 6], 10, 3)
    assert_state(model, restated)

    def raises(match):
        with pytest.raises(ValueError, match=match):
            model.check()
        model.check()  # cleared by the check that raised
        assert_state(model, restated)  # and the flagged event contributed nothing

    model.update(dev([-1, 3]), dev([2, 2**31]), dev([7, 7]))
    raises('node ids must lie in')
    model.update(dev([10]), dev([2]), dev([7]))
    raises('source at or above num_nodes')
    model.update(dev([2]), dev([10]), dev([7]))
    raises('destination at or above num_nodes')
    assert model(dev([1, -1, 10, 1]), dev([2, 2, 2, -5])).cpu().tolist()[1:] == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match='node ids must lie in'):
        model.check()
    assert model(dev([10, 1]), dev([2, 11])).cpu().tolist()[0] == 0.0  # a query's destination only has to be an id
    raises('source at or above num_nodes')
    assert model.query_one_vs_many(dev([12]), dev([2]), dev([[3, 4]])).cpu().tolist() == [[0.0, 0.0, 0.0]]
    raises('source at or above num_nodes')


def test_a_full_table_sets_the_status_and_drops_the_events():
    """the host's growth rule keeps the table at most half full, so its bookkeeping is forced here: 4 slots, 2 pairs in them, 6 new pairs"""
    model = new_model(dev([1, 2]), dev([2, 3]), dev([5, 6]), 10, 3, capacity=4)
    assert model.capacity == 4
    model._offered = -100
    model.update(dev([4, 5, 6, 7, 8, 1]), dev([5, 6, 7, 8, 9, 9]), dev([8, 8, 8, 8, 8, 8]))
    assert model.capacity == 4 and model.rehashes == 0
    with pytest.raises(ValueError, match='ran through the whole pair table'):
        model.check()
    model.check()
    pairs = sum(len(row) for row in nested(model).values()) // 2
    assert pairs == 4 and model.popularity.sum() == 4 and model.recent_len.sum() == 4  # two of the six found room; the others left nothing


def test_integer_queries_can_take_the_float32_rule():
    rng = np.random.default_rng(19)
    s, d, t = random_events(rng, 600, 0, 3000)
    plain = new_model(dev(s), dev(d), dev(t), N_NODES, 50)
    switched = new_model(dev(s), dev(d), dev(t), N_NODES, 50, co_occurrence_on_integer_queries=True)
    qs, qd = dev([p[0] for p in SOME_PAIRS]), dev([p[1] for p in SOME_PAIRS])
    as_float = plain(qs.float(), qd.float())
    assert torch.equal(switched(qs, qd), as_float) and torch.equal(switched(qs.int(), qd.int()), as_float)
    assert torch.equal(switched(qs.float(), qd.float()), as_float) and not torch.equal(plain(qs, qd), as_float)
    neg = qd.view(-1, 1).roll(3, 0).repeat(1, 4)
    assert torch.equal(switched.query_one_vs_many(qs, qd, neg), plain.query_one_vs_many(qs.float(), qd.float(), neg.float()))


def test_a_batch_reads_nothing_back():
    """update and both query forms under torch's sync debug mode: any synchronising call of torch's raises"""
    rng = np.random.default_rng(17)
    s, d, t = random_events(rng, 500, 0, 1000)
    model = new_model(dev(s), dev(d), dev(t), N_NODES, 50, capacity=1 << 14)
    s1, d1, t1 = (dev(v) for v in random_events(rng, 200, 900, 1200))
    neg = dev(rng.integers(SOURCES, N_NODES, (200, 9)))
    rows = [neg[b, : b % 10] for b in range(200)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        flat = model(s1, d1)
        many = model.query_one_vs_many(s1, d1, neg)
        as_list = model.query_one_vs_many(s1, d1, rows)
        as_float = model.query_one_vs_many(s1.float(), d1.float(), neg.float())
        model.update(s1, d1, t1)
        after = model(s1.float(), d1.float())
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert model.rehashes == 0
    assert torch.equal(many[:, 0], flat) and all(torch.equal(r, many[b, : b % 10 + 1]) for b, r in enumerate(as_list))
    assert (as_float >= many).all() and (as_float > many).any()
    restated = tr.TCoMemRestated(s, d, t, N_NODES, 50)
    restated.update(s1.cpu().numpy(), d1.cpu().numpy(), t1.cpu().numpy())
    assert_state(model, restated)
    assert tr.rel_err(after.cpu().numpy(), restated.scores64(s1.cpu().numpy(), d1.cpu().numpy(), 'float32')) < BAR
