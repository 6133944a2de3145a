"""-m gpu: vss_search_exact_batch_filtered_groups — exact top-k under per-query predicates that scores only the admitted rows
(csrc/exact_filtered_kernels.h).

Contract, for finite inputs: query q gets the min(k, admitted live rows) rows its group's bitmap admits with the smallest
(distance, slot) pairs, in that order — row ids, f32 distance bits and counts, every cell.  The yardstick is
gpu_common.ExactReference, given ONLY the admitted live rows of a group with their keys and slots: the CPU brute force in
wave-order f32, which reads nothing from the index under test.
"""
import threading

import numpy as np
import pytest

import gpu_common as gc

pytestmark = pytest.mark.gpu

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
CHUNK, MS_QT = 32768, 8


def _words(n_bits):
    return (n_bits + 63) // 64


def _bitmap(n_bits, admitted_keys):
    """bits of `admitted_keys` (all < n_bits) set, every other bit — the padding included — clear"""
    b = np.zeros(_words(n_bits), dtype=np.uint64)
    k = np.asarray(admitted_keys, dtype=np.int64)
    np.bitwise_or.at(b, k >> 6, np.uint64(1) << (k & 63).astype(np.uint64))
    return b


def _admits(bitmap, n_bits, keys):
    keys = np.asarray(keys, dtype=np.int64)
    ok = (keys >= 0) & (keys < n_bits)
    safe = np.where(ok, keys, 0)
    return ok & (((bitmap[safe >> 6] >> (safe & 63).astype(np.uint64)) & np.uint64(1)) == 1)


def keys_against_slot_order(n, top=1_000_000):
    """keys that DESCEND with the slot: an answer ordered by (distance, key) instead of (distance, slot) is caught"""
    return top - np.arange(n, dtype=np.int64)


def build(dim, metric, X, keys, M=8, M0=16, efc=16, capacity=None):
    """A cheap graph (only the exact path is under test); slot of row i = i, key of slot s = keys[s]."""
    gpu = gc.gpu_index(dim, metric, M, M0, efc)
    gpu.reserve(capacity or len(X))
    gpu.set_build_params(32768, 4)
    gpu.add(keys, X)
    return gpu


class Yardstick:
    """One ExactReference per group in use, over that group's admitted live rows only; computed once, shared by every k."""

    def __init__(self, metric, X, keys, live, bitmaps, n_bits, group_of, Q, kmax, slots_known=True):
        self.group_of = np.zeros(len(Q), dtype=np.uint32) if group_of is None else np.asarray(group_of)
        self.admitted, self.refs = {}, {}
        for g in np.unique(self.group_of):
            rows = np.nonzero(live & _admits(bitmaps[g], n_bits, keys))[0]
            qs = np.nonzero(self.group_of == g)[0]
            self.admitted[int(g)] = len(rows)
            self.refs[int(g)] = (qs, gc.ExactReference(metric, X[rows], keys[rows], rows if slots_known else None, Q[qs], kmax))

    def check(self, got, k, what):
        for g, (qs, ref) in self.refs.items():
            gc.assert_exact_answer(tuple(a[qs] for a in got), ref.top(k), "%s, group %d, k %d" % (what, g, k))


def assert_same(a, b, what):
    assert np.array_equal(a[0], b[0]), what + ": row ids"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), what + ": distance bits"
    assert np.array_equal(a[2], b[2]), what + ": counts"


# ------------------------------------------------------------------------------------------------- 1. metrics and row widths
@pytest.mark.parametrize("dim", [3, 100, 768])  # a one-lane group, a row padded to a float4 multiple, a wide row
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_metrics_and_row_widths(metric, dim):
    n, nq = 3000, 37
    X, Q = gc.make_data(n, dim, metric, 1400 + dim, nq=nq)
    keys = keys_against_slot_order(n, 5000)  # row id != slot
    n_bits = 5001
    rng = np.random.default_rng(14)
    one_row = int(keys[1234])
    bitmaps = np.stack([np.full(_words(n_bits), ONES, dtype=np.uint64),           # 0: all ones
                        np.zeros(_words(n_bits), dtype=np.uint64),                # 1: all zeros
                        _bitmap(n_bits, np.arange(0, n_bits, 3)),                 # 2: every third row id
                        _bitmap(n_bits, [one_row]),                               # 3: exactly one row
                        _bitmap(n_bits, keys[rng.random(n) < 1 / 16]),            # 4: a random 1/16
                        np.full(_words(n_bits), ONES, dtype=np.uint64)])          # 5: nobody asks for it
    # groups get MS_QT + 1, 1, MS_QT, MS_QT - 1, MS_QT + 4 (two tiles) and 0 queries, interleaved
    group_of = np.array([0] * (MS_QT + 1) + [1] + [2] * MS_QT + [3] * (MS_QT - 1) + [4] * (MS_QT + 4), dtype=np.uint32)
    assert len(group_of) == nq
    group_of = group_of[rng.permutation(nq)]
    live = np.ones(n, dtype=bool)
    ref = Yardstick(metric, X, keys, live, bitmaps, n_bits, group_of, Q, 10)
    gpu = build(dim, metric, X, keys)
    for k in (10, 1):
        got = gpu.search_exact_batch_filtered_groups(Q, k, bitmaps, n_bits, group_of)
        ref.check(got, k, "%s dim %d" % (metric, dim))
        assert gpu.last_exact_fallbacks() == 0
        one, none = group_of == 3, group_of == 1
        assert np.all(got[2][one] == 1) and np.all(got[0][one][:, 0] == one_row)
        assert np.all(got[0][one][:, 1:] == -1) and np.all(np.isposinf(got[1][one][:, 1:]))
        assert np.all(got[2][none] == 0) and np.all(got[0][none] == -1) and np.all(np.isposinf(got[1][none]))
    stats = gpu.last_exact_filtered()
    assert stats[0] == sum(ref.admitted.values())  # group 5 has no query: not listed
    assert stats[1] == sum(ref.admitted[int(g)] for g in group_of) and stats[2] == 1 and stats[3] > 0


# ------------------------------------------------------------------------------------------------- 2. chunk edges
def test_chunk_edges():
    """lists of exactly one score chunk, one chunk plus a row, and three chunks; then without the rows either side of the first
    chunk boundary of every list"""
    n, dim = 70_000, 16
    rng = np.random.default_rng(1402)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((9, dim)).astype(np.float32)
    keys = keys_against_slot_order(n)
    n_bits = 1_000_001
    first = [100, 5, 0]
    length = [CHUNK, CHUNK + 1, n]
    bitmaps = np.stack([_bitmap(n_bits, keys[f:f + c]) for f, c in zip(first, length)])
    group_of = np.array([0, 1, 2] * 3, dtype=np.uint32)
    gpu = build(dim, "l2sq", X, keys, M=4, M0=8)
    live = np.ones(n, dtype=bool)
    for stage in ("whole", "without the boundary rows"):
        ref = Yardstick("l2sq", X, keys, live, bitmaps, n_bits, group_of, Q, 300)
        if stage == "whole":
            assert [ref.admitted[g] for g in range(3)] == length
        for k in (10, 300):
            got = gpu.search_exact_batch_filtered_groups(Q, k, bitmaps, n_bits, group_of)
            ref.check(got, k, "chunk edges, " + stage)
        gone = sorted({f + p for f, c in zip(first, length) for p in (CHUNK - 1, CHUNK) if p < c})
        if stage == "whole":
            assert gpu.remove(keys[gone]) == len(gone) == 5
            live[gone] = False


# ------------------------------------------------------------------------------------------------- a shared small index
class Base:
    def __init__(self):
        self.metric, self.n, self.dim = "l2sq", 3000, 32
        self.X, self.Q = gc.make_data(self.n, self.dim, self.metric, 1403, nq=24)
        self.keys = keys_against_slot_order(self.n, 5000)  # row ids 2001 .. 5000
        self.live = np.ones(self.n, dtype=bool)
        self.gpu = build(self.dim, self.metric, self.X, self.keys, M=16, M0=32, efc=64)

    def yardstick(self, bitmaps, n_bits, group_of, kmax=10, Q=None):
        return Yardstick(self.metric, self.X, self.keys, self.live, bitmaps, n_bits, group_of, self.Q if Q is None else Q, kmax)


@pytest.fixture(scope="module")
def base():
    return Base()


# ------------------------------------------------------------------------------------------------- 3. n_bits
@pytest.mark.parametrize("n_bits", [4000, 4003, 10_000])
def test_n_bits(base, n_bits):
    """4000: smaller than the largest row id — the rows beyond are rejected; 4003: no multiple of 64, the padding bits of group 0
    SET and a group of all ones behind it; 10000: larger than every row id"""
    third = _bitmap(n_bits, np.arange(0, n_bits, 3))
    third[-1] |= ONES << np.uint64(n_bits % 64) if n_bits % 64 else np.uint64(0)  # padding bits set
    bitmaps = np.stack([third, np.full(_words(n_bits), ONES, dtype=np.uint64)])
    group_of = (np.arange(len(base.Q)) % 2).astype(np.uint32)
    ref = base.yardstick(bitmaps, n_bits, group_of)
    assert ref.admitted[1] == int(np.sum(base.keys < n_bits)) and 0 < ref.admitted[0] < ref.admitted[1]
    got = base.gpu.search_exact_batch_filtered_groups(base.Q, 10, bitmaps, n_bits, group_of)
    ref.check(got, 10, "n_bits %d" % n_bits)
    assert np.all(got[0][got[0] >= 0] < n_bits)


# ------------------------------------------------------------------------------------------------- 4. ties and re-used slots
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_identical_rows_come_back_in_slot_order(metric):
    rng = np.random.default_rng(1404)
    n, dim = 4000, 16
    X = rng.standard_normal((n, dim)).astype(np.float32)
    twins = 7 + 70 * np.arange(50)
    X[twins] = X[twins[0]]
    Q = np.concatenate([X[twins[:1]], rng.standard_normal((3, dim)).astype(np.float32)])
    keys = keys_against_slot_order(n, 5000)
    n_bits = 5001
    # group 0 admits every second copy and a tenth of the rest, group 1 everything
    some = np.concatenate([keys[twins[::2]], keys[rng.random(n) < 0.1]])
    bitmaps = np.stack([_bitmap(n_bits, some), np.full(_words(n_bits), ONES, dtype=np.uint64)])
    group_of = np.array([0, 1, 0, 1], dtype=np.uint32)
    ref = Yardstick(metric, X, keys, np.ones(n, dtype=bool), bitmaps, n_bits, group_of, Q, 45)
    gpu = build(dim, metric, X, keys)
    for k in (10, 45):
        got = gpu.search_exact_batch_filtered_groups(Q, k, bitmaps, n_bits, group_of)
        ref.check(got, k, "twins " + metric)
    assert np.array_equal(got[0][0][:25], keys[twins[::2]])  # the query AT the copies: its group's copies, by slot


def test_reused_slots_stay_exact():
    """rows removed, others added into their slots: the lists name the new rows under their new row ids (tie-free data;
    the slots are the engine's business, so the reference gets none)"""
    rng = np.random.default_rng(1405)
    n, dim = 3000, 24
    X = rng.standard_normal((n + 400, dim)).astype(np.float32)
    Q = rng.standard_normal((12, dim)).astype(np.float32)
    keys = np.concatenate([keys_against_slot_order(n, 5000), 6000 + np.arange(400, dtype=np.int64)])
    gpu = build(dim, "l2sq", X[:n], keys[:n], capacity=n + 400)
    gone = rng.choice(n, 400, replace=False)
    assert gpu.remove(keys[gone]) == 400
    gpu.add(keys[n:], X[n:])
    assert n <= gpu.nodes() < n + 400  # new rows took over freed slots (as many as the free ring still names)
    live = np.ones(n + 400, dtype=bool)
    live[gone] = False
    n_bits = 6400
    bitmaps = np.stack([np.full(_words(n_bits), ONES, dtype=np.uint64), _bitmap(n_bits, np.arange(1, n_bits, 2)),
                        _bitmap(n_bits, keys[gone])])  # 2: only removed rows — admits nothing
    group_of = (np.arange(len(Q)) % 3).astype(np.uint32)
    ref = Yardstick("l2sq", X, keys, live, bitmaps, n_bits, group_of, Q, 10, slots_known=False)
    assert ref.admitted[2] == 0
    got = gpu.search_exact_batch_filtered_groups(Q, 10, bitmaps, n_bits, group_of)
    ref.check(got, 10, "re-used slots")


# ------------------------------------------------------------------------------------------------- 5. the all-ones predicate
def test_all_ones_equals_the_exact_search(base):
    n_bits = 5001
    bitmaps = np.full((1, _words(n_bits)), ONES, dtype=np.uint64)
    for k in (1, 10, 100):
        want = base.gpu.search_batch(base.Q, k, exact=True)
        got = base.gpu.search_exact_batch_filtered_groups(base.Q, k, bitmaps, n_bits, None)
        assert_same(got, want, "all ones, k %d" % k)
        zeros = base.gpu.search_exact_batch_filtered_groups(base.Q, k, bitmaps, n_bits, np.zeros(len(base.Q), dtype=np.uint32))
        assert_same(zeros, got, "group_of None vs all zero, k %d" % k)


# ------------------------------------------------------------------------------------------------- 6. device form and errors
def _tables(base):
    n_bits = 5001
    bitmaps = np.stack([np.full(_words(n_bits), ONES, dtype=np.uint64), _bitmap(n_bits, np.arange(0, n_bits, 3)),
                        _bitmap(n_bits, np.arange(0, n_bits, 16))])
    return bitmaps, n_bits, (np.arange(len(base.Q)) % 3).astype(np.uint32)


def _device_call(base, k, bitmaps, n_bits, group_of):
    import torch
    nq = len(base.Q)
    d_Q = torch.from_numpy(base.Q).cuda()
    d_tables = torch.from_numpy(bitmaps.view(np.int64)).cuda()
    d_groups = torch.from_numpy(group_of.astype(np.int32)).cuda() if group_of is not None else None
    d_keys = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    d_dist = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    d_cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    base.gpu.search_exact_batch_filtered_groups_device(d_Q.data_ptr(), nq, k, d_tables.data_ptr(), len(bitmaps), n_bits,
                                                       d_groups.data_ptr() if d_groups is not None else None,
                                                       d_keys.data_ptr(), d_dist.data_ptr(), d_cnt.data_ptr())
    return d_keys.cpu().numpy(), d_dist.cpu().numpy(), d_cnt.cpu().numpy().astype(np.uint32)


def test_device_form_equals_the_host_form(base):
    bitmaps, n_bits, group_of = _tables(base)
    want = base.gpu.search_exact_batch_filtered_groups(base.Q, 10, bitmaps, n_bits, group_of)
    base.yardstick(bitmaps, n_bits, group_of).check(want, 10, "host form")
    assert_same(_device_call(base, 10, bitmaps, n_bits, group_of), want, "device form")
    assert_same(_device_call(base, 10, bitmaps, n_bits, None),
                base.gpu.search_exact_batch_filtered_groups(base.Q, 10, bitmaps, n_bits, None), "device form, no group numbers")


def test_unknown_group(base):
    bitmaps, n_bits, group_of = _tables(base)
    want = base.gpu.search_exact_batch_filtered_groups(base.Q, 10, bitmaps, n_bits, group_of)
    bad = group_of.copy()
    bad[[5, 11]] = [3, 4_000_000_000]
    with pytest.raises(gc.pkg().VssError, match="query 5 names group 3"):
        base.gpu.search_exact_batch_filtered_groups(base.Q, 10, bitmaps, n_bits, bad)
    got = _device_call(base, 10, bitmaps, n_bits, bad.view(np.int32))
    unknown = np.isin(np.arange(len(bad)), [5, 11])
    assert np.all(got[2][unknown] == 0) and np.all(got[0][unknown] == -1) and np.all(np.isposinf(got[1][unknown]))
    assert_same(tuple(a[~unknown] for a in got), tuple(a[~unknown] for a in want), "the other queries of that call")


def test_argument_errors_and_empty_calls(base):
    bitmaps, n_bits, group_of = _tables(base)
    g, lib, Q = base.gpu, base.gpu.lib, base.Q
    nq = len(Q)
    keys, dist, cnt = np.zeros((nq, 10), np.int64), np.zeros((nq, 10), np.float32), np.zeros(nq, np.uint32)

    def call(nq_, k_, table, n_groups):
        return lib.vss_search_exact_batch_filtered_groups(g.h, Q.ctypes.data, nq_, k_, table, n_groups, n_bits, group_of.ctypes.data,
                                                          keys.ctypes.data, dist.ctypes.data, cnt.ctypes.data)
    assert call(nq, 10, None, 3) != 0 and b"bitmaps" in lib.vss_last_error(g.h)
    assert call(nq, 10, bitmaps.ctypes.data, 0) != 0 and b"at least one group" in lib.vss_last_error(g.h)
    assert call(0, 10, None, 0) == 0 and call(nq, 0, None, 0) == 0
    with pytest.raises(gc.pkg().VssError, match="k <= 4088"):
        g.search_exact_batch_filtered_groups(Q, 4089, bitmaps, n_bits, group_of)
    got = g.search_exact_batch_filtered_groups(Q, 4088, bitmaps, n_bits, group_of)
    assert got[2][0] == base.n  # group 0 admits every row
    empty = gc.gpu_index(base.dim, base.metric)
    got = empty.search_exact_batch_filtered_groups(Q, 10, bitmaps, n_bits, group_of)
    assert np.all(got[2] == 0) and np.all(got[0] == -1) and np.all(np.isposinf(got[1]))


# ------------------------------------------------------------------------------------------------- 7. passes
def test_passes_under_a_small_list_budget(base, monkeypatch):
    """twelve overlapping dense groups (1500 to 2600 of the 3000 rows each) under a budget of max(1000, rows) = 3000 entries: one
    group per pass, and every group alone exceeds the 1000 asked for"""
    n_bits = 5001
    rng = np.random.default_rng(1407)
    sizes = 1500 + 100 * np.arange(12)
    bitmaps = np.stack([_bitmap(n_bits, rng.choice(base.keys, s, replace=False)) for s in sizes])
    group_of = (np.arange(len(base.Q)) % 12).astype(np.uint32)
    ref = base.yardstick(bitmaps, n_bits, group_of)
    want = base.gpu.search_exact_batch_filtered_groups(base.Q, 10, bitmaps, n_bits, group_of)
    ref.check(want, 10, "default budget")
    assert base.gpu.last_exact_filtered()[2] == 1
    monkeypatch.setenv("VSS_EXACT_FILTER_LIST_ENTRIES", "1000")
    small = build(base.dim, base.metric, base.X, base.keys)
    got = small.search_exact_batch_filtered_groups(base.Q, 10, bitmaps, n_bits, group_of)
    assert_same(got, want, "small budget")
    stats = small.last_exact_filtered()
    assert stats[2] == 12 >= 3 and stats[0] == sizes.sum()
    # the scratch: one list of at most `rows` entries, a count per (group, 512 slots), the plan's tables
    assert 0 < stats[3] <= 4 * (3000 + 12 * 6 + 3 * 12 + 8 * len(base.Q))


def test_only_the_groups_in_use_are_listed(base):
    n_bits = 5001
    rng = np.random.default_rng(1408)
    bitmaps = rng.integers(0, 1 << 63, size=(2000, _words(n_bits)), dtype=np.int64).view(np.uint64)
    named = np.array([1999, 3, 1024, 3, 77, 500, 1999, 77], dtype=np.uint32)
    ref = base.yardstick(bitmaps, n_bits, named, Q=base.Q[:8])
    got = base.gpu.search_exact_batch_filtered_groups(base.Q[:8], 10, bitmaps, n_bits, named)
    ref.check(got, 10, "5 of 2000 groups")
    stats = base.gpu.last_exact_filtered()
    assert len(ref.admitted) == 5 and stats[0] == sum(ref.admitted.values())


# ------------------------------------------------------------------------------------------------- 8. neighbours undisturbed
def test_neighbours_keep_their_answers(base):
    bitmaps, n_bits, group_of = _tables(base)
    g = base.gpu
    graph = g.search_batch_filtered_groups(base.Q, 10, 64, bitmaps, n_bits, group_of)
    exact = g.search_batch(base.Q, 10, exact=True)
    mine = g.search_exact_batch_filtered_groups(base.Q, 10, bitmaps, n_bits, group_of)
    assert_same(g.search_batch_filtered_groups(base.Q, 10, 64, bitmaps, n_bits, group_of), graph, "the graph call after")
    assert_same(g.search_batch(base.Q, 10, exact=True), exact, "the exact search after")
    assert_same(g.search_exact_batch_filtered_groups(base.Q, 10, bitmaps, n_bits, group_of), mine, "the call itself, again")

    plain = g.search_batch(base.Q, 10, 64)
    results, errors = {}, []

    def run(name, fn, want):
        try:
            for _ in range(3):
                results[name] = fn()
                assert_same(results[name], want, name)
        except Exception as e:  # noqa: BLE001
            errors.append((name, e))
    threads = [threading.Thread(target=run, args=("exact filtered %d" % i,
                                                  lambda: g.search_exact_batch_filtered_groups(base.Q, 10, bitmaps, n_bits, group_of),
                                                  mine)) for i in range(2)]
    threads.append(threading.Thread(target=run, args=("graph search", lambda: g.search_batch(base.Q, 10, 64), plain)))
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(results) == 3
