"""-m gpu: vss_search_batch_filtered_groups_auto — one request whose every group is answered by the cheaper of the graph walk
(vss_search_batch_filtered_groups) and the exact scan of the admitted rows (vss_search_exact_batch_filtered_groups); the rule
is csrc/filter_route.h, the kernels csrc/filter_route_kernels.h ("Routing").

Contract: route[q] is the rule applied to NumPy's count of the live rows q's group admits; a query of route 1 gets, cell for
cell (row ids, f32 distance bits, count), what the exact call gives it, a query of route 0 what the graph call gives it under
the same k and ef.  The two existing calls are the yardsticks; their own answers are held to a CPU brute force elsewhere
(tests/test_gpu_exact_filtered.py, tests/test_gpu_filter_groups.py).

The default constant routes every group of an index of a few thousand rows exact (its crossover at limit 64 is
sqrt(62 500 * L) rows, more than L below L = 62 500), so the mixed cases name a route_c that puts the boundary inside the table:
with L = 6000 and limit 64 the rule is len^2 <= route_c * 6000, and route_c = 1500 makes len = 3000 the last exact size.
A named route_c is the bare rule.  The engine's defaults (route_c = 0) add the minimum walk: where some exact-routed group
admits a row and the graph-routed groups together hold less than 2^24 (query, admitted row) pairs, they are scanned too.
"""
import numpy as np
import pytest

import gpu_common as gc
from test_gpu_exact_filtered import ONES, _admits, _bitmap, _words, assert_same, keys_against_slot_order

pytestmark = pytest.mark.gpu

U64_MAX = 2 ** 64 - 1
DEFAULT_C = 62_500
MIN_WALK = 1 << 24


def rule_exact(length, live, limit, c):
    if length == 0 or live == 0:
        return True
    return int(length) * int(length) * 64 <= int(c) * int(limit) * int(live)


def boundary(live, limit, c):
    """the largest len the rule sends exact"""
    lo, hi = 0, 2 ** 32 - 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if mid * mid * 64 <= c * limit * live else (lo, mid - 1)
    return lo


def build(dim, metric, X, keys, capacity=None, M=16, M0=32, efc=64):
    gpu = gc.gpu_index(dim, metric, M, M0, efc)
    gpu.reserve(capacity or len(X))
    gpu.set_build_params(32768, 4)
    gpu.add(keys, X)
    return gpu


def with_padding_set(bitmap, n_bits):
    b = bitmap.copy()
    if n_bits % 64:
        b[-1] |= ONES << np.uint64(n_bits % 64)
    return b


def expected_route(keys, live, bitmaps, n_bits, group_of, nq, limit, c):
    """(route per query, admitted live rows per group in use) from NumPy counts of live & admitted"""
    groups = np.zeros(nq, dtype=np.uint32) if group_of is None else np.asarray(group_of)
    admitted = {int(g): int(np.sum(live & _admits(bitmaps[g], n_bits, keys))) for g in np.unique(groups)}
    n_live = int(live.sum())
    route = np.array([1 if rule_exact(admitted[int(g)], n_live, limit, c or DEFAULT_C) else 0 for g in groups], dtype=np.uint8)
    if not c:  # the engine's defaults: a walk that saves a call that scans anyway less than MIN_WALK distances is not launched
        scans = any(admitted[int(g)] for g in groups[route == 1])
        if scans and (route == 0).any() and sum(admitted[int(g)] for g in groups[route == 0]) < MIN_WALK:
            route[:] = 1
    return route, admitted


def check_routed(gpu, Q, k, ef, bitmaps, n_bits, group_of, route_c, keys, live, what, ef_search=64, walk_all=True):
    """one routed call held to the rule, to the two existing calls, and to its own counters; returns its route.
    walk_all=False: the graph call answers only the graph-routed queries (where walking the tiny groups too would take seconds)"""
    nq = len(Q)
    limit = max(k, ef or ef_search)
    want_route, admitted = expected_route(keys, live, bitmaps, n_bits, group_of, nq, limit, route_c)
    ids, dist, cnt, route = gpu.search_batch_filtered_groups_auto(Q, k, ef, bitmaps, n_bits, group_of, route_c)
    listed, stats, shape, routed = gpu.last_exact_filtered(), gpu.last_search_stats(), gpu.last_search_shape(), gpu.last_filter_route()
    assert np.array_equal(route, want_route), what + ": routes"
    groups = np.zeros(nq, dtype=np.uint32) if group_of is None else np.asarray(group_of)
    ex, gr = route == 1, route == 0
    if ex.any():
        want = gpu.search_exact_batch_filtered_groups(Q, k, bitmaps, n_bits, group_of)
        assert_same(tuple(a[ex] for a in (ids, dist, cnt)), tuple(a[ex] for a in want), what + ": exact-routed queries")
    if gr.any():
        if group_of is None:
            want = gpu.search_batch_filtered(Q, k, ef, bitmaps[0], n_bits)
        elif walk_all:
            want = gpu.search_batch_filtered_groups(Q, k, ef, bitmaps, n_bits, group_of)
        else:
            want = [np.empty((nq,) + a.shape[1:], a.dtype) for a in (ids, dist, cnt)]
            for a, b in zip(want, gpu.search_batch_filtered_groups(Q[gr], k, ef, bitmaps, n_bits, group_of[gr])):
                a[gr] = b
        assert_same(tuple(a[gr] for a in (ids, dist, cnt)), tuple(a[gr] for a in want), what + ": graph-routed queries")
    exact_groups, graph_groups = np.unique(groups[ex]), np.unique(groups[gr])
    assert listed[0] == sum(admitted[int(g)] for g in exact_groups), what + ": rows listed"
    assert listed[1] == sum(admitted[int(g)] for g in groups[ex]), what + ": distances"
    assert list(routed) == [gr.sum(), ex.sum(), len(graph_groups), len(exact_groups), int(live.sum()), route_c or DEFAULT_C, limit, 0], what
    if not gr.any():
        assert not np.any(stats) and not np.any(shape), what + ": no walk, yet search counters"
    else:
        assert stats[2] == gr.sum(), what + ": the walk saw other queries than the graph-routed ones"
    return route


# ------------------------------------------------------------------------------------------------- 1. the mixed chunk
@pytest.mark.parametrize("dim", [3, 100, 768])  # dword rows, float4 rows, wide rows
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_mixed_chunk(metric, dim):
    n, nq, route_c = 6000, 37, 1500
    X, Q = gc.make_data(n, dim, metric, 1500 + dim, nq=nq)
    keys = keys_against_slot_order(n, 9000)  # row id != slot; row ids 3001 .. 9000
    n_bits = 9001  # no multiple of 64
    live = np.ones(n, dtype=bool)
    rng = np.random.default_rng(15)
    b = boundary(n, 64, route_c)
    assert b == 3000 and b * b * 64 == route_c * 64 * n  # exactly ON the boundary
    table = [np.full(_words(n_bits), ONES, dtype=np.uint64),          # 0: all ones
             _bitmap(n_bits, np.arange(0, n_bits, 3)),                # 1: every third row id
             _bitmap(n_bits, keys[rng.random(n) < 1 / 16]),           # 2: a random 1/16
             _bitmap(n_bits, [int(keys[4321])]),                      # 3: exactly one row
             np.zeros(_words(n_bits), dtype=np.uint64),               # 4: all zeros
             np.full(_words(n_bits), ONES, dtype=np.uint64),          # 5: nobody asks for it
             _bitmap(n_bits, rng.choice(keys, b, replace=False)),     # 6: on the boundary: exact
             _bitmap(n_bits, rng.choice(keys, b + 1, replace=False))]  # 7: one row above: graph
    bitmaps = np.stack([with_padding_set(t, n_bits) for t in table])  # set padding bits admit nothing
    group_of = np.array([0] * 6 + [1] * 9 + [2] * 5 + [3] * 3 + [4] * 2 + [6] * 6 + [7] * 6, dtype=np.uint32)
    assert len(group_of) == nq
    group_of = group_of[rng.permutation(nq)]
    gpu = build(dim, metric, X, keys)
    for k in (10, 1):
        route = check_routed(gpu, Q, k, 64, bitmaps, n_bits, group_of, route_c, keys, live, "%s dim %d k %d" % (metric, dim, k))
        assert set(route) == {0, 1}  # both routes in one call
        assert np.all(route[group_of == 6] == 1) and np.all(route[group_of == 7] == 0) and np.all(route[group_of == 0] == 0)


# ------------------------------------------------------------------------------------------------- a shared index
class Base:
    def __init__(self):
        self.metric, self.n, self.dim = "l2sq", 6000, 32
        self.X, self.Q = gc.make_data(self.n, self.dim, self.metric, 1503, nq=300)
        self.keys = keys_against_slot_order(self.n, 9000)
        self.live = np.ones(self.n, dtype=bool)
        self.n_bits = 9001
        rng = np.random.default_rng(1504)
        self.bitmaps = np.stack([np.full(_words(self.n_bits), ONES, dtype=np.uint64),        # 0: 6000 rows
                                 _bitmap(self.n_bits, np.arange(0, self.n_bits, 3)),         # 1: 2000
                                 _bitmap(self.n_bits, self.keys[rng.random(self.n) < 1 / 16]),  # 2: ~375
                                 _bitmap(self.n_bits, self.keys[:70]),                       # 3: 70
                                 _bitmap(self.n_bits, [int(self.keys[99])]),                 # 4: 1
                                 np.zeros(_words(self.n_bits), dtype=np.uint64),             # 5: 0
                                 _bitmap(self.n_bits, rng.choice(self.keys, 3500, replace=False))])  # 6: 3500
        self.gpu = build(self.dim, self.metric, self.X, self.keys)

    def check(self, Q, k, ef, group_of, route_c, what, bitmaps=None):
        return check_routed(self.gpu, Q, k, ef, self.bitmaps if bitmaps is None else bitmaps, self.n_bits, group_of, route_c,
                            self.keys, self.live, what)


@pytest.fixture(scope="module")
def base():
    return Base()


# ------------------------------------------------------------------------------------------------- 2. forced routes
def test_forced_routes(base):
    Q = base.Q[:35]
    group_of = (np.arange(35) % 7).astype(np.uint32)
    everything = base.check(Q, 10, 64, group_of, U64_MAX, "route_c = 2^64 - 1")
    assert np.all(everything == 1)
    tiny = base.check(Q, 10, 64, group_of, 1, "route_c = 1")  # len^2 <= 6000: 70 rows stay exact, 375 do not
    assert np.all(tiny[np.isin(group_of, [3, 4, 5])] == 1) and np.all(tiny[np.isin(group_of, [0, 1, 2, 6])] == 0)
    default = base.check(Q, 10, 64, group_of, 0, "the default constant")
    assert np.all(default == 1)  # sqrt(62 500 * 6000) > 6000
    # ef == 0 is the index's ef_search (64): the same routes as ef = 64, and the graph call's answers under ef = 0
    assert np.array_equal(base.check(Q, 10, 0, group_of, 1500, "ef 0"), base.check(Q, 10, 64, group_of, 1500, "ef 64"))


# ------------------------------------------------------------------------------------------------- 3. tombstones
def test_tombstones_move_the_boundary():
    """group 1 admits 2600 rows.  Whole index (L = 5000, route_c = 1300: len <= 2549): graph.  After removing 900 rows, 500 of
    them its own (L = 4100, len = 2100 <= 2308): exact — len and L both changed.  The same after compaction."""
    n, dim, route_c = 5000, 24, 1300
    X, Q = gc.make_data(n, dim, "l2sq", 1505, nq=20)
    keys = keys_against_slot_order(n, 9000)
    n_bits = 9001
    rng = np.random.default_rng(1506)
    mine = rng.choice(n, 2600, replace=False)
    bitmaps = np.stack([np.full(_words(n_bits), ONES, dtype=np.uint64), _bitmap(n_bits, keys[mine]), _bitmap(n_bits, keys[:40])])
    group_of = (np.arange(20) % 3).astype(np.uint32)
    live = np.ones(n, dtype=bool)
    gpu = build(dim, "l2sq", X, keys)
    route = check_routed(gpu, Q, 10, 64, bitmaps, n_bits, group_of, route_c, keys, live, "whole")
    assert np.all(route[group_of == 1] == 0) and np.all(route[group_of == 0] == 0) and np.all(route[group_of == 2] == 1)
    others = np.setdiff1d(np.arange(40, n), mine)
    gone = np.concatenate([mine[mine >= 40][:500], others[:400]])
    assert gpu.remove(keys[gone]) == 900
    live[gone] = False
    route = check_routed(gpu, Q, 10, 64, bitmaps, n_bits, group_of, route_c, keys, live, "900 removed")
    assert np.all(route[group_of == 1] == 1) and np.all(route[group_of == 0] == 0)
    assert gpu.last_filter_route()[4] == 4100
    gpu.compact()
    # (slots have moved: the existing calls on the compacted index are the yardstick, the counts are by row id)
    route = check_routed(gpu, Q, 10, 64, bitmaps, n_bits, group_of, route_c, keys, live, "compacted")
    assert np.all(route[group_of == 1] == 1) and np.all(route[group_of == 0] == 0)


# ------------------------------------------------------------------------------------------------- 4. batch sizes
def test_batch_sizes(base):
    rng = np.random.default_rng(1507)
    group_of = np.array([0] * 25 + [6] * 15 + [1] * 100 + [2] * 100 + [3] * 40 + [4] * 10 + [5] * 10, dtype=np.uint32)
    group_of = group_of[rng.permutation(300)]
    route = base.check(base.Q, 10, 64, group_of, 1500, "300 queries, 40 of them walked")
    assert (route == 0).sum() == 40
    for g in (0, 3):  # one query, either route
        route = base.check(base.Q[:1], 10, 64, np.array([g], dtype=np.uint32), 1500, "one query of group %d" % g)
        assert route[0] == (0 if g == 0 else 1)
    # every query walked: no list is built
    walked = np.where(np.arange(50) % 2 == 0, 0, 6).astype(np.uint32)
    assert np.all(base.check(base.Q[:50], 10, 64, walked, 1500, "all graph") == 0)
    base.gpu.search_batch_filtered_groups_auto(base.Q[:50], 10, 64, base.bitmaps, base.n_bits, walked, 1500)
    assert base.gpu.last_exact_filtered()[0] == 0 and base.gpu.last_exact_filtered()[1] == 0
    # every query scanned: no walk
    scanned = (1 + np.arange(50) % 5).astype(np.uint32)
    assert np.all(base.check(base.Q[:50], 10, 64, scanned, 1500, "all exact") == 1)
    base.gpu.search_batch_filtered_groups_auto(base.Q[:50], 10, 64, base.bitmaps, base.n_bits, scanned, 1500)
    assert not np.any(base.gpu.last_search_stats()) and not np.any(base.gpu.last_search_shape())
    assert not np.any(base.gpu.last_search_prescore()[:3])


def test_minimum_walk_under_the_default_constant():
    """70 000 rows: under the default constant the rule walks groups of more than sqrt(62 500 * 70 000) = 66 143 rows — the
    all-ones group.  Beside a scan its queries are walked only from ceil(2^24 / 70 000) = 240 of them on; alone they always are."""
    n, dim = 70_000, 16
    rng = np.random.default_rng(1508)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((300, dim)).astype(np.float32)
    keys = keys_against_slot_order(n)
    n_bits = 1_000_001
    live = np.ones(n, dtype=bool)
    bitmaps = np.stack([np.full(_words(n_bits), ONES, dtype=np.uint64), _bitmap(n_bits, keys[:500]),
                        np.zeros(_words(n_bits), dtype=np.uint64)])
    gpu = build(dim, "l2sq", X, keys, M=4, M0=8, efc=16)  # (a cheap graph: the walk is held to the graph call on the same index)
    assert boundary(n, 64, DEFAULT_C) == 66_143 and 239 * n < MIN_WALK <= 240 * n

    def routes(n_ones, n_small, n_none, route_c=0):
        group_of = np.array([0] * n_ones + [1] * n_small + [2] * n_none, dtype=np.uint32)
        group_of = group_of[rng.permutation(len(group_of))]
        route = check_routed(gpu, Q[:len(group_of)], 10, 64, bitmaps, n_bits, group_of, route_c, keys, live,
                             "%d + %d + %d queries" % (n_ones, n_small, n_none), walk_all=False)
        return route[group_of == 0]
    assert np.all(routes(239, 20, 0) == 1)  # folded into the scan ...
    assert np.all(routes(240, 20, 0) == 0)  # ... walked
    assert np.all(routes(30, 0, 0) == 0)    # nothing to scan: walked
    assert np.all(routes(30, 0, 5) == 0)    # a group that admits nothing builds no list: still nothing to scan
    assert np.all(routes(30, 20, 0, DEFAULT_C) == 0)  # a named constant is the bare rule


# ------------------------------------------------------------------------------------------------- 5. no group numbers
def test_group_of_none(base):
    Q = base.Q[:21]
    selective = base.bitmaps[[2, 0]]    # bitmap 0 = the random 1/16: the exact call's answer
    unselective = base.bitmaps[[0, 2]]  # bitmap 0 = all ones: vss_search_batch_filtered's answer
    assert np.all(base.check(Q, 10, 64, None, 1500, "selective bitmap", selective) == 1)
    assert np.all(base.check(Q, 10, 64, None, 1500, "unselective bitmap", unselective) == 0)


# ------------------------------------------------------------------------------------------------- 6. the device form
def _device_call(base, Q, k, ef, group_of, route_c, with_dist=True, with_route=True):
    import torch
    nq = len(Q)
    d_Q = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    d_tables = torch.from_numpy(base.bitmaps.view(np.int64)).cuda()
    d_groups = torch.from_numpy(group_of.view(np.int32)).cuda() if group_of is not None else None
    d_keys = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    d_dist = torch.zeros((nq, k), dtype=torch.float32, device="cuda") if with_dist else None
    d_cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
    d_route = torch.full((nq,), 9, dtype=torch.uint8, device="cuda") if with_route else None
    torch.cuda.synchronize()
    base.gpu.search_batch_filtered_groups_auto_device(d_Q.data_ptr(), nq, k, ef, d_tables.data_ptr(), len(base.bitmaps), base.n_bits,
                                                      d_groups.data_ptr() if d_groups is not None else None, d_keys.data_ptr(),
                                                      d_dist.data_ptr() if with_dist else None, d_cnt.data_ptr(),
                                                      d_route.data_ptr() if with_route else None, route_c)
    return (d_keys.cpu().numpy(), d_dist.cpu().numpy() if with_dist else None, d_cnt.cpu().numpy().astype(np.uint32),
            d_route.cpu().numpy() if with_route else None)


def test_device_form(base):
    Q = base.Q[:35]
    group_of = (np.arange(35) % 7).astype(np.uint32)
    want = base.gpu.search_batch_filtered_groups_auto(Q, 10, 64, base.bitmaps, base.n_bits, group_of, 1500)
    assert set(want[3]) == {0, 1}
    got = _device_call(base, Q, 10, 64, group_of, 1500)
    assert_same(got[:3], want[:3], "device form")
    assert np.array_equal(got[3], want[3])
    # no distances, no routes asked for
    bare = _device_call(base, Q, 10, 64, group_of, 1500, with_dist=False, with_route=False)
    assert np.array_equal(bare[0], want[0]) and np.array_equal(bare[2], want[2]) and bare[1] is None and bare[3] is None
    # no group numbers: bitmap 0 (all ones) for everybody
    none = base.gpu.search_batch_filtered_groups_auto(Q, 10, 64, base.bitmaps, base.n_bits, None, 1500)
    got = _device_call(base, Q, 10, 64, None, 1500)
    assert_same(got[:3], none[:3], "device form, no group numbers")
    assert np.all(got[3] == 0)
    # queries of groups the table does not hold: route 255, empty answers, the others as before
    bad = group_of.copy()
    bad[[5, 11]] = [7, 4_000_000_000]
    with pytest.raises(gc.pkg().VssError, match="query 5 names group 7"):
        base.gpu.search_batch_filtered_groups_auto(Q, 10, 64, base.bitmaps, base.n_bits, bad, 1500)
    got = _device_call(base, Q, 10, 64, bad, 1500)
    unknown = np.isin(np.arange(35), [5, 11])
    assert np.all(got[3][unknown] == 255) and np.array_equal(got[3][~unknown], want[3][~unknown])
    assert np.all(got[2][unknown] == 0) and np.all(got[0][unknown] == -1) and np.all(np.isposinf(got[1][unknown]))
    assert_same(tuple(a[~unknown] for a in got[:3]), tuple(a[~unknown] for a in want[:3]), "the other queries of that call")
    # ... also where nothing is exact-routed, and where nothing is walked
    for route_c, groups in ((1500, [0, 6]), (U64_MAX, [0, 1])):
        some = np.array(groups, dtype=np.uint32)[np.arange(35) % 2]
        ok = base.gpu.search_batch_filtered_groups_auto(Q, 10, 64, base.bitmaps, base.n_bits, some, route_c)
        some[[5, 11]] = [7, 4_000_000_000]
        got = _device_call(base, Q, 10, 64, some, route_c)
        assert np.all(got[3][unknown] == 255) and np.all(got[2][unknown] == 0) and np.all(got[0][unknown] == -1)
        assert np.all(np.isposinf(got[1][unknown]))
        assert_same(tuple(a[~unknown] for a in got[:3]), tuple(a[~unknown] for a in ok[:3]), "route_c %d" % route_c)


# ------------------------------------------------------------------------------------------------- 7. limits
def test_wide_limits(base):
    """k = ef = 600: the walk keeps its lists in LDS, the scan has k > 512; limit 600 and route_c = 160 put the boundary at 3000"""
    assert boundary(base.n, 600, 160) == 3000
    Q = base.Q[:14]
    group_of = (np.arange(14) % 7).astype(np.uint32)
    route = base.check(Q, 600, 600, group_of, 160, "k 600")
    assert set(route) == {0, 1}
    assert np.all(route[np.isin(group_of, [0, 6])] == 0) and np.all(route[np.isin(group_of, [1, 2, 3, 4, 5])] == 1)


def test_k_above_the_exact_limit(base):
    """k = 5000 is refused only where something is exact-routed"""
    Q = base.Q[:4]
    walked = np.zeros(4, dtype=np.uint32)  # all ones: 6000^2 * 64 > 1 * 5000 * 6000
    ids, dist, cnt, route = base.gpu.search_batch_filtered_groups_auto(Q, 5000, 64, base.bitmaps, base.n_bits, walked, 1)
    assert np.all(route == 0)
    assert_same((ids, dist, cnt), base.gpu.search_batch_filtered_groups(Q, 5000, 64, base.bitmaps, base.n_bits, walked), "k 5000")
    with pytest.raises(gc.pkg().VssError, match="k <= 4088"):
        base.gpu.search_batch_filtered_groups_auto(Q, 5000, 64, base.bitmaps, base.n_bits, np.array([0, 4, 0, 0], dtype=np.uint32), 1)


# ------------------------------------------------------------------------------------------------- 8. empty calls
def test_empty_index_and_empty_calls(base):
    Q = base.Q[:7]
    group_of = (np.arange(7) % 7).astype(np.uint32)
    empty = gc.gpu_index(base.dim, base.metric)
    ids, dist, cnt, route = empty.search_batch_filtered_groups_auto(Q, 10, 64, base.bitmaps, base.n_bits, group_of, 1)
    assert np.all(route == 1) and np.all(cnt == 0) and np.all(ids == -1) and np.all(np.isposinf(dist))
    assert list(empty.last_filter_route()[:5]) == [0, 7, 0, 7, 0]
    g, lib = base.gpu, base.gpu.lib
    keys, d, c, r = np.zeros((7, 10), np.int64), np.zeros((7, 10), np.float32), np.zeros(7, np.uint32), np.zeros(7, np.uint8)

    def call(nq, k, table, n_groups):
        return lib.vss_search_batch_filtered_groups_auto(g.h, Q.ctypes.data, nq, k, 64, table, n_groups, base.n_bits,
                                                         group_of.ctypes.data, 0, keys.ctypes.data, d.ctypes.data, c.ctypes.data,
                                                         r.ctypes.data)
    assert call(0, 10, None, 0) == 0 and call(7, 0, None, 0) == 0
    assert call(7, 10, None, 7) != 0 and b"bitmaps" in lib.vss_last_error(g.h)
    assert call(7, 10, base.bitmaps.ctypes.data, 0) != 0 and b"at least one group" in lib.vss_last_error(g.h)
    ids, dist, cnt, route = g.search_batch_filtered_groups_auto(Q[:0], 10, 64, base.bitmaps, base.n_bits, group_of[:0])
    assert ids.shape == (0, 10) and route.shape == (0,)
