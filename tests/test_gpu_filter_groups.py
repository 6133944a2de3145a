"""-m gpu: vss_search_batch_filtered_groups — one predicate PER QUERY in one launch (the chunk of HNSW_INDEX_JOIN whose
LATERAL subquery is correlated: `WHERE items.tenant = q.tenant`).  Its contract is a restatement of the existing call:
query q gets what vss_search_batch_filtered returns for it alone under bitmap group_of[q].  Every test therefore holds the
grouped call against two yardsticks — the oracle (search_many_filtered, per query with that query's own bitmap), and the
existing vss_search_batch_filtered, called once per group on the same index — cell by cell: row ids, f32 distance bits and
counts equal to both, per-query work counters equal to the oracle's."""
import numpy as np
import pytest

import gpu_common as gc
import golden_cases

pytestmark = pytest.mark.gpu

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _words(n_bits):
    return (n_bits + 63) // 64


def _all_ones(n_bits):
    """every word all ones: the padding bits after n_bits are SET, and must admit nothing"""
    return np.full(_words(n_bits), ONES, dtype=np.uint64)


def _admits(bitmap, n_bits, keys):
    keys = np.asarray(keys, dtype=np.int64)
    ok = (keys >= 0) & (keys < n_bits)
    safe = np.where(ok, keys, 0)
    return ok & (((bitmap[safe >> 6] >> (safe & 63).astype(np.uint64)) & np.uint64(1)) == 1)


class Graph:
    """One graph in the engine and in the oracle (the engine's own stream: the oracle reads the reference's format),
    and the oracle's answers, computed once per (query, bitmap, k, ef) and shared."""

    def __init__(self, metric, n=4000, dim=32, nq=48, M=16, M0=None, efc=128, build=(256, 8), keys=None, dead=None, seed=515):
        self.metric, self.n, self.dim = metric, n, dim
        self.X, self.Q = gc.make_data(n, dim, metric, seed, nq=nq)
        self.keys = np.arange(n, dtype=np.int64) if keys is None else keys
        self.gpu = gc.gpu_index(dim, metric, M, M0, efc)
        self.gpu.reserve(n)
        self.gpu.set_build_params(*build)
        self.gpu.add(self.keys, self.X)
        self.dead = np.zeros(0, dtype=np.int64) if dead is None else dead
        if len(self.dead):
            assert self.gpu.remove(self.dead) == len(self.dead)
        self.cpu = gc.oracle_index(dim, metric, M, M0, efc)
        self.cpu.load(self.gpu.save())
        self._oracle = {}

    def oracle(self, Q, bitmaps, n_bits, group_of, k, ef):
        """per query, with that query's own bitmap"""
        nq = len(Q)
        keys = np.full((nq, k), -1, dtype=np.int64)
        dist = np.full((nq, k), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.int64)
        st = np.zeros((nq, 2), dtype=np.uint64)
        for q in range(nq):
            memo = (Q[q].tobytes(), bitmaps[group_of[q]].tobytes(), n_bits, k, ef)
            if memo not in self._oracle:
                r = self.cpu.search_many_filtered(Q[q:q + 1], k, ef, bitmaps[group_of[q]], n_bits)
                self._oracle[memo] = tuple(a[0] for a in r)
            keys[q], dist[q], cnt[q], st[q] = self._oracle[memo]
        return keys, dist, cnt, st

    def per_group(self, Q, bitmaps, n_bits, group_of, k, ef):
        """what a caller had to do before: one vss_search_batch_filtered per distinct predicate"""
        nq = len(Q)
        keys = np.full((nq, k), -1, dtype=np.int64)
        dist = np.full((nq, k), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        for g in range(len(bitmaps)):
            at = np.nonzero(group_of == g)[0]
            if len(at):
                keys[at], dist[at], cnt[at] = self.gpu.search_batch_filtered(Q[at], k, ef, bitmaps[g], n_bits)
        return keys, dist, cnt

    def check(self, Q, bitmaps, n_bits, group_of, k, ef, what, oracle_queries=None):
        """the grouped call against both yardsticks; returns its answers"""
        group_of = np.asarray(group_of, dtype=np.uint32)
        gk, gd, gcnt = self.gpu.search_batch_filtered_groups(Q, k, ef, bitmaps, n_bits, group_of)
        stats = self.gpu.last_query_stats(len(Q)).copy()
        totals = self.gpu.last_search_stats().copy()
        shape = self.gpu.last_search_shape().copy()
        pk, pd, pcnt = self.per_group(Q, bitmaps, n_bits, group_of, k, ef)
        bad = [q for q in range(len(Q)) if not (np.array_equal(gk[q], pk[q]) and np.array_equal(_bits(gd[q]), _bits(pd[q]))
                                                 and gcnt[q] == pcnt[q])]
        assert not bad, "%s: %d of %d queries differ from their group's own filtered call; first: query %d of group %d, %r / %r" % (
            what, len(bad), len(Q), bad[0], group_of[bad[0]], gk[bad[0]].tolist(), pk[bad[0]].tolist())
        sel = np.arange(len(Q)) if oracle_queries is None else np.arange(oracle_queries)
        ck, cd, ccnt, cst = self.oracle(Q[sel], bitmaps, n_bits, group_of[sel], k, ef)
        bad = [int(q) for q in sel if not (np.array_equal(gk[q], ck[q]) and np.array_equal(_bits(gd[q]), _bits(cd[q]))
                                           and gcnt[q] == ccnt[q])]
        assert not bad, "%s: %d of %d queries differ from the oracle; first: query %d of group %d, %r / %r" % (
            what, len(bad), len(sel), bad[0], group_of[bad[0]], gk[bad[0]].tolist(), ck[bad[0]].tolist())
        assert np.array_equal(stats[sel], cst.astype(np.uint32)), (what, "per-query work counters")
        assert totals[0] == stats[:, 0].sum() and totals[1] == stats[:, 1].sum() and totals[2] == len(Q), (what, totals)
        # every returned row is live and admitted by its OWN group; unused cells are -1 / +inf
        for q in range(len(Q)):
            row = gk[q, :gcnt[q]]
            assert np.all(_admits(bitmaps[group_of[q]], n_bits, row)), (what, q)
            assert not set(row.tolist()) & set(self.dead.tolist()), (what, q)
            assert np.all(gk[q, gcnt[q]:] == -1) and np.all(np.isinf(gd[q, gcnt[q]:])), (what, q)
        return dict(keys=gk, dist=gd, cnt=gcnt, stats=stats, totals=totals, shape=shape)


def _case_a(metric):
    """4000 x 32, keys 2i + 1, every ninth row removed, n_bits = 2n - 3: a 0.5 bitmap, its complement, all ones with padding"""
    n = 4000
    keys = np.arange(n, dtype=np.int64) * 2 + 1
    g = Graph(metric, n=n, keys=keys, dead=keys[::9])
    n_bits = 2 * n - 3
    half = golden_cases.filter_bitmap(n_bits, 41, 0.5)
    g.n_bits = n_bits
    g.three = np.stack([half, ~half, _all_ones(n_bits)])
    assert n_bits % 64 and g.three[2][-1] == ONES  # (the padding IS set)
    return g


_graphs = {}


def graph_a(metric):
    if metric not in _graphs:
        _graphs[metric] = _case_a(metric)
    return _graphs[metric]


@pytest.mark.parametrize("metric", ["l2sq", "cosine"])
def test_a_adjacent_queries_different_predicates(metric):
    """group_of = q % 3: neighbouring walkers of one workgroup hold different groups.  Groups 0 and 1 are complements, so
    they share no returned row."""
    g = graph_a(metric)
    group_of = np.arange(len(g.Q)) % 3
    for k, ef in ((10, 64), (20, 200)):
        r = g.check(g.Q, g.three, g.n_bits, group_of, k, ef, (metric, k, ef))
        rows = [set(r["keys"][group_of == grp][r["keys"][group_of == grp] >= 0].tolist()) for grp in (0, 1)]
        assert rows[0] and rows[1] and not rows[0] & rows[1]
        assert np.all(r["cnt"] == k)


@pytest.mark.parametrize("solo,shape6", [(0, 0), (2, 1)])
def test_b_same_inputs_in_both_launch_shapes(solo, shape6):
    """The workgroup engine (k_search) and one walking wave per query (k_search_solo), forced: the same answers, for the
    whole batch and for 1 and 3 queries alone."""
    g = graph_a("l2sq")
    group_of = np.arange(len(g.Q)) % 3
    g.gpu.set_option("search.solo", solo)
    try:
        for nq in (len(g.Q), 1, 3):
            r = g.check(g.Q[:nq], g.three, g.n_bits, group_of[:nq], 10, 64, ("solo", solo, nq))
            assert r["shape"][6] == shape6, r["shape"]
    finally:
        g.gpu.set_option("search.solo", 1)


def test_c_rerun_rounds_keep_the_predicate():
    """Two groups at 0.02 and 0.9, interleaved, k 10 / ef 48: queries of the rare group outgrow the register queue and are
    re-run through the launch's work list, where a walker's position in the queue is no longer its query — the re-run
    query must keep its own predicate.  Chosen fraction of the rare group: 0.02, as the issue set it; observed on the
    MI355X: last_search_stats()[3] == 48 after the grouped call (the count sums the re-run rounds' queries)."""
    g = graph_a("l2sq")
    two = np.stack([golden_cases.filter_bitmap(g.n_bits, 43, 0.02), golden_cases.filter_bitmap(g.n_bits, 44, 0.9)])
    group_of = np.arange(len(g.Q)) % 2
    r = g.check(g.Q, two, g.n_bits, group_of, 10, 48, "re-run rounds")
    print("re-run queries of the grouped call:", int(r["totals"][3]))
    assert r["totals"][3] > 0


@pytest.mark.parametrize("k,ef", [(600, 1024), (1000, 16)])
def test_d_limits_beyond_the_register_lists(k, ef):
    """4000 x 32, M 8 / M0 16 / ef_construction 700, groups at 0.01 and 0.3: candidate lists beyond the registers, an unbounded
    queue.  Every seventh row is removed first, as test_limits_beyond_the_register_lists_and_rare_predicates does before its
    predicates: tombstones and a predicate together."""
    if "d" not in _graphs:
        n = 4000
        _graphs["d"] = Graph("l2sq", n=n, dim=32, nq=24, M=8, M0=16, efc=700, build=(64, 4), dead=np.arange(0, n, 7), seed=2468)
    g = _graphs["d"]
    two = np.stack([golden_cases.filter_bitmap(g.n, 605, 0.01), golden_cases.filter_bitmap(g.n, 606, 0.3)])
    g.check(g.Q, two, g.n, np.arange(len(g.Q)) % 2, k, ef, ("limits", k, ef))


def test_e_degenerate_groups():
    g = graph_a("l2sq")
    Q, n_bits = g.Q[:12], g.n_bits
    # an all-zero group: count 0, cells -1 / +inf, and the call returns; next to it a group of five live rows
    five = np.zeros(_words(n_bits), dtype=np.uint64)
    live = [int(key) for key in g.keys[1:200:41] if key not in set(g.dead.tolist())][:5]
    assert len(live) == 5
    for key in live:
        five[key >> 6] |= np.uint64(1) << np.uint64(key & 63)
    tables = np.stack([np.zeros(_words(n_bits), dtype=np.uint64), five])
    group_of = np.arange(len(Q)) % 2
    r = g.check(Q, tables, n_bits, group_of, 10, 64, "empty and five rows")
    assert np.all(r["cnt"][group_of == 0] == 0) and np.all(r["keys"][group_of == 0] == -1)
    assert np.all(np.isposinf(r["dist"][group_of == 0]))
    assert np.all(r["cnt"][group_of == 1] <= 5) and np.all(r["cnt"][group_of == 1] > 0)
    # n_bits at both sides of a word edge, two groups; group 1's first word is all ones, so the bits that FOLLOW group 0's
    # n_bits in memory are set: rows with id >= n_bits stay rejected in group 0 (and in group 1)
    for small in (1, 63, 64, 65):
        tables = np.stack([_all_ones(small), _all_ones(small)])
        tables[0][-1] = ONES if small % 64 == 0 else np.uint64((1 << (small % 64)) - 1)  # group 0: no padding of its own
        r = g.check(Q, tables, small, group_of, 10, 64, ("n_bits", small))
        assert np.all(r["keys"][r["keys"] >= 0] < small)
        assert np.all(r["cnt"] <= sum(1 for key in g.keys if key < small and key not in set(g.dead.tolist())))


def test_f_a_whole_batch():
    """1024 queries, 7 groups of mixed density, pseudo-random group numbers; the oracle on the first 64 queries"""
    g = graph_a("l2sq")
    rng = np.random.default_rng(77)
    Q = np.ascontiguousarray(np.tile(g.Q, (22, 1))[:1024] + rng.normal(0, 0.05, size=(1024, g.dim)).astype(np.float32))
    fractions = (0.5, 0.05, 0.9, 0.2, 1 / 16, 0.7)
    tables = np.stack([golden_cases.filter_bitmap(g.n_bits, 900 + i, f) for i, f in enumerate(fractions)] + [_all_ones(g.n_bits)])
    group_of = rng.integers(0, 7, size=1024)
    assert len(set(group_of.tolist())) == 7
    g.check(Q, tables, g.n_bits, group_of, 10, 64, "1024 queries", oracle_queries=64)


def test_g_errors():
    g = graph_a("l2sq")
    gpu, Q, n_bits = g.gpu, g.Q, g.n_bits
    lib = gpu.lib
    group_of = (np.arange(len(Q)) % 3).astype(np.uint32)
    before = gpu.search_batch(Q, 10, 64)
    keys = np.full((len(Q), 10), -7, dtype=np.int64)
    dist = np.zeros((len(Q), 10), dtype=np.float32)
    cnt = np.full(len(Q), 99, dtype=np.uint32)
    tables = np.ascontiguousarray(g.three)

    def call(allowed, n_groups, groups):
        rc = lib.vss_search_batch_filtered_groups(gpu.h, Q.ctypes.data, len(Q), 10, 64, allowed, n_groups, n_bits, groups,
                                                  keys.ctypes.data, dist.ctypes.data, cnt.ctypes.data)
        return rc, lib.vss_last_error(gpu.h).decode()

    rc, why = call(None, 3, group_of.ctypes.data)
    assert rc != 0 and "needs the groups' row-id bitmaps" in why, why
    rc, why = call(tables.ctypes.data, 3, None)
    assert rc != 0 and "needs the group of every query" in why, why
    rc, why = call(tables.ctypes.data, 0, group_of.ctypes.data)
    assert rc != 0 and "needs at least one group" in why, why
    bad = group_of.copy()
    bad[31], bad[17] = 3, 9
    rc, why = call(tables.ctypes.data, 3, bad.ctypes.data)
    assert rc != 0 and "query 17 names group 9, the table holds 3" in why, why
    assert np.all(keys == -7) and np.all(cnt == 99)  # nothing was launched, nothing written
    with pytest.raises(RuntimeError, match="query 17 names group 9"):
        gpu.search_batch_filtered_groups(Q, 10, 64, tables, n_bits, bad)
    with pytest.raises(ValueError):
        gpu.search_batch_filtered_groups(Q, 10, 64, tables[:, :-1], n_bits, group_of)
    # no queries: nothing to refuse
    assert lib.vss_search_batch_filtered_groups(gpu.h, None, 0, 10, 64, None, 0, n_bits, None, None, None, None) == 0
    after = gpu.search_batch(Q, 10, 64)
    for a, b in zip(before, after):
        assert np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b)
    good = gpu.search_batch_filtered_groups(Q, 10, 64, tables, n_bits, group_of)

    # device form: the engine cannot see the group numbers; a query of an unknown group is answered as if its predicate
    # admitted nothing, its neighbours are unaffected, and the table's buffer ends where the table ends
    import torch
    d_Q = torch.from_numpy(Q).cuda()
    d_tables = torch.from_numpy(tables.view(np.int64)).cuda()
    d_groups = torch.from_numpy(bad.view(np.int32)).cuda()
    d_keys = torch.full((len(Q), 10), -7, dtype=torch.int64, device="cuda")
    d_dist = torch.zeros((len(Q), 10), dtype=torch.float32, device="cuda")
    d_cnt = torch.full((len(Q),), 99, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gpu.search_batch_filtered_groups_device(d_Q.data_ptr(), len(Q), 10, 64, d_tables.data_ptr(), 3, n_bits, d_groups.data_ptr(),
                                            d_keys.data_ptr(), d_dist.data_ptr(), d_cnt.data_ptr())
    torch.cuda.synchronize()
    dk, dd, dc = d_keys.cpu().numpy(), d_dist.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32)
    for q in (17, 31):
        assert dc[q] == 0 and np.all(dk[q] == -1) and np.all(np.isposinf(dd[q])), (q, dk[q], dd[q], dc[q])
    rest = np.setdiff1d(np.arange(len(Q)), (17, 31))
    assert np.array_equal(dk[rest], good[0][rest]) and np.array_equal(_bits(dd[rest]), _bits(good[1][rest]))
    assert np.array_equal(dc[rest], good[2][rest])
    with pytest.raises(RuntimeError, match="needs the group of every query"):
        gpu.search_batch_filtered_groups_device(d_Q.data_ptr(), len(Q), 10, 64, d_tables.data_ptr(), 3, n_bits, None,
                                                d_keys.data_ptr(), d_dist.data_ptr(), d_cnt.data_ptr())


def test_h_one_table_across_a_block_edge_of_the_resolve_kernel():
    """The single-table device calls resolve their bitmaps through the batched resolve kernel, as a launch of one batch: 257
    queries are two 256-thread blocks of it, the second with one live thread.  Queries 0, 255 and 256 — the first thread, the
    last of block 0 and the only one of block 1 — name groups the table does not hold and come back empty; every other query
    gets what search_batch_filtered returns for it under its own group's bitmap.  The pipelined form on context 1 returns the
    same cells."""
    import torch
    g = graph_a("l2sq")
    nq, k, ef = 257, 10, 64
    rng = np.random.default_rng(257)
    Q = np.ascontiguousarray(np.tile(g.Q, (6, 1))[:nq] + rng.normal(0, 0.05, size=(nq, g.dim)).astype(np.float32))
    group_of = (np.arange(nq) % 3).astype(np.uint32)
    unknown = np.array([0, 255, 256])
    group_of[unknown] = (3, 7, 4000000000)
    known = np.setdiff1d(np.arange(nq), unknown)
    pk, pd, pcnt = g.per_group(Q, g.three, g.n_bits, group_of, k, ef)  # (groups 0-2 only: the unknown stay -1 / +inf / 0)

    d_Q = torch.from_numpy(Q).cuda()
    d_tables = torch.from_numpy(np.ascontiguousarray(g.three).view(np.int64)).cuda()
    d_groups = torch.from_numpy(group_of.view(np.int32)).cuda()

    def cells(run):
        d_keys = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
        d_dist = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        d_cnt = torch.full((nq,), 99, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        run(d_Q.data_ptr(), nq, k, ef, d_tables.data_ptr(), 3, g.n_bits, d_groups.data_ptr(), d_keys.data_ptr(),
            d_dist.data_ptr(), d_cnt.data_ptr())
        torch.cuda.synchronize()
        return d_keys.cpu().numpy(), d_dist.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32)

    def pipelined(*args):
        g.gpu.search_filtered_groups_begin(1, *args)
        g.gpu.search_end(1)

    dk, dd, dc = cells(g.gpu.search_batch_filtered_groups_device)
    for q in unknown:
        assert dc[q] == 0 and np.all(dk[q] == -1) and np.all(np.isposinf(dd[q])), (q, dk[q], dd[q], dc[q])
    assert np.array_equal(dk[known], pk[known]) and np.array_equal(_bits(dd[known]), _bits(pd[known]))
    assert np.array_equal(dc[known], pcnt[known]) and np.all(dc[known] > 0)
    bk, bd, bc = cells(pipelined)
    assert np.array_equal(bk, dk) and np.array_equal(_bits(bd), _bits(dd)) and np.array_equal(bc, dc)


def test_group_tables_are_counted_in_memory_usage():
    g = graph_a("l2sq")
    fresh = gc.gpu_index(g.dim, "l2sq")
    fresh.load(g.gpu.save())
    base = fresh.memory_usage()
    fresh.search_batch_filtered_groups(g.Q, 10, 64, g.three, g.n_bits, np.arange(len(g.Q)) % 3)
    assert fresh.memory_usage() >= base + g.three.nbytes + 4 * len(g.Q)
