"""-m gpu: filtered probes through the pipelined and the multi-batch calls — vss_search_batch_filtered_device_begin,
vss_search_batch_filtered_groups_device_begin and vss_search_multi_filtered_device_begin, each completed by
vss_search_batch_end.  Their contract restates the blocking calls': every query gets, bit for bit, what
vss_search_batch_filtered_device returns for it alone under its own bitmap.  Every test therefore holds the new call against
two yardsticks, cell by cell (row ids, f32 distance bits, counts): the existing blocking call on the same index, and the
oracle (search_many_filtered per query with that query's own bitmap).  A query whose group number is not in its table has no
bitmap to hand the oracle: it is given an all-zero one there, which is what the contract says such a query is answered like.

The graphs are those of tests/test_gpu_filter_groups.py (imported, with its cache of built graphs and oracle answers)."""
import numpy as np
import pytest

import gpu_common as gc
import golden_cases
import test_gpu_filter_groups as fg

pytestmark = pytest.mark.gpu

_bits, _words, _all_ones = fg._bits, fg._words, fg._all_ones


def _dev(a):
    """a numpy array on the device (torch has no unsigned 32 / 64-bit tensors: the same bytes, signed)"""
    import torch
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).cuda()


class Cells:
    """the device cells of one batch of answers, pre-filled (-7 / 0 / 99) so that a cell nobody wrote shows"""

    def __init__(self, nq, k, dist=True):
        import torch
        self.keys = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
        self.dist = torch.zeros((nq, k), dtype=torch.float32, device="cuda") if dist else None
        self.cnt = torch.full((nq,), 99, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def ptrs(self):
        return self.keys.data_ptr(), self.dist.data_ptr() if self.dist is not None else 0, self.cnt.data_ptr()

    def fetch(self):
        import torch
        torch.cuda.synchronize()
        return (self.keys.cpu().numpy(), self.dist.cpu().numpy() if self.dist is not None else None,
                self.cnt.cpu().numpy().view(np.uint32))

    def untouched(self):
        k, d, c = self.fetch()
        return np.all(k == -7) and np.all(c == 99) and (d is None or np.all(d == 0))


def _same(got, want, what):
    gk, gd, gcnt = got
    wk, wd, wcnt = want
    bad = [q for q in range(len(wk)) if not (np.array_equal(gk[q], wk[q]) and gcnt[q] == wcnt[q]
                                             and (gd is None or np.array_equal(_bits(gd[q]), _bits(wd[q]))))]
    assert not bad, "%s: %d of %d queries differ; first: query %d, %r / %r" % (what, len(bad), len(wk), bad[0],
                                                                              gk[bad[0]].tolist(), wk[bad[0]].tolist())


class Batch:
    """One chunk of a join: its queries, its own table of bitmaps and its group numbers (None = no group numbers: every query
    takes bitmap 0), on the host and on the device; and what both yardsticks say it is answered with."""

    def __init__(self, g, Q, tables, group_of, n_bits, k, ef):
        self.Q = np.ascontiguousarray(Q, dtype=np.float32)
        self.tables = np.ascontiguousarray(np.atleast_2d(tables), dtype=np.uint64)
        assert self.tables.shape[1] == _words(n_bits)
        self.group_of = None if group_of is None else np.ascontiguousarray(group_of, dtype=np.uint32)
        self.n_bits, self.k, self.ef = n_bits, k, ef
        self.d_Q, self.d_tables = _dev(self.Q), _dev(self.tables)
        self.d_group_of = None if group_of is None else _dev(self.group_of)
        self.d_zeros = _dev(np.zeros(len(self.Q), dtype=np.uint32))
        self._expect(g)

    def groups(self):
        return np.zeros(len(self.Q), dtype=np.uint32) if self.group_of is None else self.group_of

    def group_ptr(self):
        return 0 if self.d_group_of is None else self.d_group_of.data_ptr()

    def _expect(self, g):
        # yardstick 1: the blocking grouped device call (it answers a query of an unknown group with count 0, -1 / +inf)
        cells = Cells(len(self.Q), self.k)
        g.gpu.search_batch_filtered_groups_device(self.d_Q.data_ptr(), len(self.Q), self.k, self.ef, self.d_tables.data_ptr(),
                                                  len(self.tables), self.n_bits,
                                                  (self.d_zeros if self.d_group_of is None else self.d_group_of).data_ptr(),
                                                  *cells.ptrs())
        self.want = cells.fetch()
        self.stats = g.gpu.last_search_stats().copy()
        # yardstick 2: the oracle, per query under its own bitmap; an unknown group = a bitmap that admits nothing
        padded = np.vstack([self.tables, np.zeros((1, self.tables.shape[1]), dtype=np.uint64)])
        known = np.minimum(self.groups(), len(self.tables))
        ok, od, ocnt, _ = g.oracle(self.Q, padded, self.n_bits, known, self.k, self.ef)
        _same(self.want, (ok, od, ocnt), "the blocking call against the oracle")
        for q in np.nonzero(self.groups() >= len(self.tables))[0]:
            assert self.want[2][q] == 0 and np.all(self.want[0][q] == -1) and np.all(np.isposinf(self.want[1][q])), q


def _multi_begin(gpu, context, batches, cells):
    b0 = batches[0]
    gpu.search_multi_filtered_begin(context, [b.d_Q.data_ptr() for b in batches], len(b0.Q), b0.k, b0.ef,
                                    [b.d_tables.data_ptr() for b in batches], [len(b.tables) for b in batches], b0.n_bits,
                                    [b.group_ptr() for b in batches], [c.ptrs()[0] for c in cells], [c.ptrs()[1] for c in cells],
                                    [c.ptrs()[2] for c in cells])


def _more_queries(g, nq, seed):
    rng = np.random.default_rng(seed)
    reps = -(-nq // len(g.Q))
    return np.ascontiguousarray(np.tile(g.Q, (reps, 1))[:nq] + rng.normal(0, 0.05, size=(nq, g.dim)).astype(np.float32))


@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_a_one_bitmap_three_contexts_in_flight(metric):
    """16 queries per context, k 10 / ef 64: a 0.5 bitmap on context 0, its complement on 1, a 0.02 bitmap on 2; completed in
    the order 2, 0, 1.  A context in flight refuses a second _begin, and the index refuses to be reserved meanwhile."""
    g = fg.graph_a(metric)
    gpu, n_bits, k, ef = g.gpu, g.n_bits, 10, 64
    bitmaps = [g.three[0], g.three[1], golden_cases.filter_bitmap(n_bits, 42, 0.02)]
    Qs = [np.ascontiguousarray(g.Q[16 * c:16 * c + 16]) for c in range(3)]
    want = [gpu.search_batch_filtered(Qs[c], k, ef, bitmaps[c], n_bits) for c in range(3)]
    d_Q, d_bitmaps, cells = [_dev(Q) for Q in Qs], [_dev(b) for b in bitmaps], [Cells(16, k) for _ in range(3)]
    for c in range(3):
        gpu.search_filtered_begin(c, d_Q[c].data_ptr(), 16, k, ef, d_bitmaps[c].data_ptr(), n_bits, *cells[c].ptrs())
    with pytest.raises(gc.pkg().VssError, match="already has a batch in flight"):
        gpu.search_filtered_begin(1, d_Q[0].data_ptr(), 16, k, ef, d_bitmaps[0].data_ptr(), n_bits, *cells[0].ptrs())
    with pytest.raises(gc.pkg().VssError, match="vss_reserve while search context"):
        gpu.reserve(4 * g.n)
    for c in (2, 0, 1):
        gpu.search_end(c)
    for c in range(3):
        _same(cells[c].fetch(), want[c], (metric, "context", c, "against search_batch_filtered"))
        ok, od, ocnt, _ = g.oracle(Qs[c], np.stack(bitmaps), n_bits, np.full(16, c), k, ef)
        _same(cells[c].fetch(), (ok, od, ocnt), (metric, "context", c, "against the oracle"))
    assert all(c.fetch()[2].sum() > 0 for c in cells)  # (no comparison of empty answers)
    # nothing to do: nothing pending
    gpu.search_filtered_begin(3, None, 0, k, ef, None, n_bits, None, None, None)
    gpu.search_filtered_begin(3, d_Q[0].data_ptr(), 16, k, ef, d_bitmaps[0].data_ptr(), n_bits, *cells[0].ptrs())
    gpu.search_end(3)
    _same(cells[0].fetch(), want[0], (metric, "context 3 after an empty _begin"))
    with pytest.raises(gc.pkg().VssError, match="needs a row-id bitmap"):
        gpu.search_filtered_begin(3, d_Q[0].data_ptr(), 16, k, ef, None, n_bits, *cells[0].ptrs())


def test_b_groups_form_on_two_contexts():
    """Each context its own table: three groups with group_of = q % 3 on context 1; on context 2 five groups, one of them
    all zeros, and two queries whose group number is beyond the table — count 0, cells -1 / +inf, neighbours unaffected (the
    blocking device form's answer, tests/test_gpu_filter_groups.py::test_g_errors)."""
    g = fg.graph_a("l2sq")
    gpu, n_bits, k, ef = g.gpu, g.n_bits, 10, 64
    five = np.stack([golden_cases.filter_bitmap(n_bits, 50, 0.3), np.zeros(_words(n_bits), dtype=np.uint64),
                     golden_cases.filter_bitmap(n_bits, 51, 0.05), _all_ones(n_bits), g.three[1]])
    groups5 = (np.arange(24) % 5).astype(np.uint32)
    groups5[17], groups5[6] = 9, 5
    batches = [Batch(g, g.Q[:24], g.three, np.arange(24) % 3, n_bits, k, ef), Batch(g, g.Q[24:48], five, groups5, n_bits, k, ef)]
    cells = [Cells(24, k), Cells(24, k)]
    for context, b, c in zip((1, 2), batches, cells):
        gpu.search_filtered_groups_begin(context, b.d_Q.data_ptr(), 24, k, ef, b.d_tables.data_ptr(), len(b.tables), n_bits,
                                         b.group_ptr(), *c.ptrs())
    gpu.search_end(1)
    gpu.search_end(2)
    for b, c in zip(batches, cells):
        _same(c.fetch(), b.want, "groups form")
    got = cells[1].fetch()
    for q in (6, 17):
        assert got[2][q] == 0 and np.all(got[0][q] == -1) and np.all(np.isposinf(got[1][q]))
    assert np.all(got[2][groups5 == 1] == 0) and np.all(got[2][groups5 == 3] > 0)
    with pytest.raises(gc.pkg().VssError, match="needs the group of every query"):
        gpu.search_filtered_groups_begin(1, batches[0].d_Q.data_ptr(), 24, k, ef, batches[0].d_tables.data_ptr(), 3, n_bits, None,
                                         *cells[0].ptrs())
    with pytest.raises(gc.pkg().VssError, match="needs at least one group"):
        gpu.search_filtered_groups_begin(1, batches[0].d_Q.data_ptr(), 24, k, ef, batches[0].d_tables.data_ptr(), 0, n_bits,
                                         batches[0].group_ptr(), *cells[0].ptrs())
    gpu.search_end(1)  # (nothing pending)


_case_c = {}


def five_batches():
    """5 batches x 13 queries, k 10 / ef 64, each batch its own table: 0 one bitmap without group numbers; 1 three groups,
    interleaved; 2 all ones with set padding; 3 three groups and one group number the table does not hold; 4 an all-zero
    bitmap without group numbers."""
    if not _case_c:
        g = fg.graph_a("l2sq")
        Q, n_bits = _more_queries(g, 65, 78), g.n_bits
        zeros = np.zeros(_words(n_bits), dtype=np.uint64)
        unknown = (np.arange(13) % 3).astype(np.uint32)
        unknown[5] = 3
        spec = [(g.three[0], None), (g.three, np.arange(13) % 3), (_all_ones(n_bits), np.zeros(13)), (g.three, unknown), (zeros, None)]
        _case_c["batches"] = [Batch(g, Q[13 * b:13 * b + 13], tables, groups, n_bits, 10, 64) for b, (tables, groups) in enumerate(spec)]
    return fg.graph_a("l2sq"), _case_c["batches"]


def _check_five(cells, batches, what, skip_dist=()):
    for b, (c, batch) in enumerate(zip(cells, batches)):
        got = c.fetch()
        assert (got[1] is None) == (b in skip_dist)
        _same(got, batch.want, (what, "batch", b))
    got = cells[3].fetch()
    assert got[2][5] == 0 and np.all(got[0][5] == -1)
    assert np.all(cells[4].fetch()[2] == 0) and np.all(cells[2].fetch()[2] > 0)


@pytest.mark.parametrize("solo,shape6", [(1, None), (0, 0), (2, 1)])
def test_c_five_batches_one_launch(solo, shape6):
    """One launch answers the five batches; every batch equals its own blocking grouped device call and the oracle, the work
    counters are the sum of the five calls', and both kernels (k_search_groups: search.solo 0, k_search_solo_groups: 2) carry
    such a launch.  Batch 1 has no distance buffer."""
    g, batches = five_batches()
    g.gpu.set_option("search.solo", solo)
    try:
        cells = [Cells(13, 10, dist=b != 1) for b in range(5)]
        _multi_begin(g.gpu, 1, batches, cells)
        g.gpu.search_end(1)
        st, shape = g.gpu.last_search_stats().copy(), g.gpu.last_search_shape().copy()
    finally:
        g.gpu.set_option("search.solo", 1)
    _check_five(cells, batches, ("solo", solo), skip_dist=(1,))
    print("work counters of the launch:", st.tolist(), "of the five calls:", [b.stats.tolist() for b in batches])
    assert int(st[0]) == sum(int(b.stats[0]) for b in batches) and int(st[1]) == sum(int(b.stats[1]) for b in batches)
    assert int(st[2]) == 65
    if shape6 is not None:
        assert shape[6] == shape6, shape


def test_d_edges_of_the_batch_count():
    g = fg.graph_a("l2sq")
    gpu, n_bits, k, ef = g.gpu, g.n_bits, 10, 64
    Q = _more_queries(g, 64, 79)
    # 32 batches x 2 queries: one table address for all of them, every batch its own two group numbers
    batches = [Batch(g, Q[2 * b:2 * b + 2], g.three, [b % 3, (b + 1) % 3], n_bits, k, ef) for b in range(32)]
    for b in batches[1:]:
        b.d_tables = batches[0].d_tables
    cells = [Cells(2, k) for _ in range(32)]
    _multi_begin(gpu, 2, batches, cells)
    gpu.search_end(2)
    assert int(gpu.last_search_stats()[2]) == 64
    for b in range(32):
        _same(cells[b].fetch(), batches[b].want, ("32 batches", b))
    # 1 batch = the groups _begin form
    one = Batch(g, g.Q[:24], g.three, np.arange(24) % 3, n_bits, k, ef)
    multi, single = Cells(24, k), Cells(24, k)
    _multi_begin(gpu, 0, [one], [multi])
    gpu.search_end(0)
    gpu.search_filtered_groups_begin(0, one.d_Q.data_ptr(), 24, k, ef, one.d_tables.data_ptr(), 3, n_bits, one.group_ptr(),
                                     *single.ptrs())
    gpu.search_end(0)
    _same(multi.fetch(), single.fetch(), "one batch against the groups _begin form")
    _same(multi.fetch(), one.want, "one batch")
    # refusals: nothing is enqueued, nothing written
    fresh = [Cells(2, k) for _ in range(33)]
    with pytest.raises(gc.pkg().VssError, match="1 to 32 batches per launch"):
        _multi_begin(gpu, 2, batches + [batches[0]], fresh)
    three = batches[:3]

    def refused(match, tables=None, n_groups=None):
        with pytest.raises(gc.pkg().VssError, match=match):
            gpu.search_multi_filtered_begin(2, [b.d_Q.data_ptr() for b in three], 2, k, ef,
                                            tables or [b.d_tables.data_ptr() for b in three], n_groups or [3, 3, 3], n_bits,
                                            [b.group_ptr() for b in three], [c.ptrs()[0] for c in fresh[:3]],
                                            [c.ptrs()[1] for c in fresh[:3]], [c.ptrs()[2] for c in fresh[:3]])

    refused("batch 1 needs at least one group", n_groups=[3, 0, 3])
    refused("batch 2 needs its groups' row-id bitmaps", tables=[three[0].d_tables.data_ptr(), three[1].d_tables.data_ptr(), 0])
    refused("batch 0: .* more than a table can hold", n_groups=[1 << 62, 3, 3])
    with pytest.raises(gc.pkg().VssError, match="out of range"):
        _multi_begin(gpu, 4, three, fresh[:3])
    with pytest.raises(gc.pkg().VssError, match="null table"):
        gpu.search_multi_filtered_begin(2, [b.d_Q.data_ptr() for b in three], 2, k, ef, None, [3, 3, 3], n_bits,
                                        [b.group_ptr() for b in three], [c.ptrs()[0] for c in fresh[:3]],
                                        [c.ptrs()[1] for c in fresh[:3]], [c.ptrs()[2] for c in fresh[:3]])
    gpu.search_end(2)  # (nothing pending)
    assert all(c.untouched() for c in fresh)
    # a launch of no queries: nothing to refuse, nothing pending
    gpu.search_multi_filtered_begin(2, [0, 0], 0, k, ef, [0, 0], [0, 0], n_bits, [0, 0], [0, 0], [0, 0], [0, 0])
    gpu.search_end(2)


def test_e_rerun_rounds_keep_the_predicate_across_batches():
    """The input of test_c_rerun_rounds_keep_the_predicate (bitmaps at 0.02 and 0.9, group_of = q % 2, k 10 / ef 48; 48 re-run
    queries on the MI355X), split into 4 batches of 12 in one launch: a re-run query is found through the launch's work list,
    and must keep the predicate of ITS batch's table."""
    g = fg.graph_a("l2sq")
    n_bits = g.n_bits
    two = np.stack([golden_cases.filter_bitmap(n_bits, 43, 0.02), golden_cases.filter_bitmap(n_bits, 44, 0.9)])
    group_of = (np.arange(len(g.Q)) % 2).astype(np.uint32)
    want = g.gpu.search_batch_filtered_groups(g.Q, 10, 48, two, n_bits, group_of)
    reruns = int(g.gpu.last_search_stats()[3])
    print("re-run queries of the blocking grouped call:", reruns)
    assert reruns > 0  # the yardstick itself: without re-run rounds this test would show nothing
    batches = [Batch(g, g.Q[12 * b:12 * b + 12], two, group_of[12 * b:12 * b + 12], n_bits, 10, 48) for b in range(4)]
    cells = [Cells(12, 10) for _ in range(4)]
    _multi_begin(g.gpu, 1, batches, cells)
    g.gpu.search_end(1)
    st = g.gpu.last_search_stats().copy()
    print("re-run queries of the multi-batch launch:", int(st[3]))
    for b in range(4):
        _same(cells[b].fetch(), tuple(a[12 * b:12 * b + 12] for a in want), ("re-run rounds, against the blocking call", b))
        _same(cells[b].fetch(), batches[b].want, ("re-run rounds, against the oracle's yardstick", b))
    assert int(st[3]) == reruns and int(st[2]) == 48


def test_f_limits_beyond_the_register_lists():
    """test_d_limits_beyond_the_register_lists' graph (M 8 / M0 16 / ef_construction 700, every seventh row removed), groups at
    0.01 and 0.3, k 600 / ef 1024: candidate lists beyond the registers and an unbounded queue, two batches of 12 in one launch."""
    if "d" not in fg._graphs:
        n = 4000
        fg._graphs["d"] = fg.Graph("l2sq", n=n, dim=32, nq=24, M=8, M0=16, efc=700, build=(64, 4), dead=np.arange(0, n, 7), seed=2468)
    g = fg._graphs["d"]
    two = np.stack([golden_cases.filter_bitmap(g.n, 605, 0.01), golden_cases.filter_bitmap(g.n, 606, 0.3)])
    group_of = np.arange(len(g.Q)) % 2
    batches = [Batch(g, g.Q[12 * b:12 * b + 12], two, group_of[12 * b:12 * b + 12], g.n, 600, 1024) for b in range(2)]
    cells = [Cells(12, 600) for _ in range(2)]
    _multi_begin(g.gpu, 3, batches, cells)
    g.gpu.search_end(3)
    for b in range(2):
        _same(cells[b].fetch(), batches[b].want, ("limits", b))


def test_g_two_launches_overlapping_on_two_contexts():
    """The five batches of test c as two launches in flight — batches 0-2 on context 0, 3-4 on context 2 — issued when the
    previous launch starts to drain (search.gating on, the default) or immediately (off): the same answers."""
    g, batches = five_batches()
    gpu = g.gpu
    try:
        for gated in (True, False):
            gpu.set_search_gating(gated)
            cells = [Cells(13, 10) for _ in range(5)]
            for rounds in range(3):
                _multi_begin(gpu, 0, batches[:3], cells[:3])
                _multi_begin(gpu, 2, batches[3:], cells[3:])
                gpu.search_end(0)
                gpu.search_end(2)
            _check_five(cells, batches, ("gating", gated))
    finally:
        gpu.set_search_gating(True)


def test_bitmap_addresses_are_counted_in_memory_usage():
    """the context's table of one bitmap address per query is sized for the 32 batches a launch may carry, and counted"""
    g, batches = five_batches()
    fresh = gc.gpu_index(g.dim, "l2sq")
    fresh.load(g.gpu.save())
    base = fresh.memory_usage()
    cells = [Cells(13, 10) for _ in range(5)]
    _multi_begin(fresh, 1, batches, cells)
    fresh.search_end(1)
    _check_five(cells, batches, "a fresh index")
    assert fresh.memory_usage() >= base + 8 * 32 * 13
