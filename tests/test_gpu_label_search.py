"""-m gpu: vss_search_batch_by_label — equality predicates on the index's resident label column (csrc/label_filter.h; the
walkers' admission in csrc/hnsw_kernels.h, the listing kernels in csrc/exact_filtered_kernels.h).

Contract, and the only yardstick here: let v_0 < v_1 < ... be the distinct values of `want`, bitmap g have bit r set iff
r < labelled_rows and labels[r] == v_g != NO_LABEL, and group_of[q] be the index of want[q].  Then the call in mode
graph / exact / auto returns cell for cell — row ids, f32 distance bits, counts, routes — what
vss_search_batch_filtered_groups / vss_search_exact_batch_filtered_groups / vss_search_batch_filtered_groups_auto return for
that table, and leaves the same counters behind.  No tolerance, no cell left out.  (The bitmap calls' own answers are held to
a CPU brute force in tests/test_gpu_exact_filtered.py, test_gpu_filter_groups.py and test_gpu_filter_route.py.)

Two things the cases below could not take from their description as it stood, both arithmetic:
  * the mixed chunk has 6000 rows of ids 3001 .. 9000 with labels for ids < 8000, i.e. 4999 labelled rows: tenants of 3000 and
    1500 rows leave 499, so the six middling tenants hold about 80 rows each, not 200.  With L = 6000 and limit 64 the rule
    under route_c = 1500 is len <= 3000: the 3000-row tenant sits exactly ON the boundary (exact).  route_c = 1499 and 3 are
    run as well, so that one call has both routes.
  * labels partition the rows, so the lists of one call never hold more than `rows` entries and always fit one pass of the
    exact plan, whose budget is max(VSS_EXACT_FILTER_LIST_ENTRIES, rows).  The small-budget case runs and is compared, with
    the pass count the bitmap call reports (1).
"""
import numpy as np
import pytest

import gpu_common as gc
from test_gpu_exact_filtered import _bitmap, _words, assert_same, keys_against_slot_order

pytestmark = pytest.mark.gpu

NO_LABEL = 0xFFFFFFFF
MODES = ("graph", "exact", "auto")


def build(dim, metric, X, keys, capacity=None, M=16, M0=32, efc=64):
    gpu = gc.gpu_index(dim, metric, M, M0, efc)
    gpu.reserve(capacity or len(X))
    gpu.set_build_params(32768, 4)
    gpu.add(keys, X)
    return gpu


def derived_table(labels, want):
    """the table of the contract: (bitmaps, n_bits, group_of)"""
    labels = np.asarray(labels, dtype=np.uint32)
    values, group_of = np.unique(np.asarray(want, dtype=np.uint32), return_inverse=True)
    n_bits = len(labels)
    bitmaps = np.zeros((len(values), _words(n_bits)), dtype=np.uint64)
    for g, v in enumerate(values):
        if v != NO_LABEL:
            bitmaps[g] = _bitmap(n_bits, np.nonzero(labels == v)[0])
    return bitmaps, n_bits, group_of.astype(np.uint32)


def counters(gpu, mode):
    c = {}
    if mode != "exact":
        c["stats"], c["shape"] = gpu.last_search_stats().tolist(), gpu.last_search_shape().tolist()
        c["prescore"], c["descent"] = gpu.last_search_prescore().tolist(), gpu.last_search_prescore_descent().tolist()
    if mode != "graph":
        c["exact"] = gpu.last_exact_filtered()[:3].tolist()
    if mode == "auto":
        c["route"] = gpu.last_filter_route().tolist()
    return c


def bitmap_call(gpu, mode, Q, k, ef, table, route_c):
    bitmaps, n_bits, group_of = table
    if mode == "graph":
        return gpu.search_batch_filtered_groups(Q, k, ef, bitmaps, n_bits, group_of) + (np.zeros(len(Q), np.uint8),)
    if mode == "exact":
        return gpu.search_exact_batch_filtered_groups(Q, k, bitmaps, n_bits, group_of) + (np.ones(len(Q), np.uint8),)
    return gpu.search_batch_filtered_groups_auto(Q, k, ef, bitmaps, n_bits, group_of, route_c)


def check(gpu, Q, k, ef, labels, want, route_c, what, modes=MODES):
    """every mode against the bitmap call of that mode on the derived table: answers, routes, counters.  Returns
    {mode: (the by-label answer, the bitmap call's counters)}"""
    assert gpu.labelled_rows() == len(labels), what
    table = derived_table(labels, want)
    out = {}
    for mode in modes:
        where = "%s, mode %s, route_c %d" % (what, mode, route_c)
        ref = bitmap_call(gpu, mode, Q, k, ef, table, route_c)
        ref_counters = counters(gpu, mode)
        got = gpu.search_batch_by_label(Q, k, ef, want, mode, route_c)
        got_counters = counters(gpu, mode)
        assert_same(got[:3], ref[:3], where)
        assert np.array_equal(got[3], ref[3]), where + ": routes"
        assert got_counters == ref_counters, where + ": counters %r, the bitmap call's %r" % (got_counters, ref_counters)
        out[mode] = (got, ref_counters)
    return out


def assert_nothing(answer, rows, what):
    ids, dist, cnt, _ = answer
    assert np.all(cnt[rows] == 0) and np.all(ids[rows] == -1) and np.all(np.isposinf(dist[rows])), what


# ------------------------------------------------------------------------------------------------- 1. the mixed chunk
def mixed_labels(keys, labelled, rng):
    """by row id: tenant 1 holds 3000 live rows, tenant 2 1500, tenants 10 .. 15 about 80 each, tenants 100 .. 104 one row each,
    20 rows NO_LABEL; ids that no row has keep tenant 7 (which no live row carries)"""
    labels = np.full(labelled, 7, dtype=np.uint32)
    mine = rng.permutation(keys[keys < labelled])
    labels[mine[:3000]] = 1
    labels[mine[3000:4500]] = 2
    labels[mine[4500:4505]] = 100 + np.arange(5)
    labels[mine[4505:4525]] = NO_LABEL
    labels[mine[4525:]] = 10 + rng.integers(0, 6, len(mine) - 4525)
    return labels


@pytest.mark.parametrize("dim", [3, 100, 768])  # dword rows, float4 rows, wide rows
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_mixed_chunk(metric, dim):
    n, nq, labelled = 6000, 37, 8000
    X, Q = gc.make_data(n, dim, metric, 1700 + dim, nq=nq)
    keys = keys_against_slot_order(n, 9000)  # row id != slot; row ids 3001 .. 9000, those from 8000 on without a cell
    rng = np.random.default_rng(17)
    labels = mixed_labels(keys, labelled, rng)
    assert (labels[keys[keys < labelled]] == 1).sum() == 3000 and (labels[keys[keys < labelled]] == 2).sum() == 1500
    # one NULL tenant, one value no row carries (7: only ids without a row), one nobody carries at all, two sharing tenant 11
    want = np.array([1] * 5 + [2] * 6 + [10, 11, 11, 12, 13, 14, 15] * 2 + [100, 101, 102, 103, 104] + [NO_LABEL, 7, 4_000_000_000]
                    + [1, 2, 10, 100], dtype=np.uint32)
    assert len(want) == nq
    want = want[rng.permutation(nq)]
    gpu = build(dim, metric, X, keys)
    gpu.set_labels(0, labels)
    what = "%s dim %d" % (metric, dim)
    got = check(gpu, Q, 10, 64, labels, want, 1500, what)
    for mode in MODES:
        assert_nothing(got[mode][0], np.isin(want, [NO_LABEL, 7, 4_000_000_000]), what + " " + mode)
    assert np.all(got["exact"][0][2][want == 1] == 10) and np.all(got["exact"][0][2][want == 100] == 1)
    assert np.all(got["auto"][0][3] == 1)  # len 3000 is ON the boundary of route_c 1500: exact
    check(gpu, Q, 10, 64, labels, want, 0, what, modes=("auto",))
    route = check(gpu, Q, 10, 64, labels, want, 1499, what, modes=("auto",))["auto"][0][3]
    assert np.all(route[want == 1] == 0) and np.all(route[want != 1] == 1)
    route = check(gpu, Q, 10, 64, labels, want, 3, what, modes=("auto",))["auto"][0][3]  # len^2 <= 18000: 134 rows
    assert np.all(route[np.isin(want, [1, 2])] == 0) and np.all(route[~np.isin(want, [1, 2])] == 1)


# ------------------------------------------------------------------------------------------------- 2. listing edges
def edge_labels(n, keys, labelled):
    """by SLOT (a listing wave owns 512 consecutive slots, a row of it 64): slots 0 .. 63 carry 64 different labels, the rest of
    the first block five labels in turn, the second block label 7 only, what follows a label nobody wants"""
    slot = np.arange(n)
    by_slot = np.where(slot < 64, 1000 + slot, np.where(slot < 512, slot % 5, np.where(slot < 1024, 7, 99_999))).astype(np.uint32)
    labels = np.full(labelled, NO_LABEL, dtype=np.uint32)
    labels[keys] = by_slot
    return labels


@pytest.mark.parametrize("n", [1, 511, 512, 513, 1025])  # FL_WAVE_SLOTS = 512
def test_listing_edges(n):
    dim = 8
    X, Q = gc.make_data(n, dim, "l2sq", 1710 + n, nq=72)
    keys = keys_against_slot_order(n, 2000)
    labels = edge_labels(n, keys, 2001)
    want = np.concatenate([1000 + np.arange(64), np.arange(5), [7, 123_456, NO_LABEL]]).astype(np.uint32)
    gpu = build(dim, "l2sq", X, keys, M=4, M0=8, efc=16)
    gpu.set_labels(0, labels)
    got = check(gpu, Q, 10, 64, labels, want, 1, "n %d" % n)
    listed = got["exact"][1]["exact"][0]
    assert listed == (n if n <= 1024 else 1024)  # every row but the one whose label nobody wants
    # a call whose values all sit in other blocks: the first block holds no wanted label
    if n > 512:
        check(gpu, Q[:3], 10, 64, labels, np.array([7, 7, 99_998], dtype=np.uint32), 1, "n %d, first block unwanted" % n)


def test_every_query_its_own_label():
    n, dim, nq = 1025, 8, 200
    X, Q = gc.make_data(n, dim, "l2sq", 1720, nq=nq)
    keys = keys_against_slot_order(n, 2000)
    labels = np.full(2001, NO_LABEL, dtype=np.uint32)
    labels[keys] = (np.arange(n) * 7 % nq).astype(np.uint32)  # neighbouring lanes carry different labels
    want = np.random.default_rng(1721).permutation(nq).astype(np.uint32)
    gpu = build(dim, "l2sq", X, keys, M=4, M0=8, efc=16)
    gpu.set_labels(0, labels)
    got = check(gpu, Q, 10, 64, labels, want, 1, "200 values")
    assert got["exact"][1]["exact"][0] == n and np.all(got["exact"][0][2] >= 5)


def test_small_list_budget(monkeypatch):
    n, dim, nq = 3000, 16, 24
    X, Q = gc.make_data(n, dim, "l2sq", 1730, nq=nq)
    keys = keys_against_slot_order(n, 5000)
    rng = np.random.default_rng(1731)
    labels = rng.integers(0, 12, 5001).astype(np.uint32)
    want = (np.arange(nq) % 12).astype(np.uint32)
    monkeypatch.setenv("VSS_EXACT_FILTER_LIST_ENTRIES", "1000")
    gpu = build(dim, "l2sq", X, keys, M=4, M0=8, efc=16)
    gpu.set_labels(0, labels)
    got = check(gpu, Q, 10, 64, labels, want, 0, "budget 1000", modes=("exact", "auto"))
    assert got["exact"][1]["exact"] == [n, 2 * n, 1]  # a partition fits one pass whatever the budget


# ------------------------------------------------------------------------------------------------- 3. kernel shapes
class Base:
    def __init__(self):
        self.metric, self.n, self.dim = "l2sq", 6000, 32
        self.X, self.Q = gc.make_data(self.n, self.dim, self.metric, 1740, nq=300)
        self.keys = keys_against_slot_order(self.n, 9000)
        rng = np.random.default_rng(1741)
        # tenants 0 .. 3 hold 3500 / 1500 / 700 / 290 rows, tenant 4 six, tenant 5 one, three rows NO_LABEL
        by_slot = np.repeat(np.arange(4), [3500, 1500, 700, 290]).astype(np.uint32)
        by_slot = np.concatenate([by_slot, [4] * 6, [5], [NO_LABEL] * 3]).astype(np.uint32)[rng.permutation(self.n)]
        self.labels = np.full(9001, NO_LABEL, dtype=np.uint32)
        self.labels[self.keys] = by_slot
        self.gpu = build(self.dim, self.metric, self.X, self.keys)
        self.gpu.set_labels(0, self.labels)

    def check(self, Q, k, ef, want, route_c, what, modes=MODES):
        return check(self.gpu, Q, k, ef, self.labels, np.asarray(want, dtype=np.uint32), route_c, what, modes)


@pytest.fixture(scope="module")
def base():
    return Base()


@pytest.mark.parametrize("ef", [64, 300, 600])  # lists in registers (2 and 8 per lane) and outside them
def test_list_widths(base, ef):
    want = np.arange(21) % 7  # tenant 6 does not exist
    route_c = {64: 1000, 300: 300, 600: 160}[ef]  # len^2 * 64 <= route_c * limit * 6000 ends near 3000 rows at each limit
    got = base.check(base.Q[:21], 100, ef, want, route_c, "ef %d" % ef)
    assert (got["graph"][1]["shape"][4] != 0) == (ef == 600)  # beyond 512 the list has left the registers (the bitmap call's shape)
    route = got["auto"][0][3]
    assert np.all(route[want == 0] == 0) and np.all(route[want != 0] == 1)  # tenant 0 (3500 rows) is walked, 1500 are scanned


def test_one_query_takes_the_solo_kernel():
    n, dim = 2000, 128
    X, Q = gc.make_data(n, dim, "l2sq", 1750, nq=4)
    keys = keys_against_slot_order(n, 3000)
    labels = (np.arange(3001) % 3).astype(np.uint32)
    gpu = build(dim, "l2sq", X, keys, M=8, M0=16, efc=32)
    gpu.set_labels(0, labels)
    for q in range(2):
        got = check(gpu, Q[q:q + 1], 10, 64, labels, np.array([q + 1], dtype=np.uint32), 1, "one query")
        assert got["graph"][1]["shape"][6] == 1 and got["graph"][0][2][0] == 10


@pytest.mark.parametrize("nq", [204, 300])  # the join's chunk; more than a launch of one query per compute unit
def test_host_batches(base, nq):
    want = np.random.default_rng(1760 + nq).integers(0, 7, nq)
    got = base.check(base.Q[:nq], 10, 64, want, 1500, "%d queries" % nq)
    assert set(got["auto"][0][3]) == {0, 1}


def test_rare_predicate_reruns(base):
    """tenants of six rows and of one: the walk rejects nearly every row it meets, its pending candidates outgrow the register
    queue, and the queries are re-run through the unbounded one — reading the same table of wanted labels again"""
    want = np.array([4, 5] * 8, dtype=np.uint32)
    got = base.check(base.Q[:16], 10, 64, want, 1500, "rare tenants", modes=("graph",))
    ids, _, cnt, _ = got["graph"][0]
    assert np.all(cnt[want == 4] <= 6) and np.all(cnt[want == 5] <= 1) and cnt.sum() > 0  # (a walk may miss a row; it invents none)
    assert got["graph"][1]["stats"][3] > 0  # (the bitmap call's counter: queries were re-run)


def test_device_form(base):
    import torch
    nq, k = 35, 10
    Q = base.Q[:nq]
    want = (np.arange(nq) % 7).astype(np.uint32)
    want[3] = NO_LABEL
    d_Q = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    d_want = torch.from_numpy(want.view(np.int32)).cuda()
    for mode in MODES:
        ref = base.gpu.search_batch_by_label(Q, k, 64, want, mode, 1500)
        for bare in (False, True):
            d_keys = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
            d_dist = None if bare else torch.zeros((nq, k), dtype=torch.float32, device="cuda")
            d_cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
            d_route = None if bare else torch.full((nq,), 9, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            base.gpu.search_batch_by_label_device(d_Q.data_ptr(), nq, k, 64, d_want.data_ptr(), d_keys.data_ptr(),
                                                  None if bare else d_dist.data_ptr(), d_cnt.data_ptr(),
                                                  None if bare else d_route.data_ptr(), mode, 1500)
            assert np.array_equal(d_keys.cpu().numpy(), ref[0]), mode
            assert np.array_equal(d_cnt.cpu().numpy().astype(np.uint32), ref[2]), mode
            if not bare:
                assert np.array_equal(d_dist.cpu().numpy().view(np.uint32), ref[1].view(np.uint32)), mode
                assert np.array_equal(d_route.cpu().numpy(), ref[3]), mode
    # labels written from device memory: the same column
    other = gc.gpu_index(base.dim, base.metric)
    d_labels = torch.from_numpy(base.labels.view(np.int32)).cuda()
    torch.cuda.synchronize()
    other.set_labels_device(0, d_labels.data_ptr(), len(base.labels))
    assert other.labelled_rows() == len(base.labels)


# ------------------------------------------------------------------------------------------------- 4. lifecycle
def test_lifecycle():
    n, dim, nq = 3000, 16, 24
    rng = np.random.default_rng(1770)
    X, Q = gc.make_data(n + 400, dim, "l2sq", 1771, nq=nq)
    keys = keys_against_slot_order(n, 5000)            # ids 2001 .. 5000
    new_keys = np.arange(400, dtype=np.int64) + 100    # the rows added later: ids 100 .. 499, labelled from the start
    labels = rng.integers(0, 5, 5001).astype(np.uint32)
    labels[rng.choice(5001, 50, replace=False)] = NO_LABEL
    want = (np.arange(nq) % 6).astype(np.uint32)       # tenant 5 does not exist (yet)
    gpu = build(dim, "l2sq", X[:n], keys, capacity=n + 400, M=8, M0=16, efc=32)
    before = gpu.memory_usage()
    gpu.set_labels(0, labels)
    column = gpu.memory_usage() - before
    assert 4 * len(labels) <= column <= 6 * len(labels)  # the column's bytes (it grows by halves)
    check(gpu, Q, 10, 64, labels, want, 100, "built")
    # rows removed, rows added into their slots, compaction: the column is by row id and needs no call
    gone = rng.choice(n, 700, replace=False)
    assert gpu.remove(keys[gone]) == 700
    check(gpu, Q, 10, 64, labels, want, 100, "700 removed")
    gpu.add(new_keys, X[n:])
    got = check(gpu, Q, 10, 64, labels, want, 100, "400 added into reused slots")
    assert np.any(np.isin(got["exact"][0][0], new_keys))
    gpu.compact()
    check(gpu, Q, 10, 64, labels, want, 100, "compacted")
    # a range overwritten: the answers follow
    labels[2500:3500] = 5
    gpu.set_labels(2500, labels[2500:3500])
    got = check(gpu, Q, 10, 64, labels, want, 100, "overwritten")
    assert np.all(got["exact"][0][2][want == 5] == 10)
    # grown past the end, skipping a gap: the gap holds NO_LABEL
    gpu.set_labels(6000, np.full(10, 3, dtype=np.uint32))
    labels = np.concatenate([labels, np.full(6000 - 5001, NO_LABEL, np.uint32), np.full(10, 3, np.uint32)])
    assert gpu.labelled_rows() == 6010
    check(gpu, Q, 10, 64, labels, want, 100, "grown", modes=("exact", "auto"))
    gpu.set_labels(123, np.zeros(0, dtype=np.uint32))  # n == 0: a no-op
    assert gpu.labelled_rows() == 6010
    # cleared: the search is an error that says so, and the bytes are back
    gpu.clear_labels()
    assert gpu.labelled_rows() == 0
    with pytest.raises(gc.pkg().VssError, match="no label column"):
        gpu.search_batch_by_label(Q, 10, 64, want)
    # vss_load clears the column
    gpu.set_labels(0, labels)
    gpu.load(gpu.save())
    assert gpu.labelled_rows() == 0
    with pytest.raises(gc.pkg().VssError, match="no label column"):
        gpu.search_batch_by_label(Q, 10, 64, want, "exact")
    gpu.set_labels(0, labels)
    check(gpu, Q, 10, 64, labels, want, 100, "loaded and labelled again", modes=("auto",))


def test_memory_usage_returns_after_clear():
    gpu = gc.gpu_index(8, "l2sq")
    before = gpu.memory_usage()
    gpu.set_labels(1000, np.arange(24, dtype=np.uint32))
    assert gpu.labelled_rows() == 1024 and gpu.memory_usage() - before >= 4 * 1024
    gpu.clear_labels()
    assert gpu.memory_usage() == before


# ------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals(base):
    import torch
    g, Q = base.gpu, base.Q[:4]
    want = np.zeros(4, dtype=np.uint32)
    err = gc.pkg().VssError
    for mode in (3, -1, 255):
        with pytest.raises(err, match="mode"):
            g.search_batch_by_label(Q, 10, 64, want, mode)
    bare = gc.gpu_index(base.dim, base.metric)
    for mode in MODES:
        with pytest.raises(err, match="no label column"):
            bare.search_batch_by_label(Q, 10, 64, want, mode)
    with pytest.raises(err, match="mode"):  # the mode is refused first
        bare.search_batch_by_label(Q, 10, 64, want, 7)
    # first_rowid + n beyond 2^32 (2^32 itself would be a column of 16 GiB: held to the CPU check)
    rows = g.labelled_rows()
    with pytest.raises(err, match="2\\^32"):
        g.set_labels(2 ** 32 - 1, np.zeros(2, dtype=np.uint32))
    with pytest.raises(err, match="2\\^32"):
        g.set_labels(2 ** 32 + 5, np.zeros(1, dtype=np.uint32))
    assert g.labelled_rows() == rows
    # a mutating call while a _begin context is open
    d_Q = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    d_keys = torch.zeros((4, 10), dtype=torch.int64, device="cuda")
    d_dist = torch.zeros((4, 10), dtype=torch.float32, device="cuda")
    d_cnt = torch.zeros((4,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g.search_begin(1, d_Q.data_ptr(), 4, 10, 64, d_keys.data_ptr(), d_dist.data_ptr(), d_cnt.data_ptr())
    try:
        with pytest.raises(err, match="still has a batch in flight"):
            g.set_labels(0, np.zeros(3, dtype=np.uint32))
        with pytest.raises(err, match="still has a batch in flight"):
            g.clear_labels()
    finally:
        g.search_end(1)
    assert g.labelled_rows() == rows
    base.check(Q, 10, 64, want, 1500, "after the refusals", modes=("auto",))


# ------------------------------------------------------------------------------------------------- 6. one staging path
def test_call_kinds_share_one_leased_context():
    """The host-pointer forms of four call kinds stage through the same leased context (a serial caller always leases the first
    free one), whose buffers are reused: group numbers and wanted labels land in the SAME cells, bitmaps next to them.  Seven calls
    of alternating kinds at growing and shrinking batch sizes; every answer — ids, distance bits, counts, routes — is that of the
    _device form of the same call on freshly uploaded tensors, which stages nothing.  Group g of the table is never label g: a
    staged cell that still held the previous call's kind of word would name another predicate."""
    import torch
    n, dim, k, ef, route_c = 3000, 32, 10, 64, 100
    X, Q = gc.make_data(n, dim, "l2sq", 1780, nq=257)
    keys = np.arange(n, dtype=np.int64)
    gpu = build(dim, "l2sq", X, keys)
    assert gpu.remove(keys[4::9]) == len(keys[4::9])
    labels = np.where(keys % 2 == 0, 100, keys % 16).astype(np.uint32)
    gpu.set_labels(0, labels)
    values = np.concatenate([[100], np.arange(16)]).astype(np.uint32)  # group 0: half the rows; the even values: nobody
    bitmaps = np.stack([_bitmap(n, np.nonzero(labels == v)[0]) for v in values])
    assert bitmaps.shape[0] == 17

    def dev(a, as_type):
        return torch.from_numpy(np.ascontiguousarray(a).view(as_type)).cuda()

    def on_device(call, nq, routed):
        d_keys = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
        d_dist = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        d_cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
        d_route = torch.full((nq,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        call(d_keys.data_ptr(), d_dist.data_ptr(), d_cnt.data_ptr(), d_route.data_ptr())
        out = (d_keys.cpu().numpy(), d_dist.cpu().numpy(), d_cnt.cpu().numpy().astype(np.uint32))
        return out + ((d_route.cpu().numpy(),) if routed else ())

    both_routes = False
    for nq in (65, 7, 257, 7):
        rng = np.random.default_rng(1781 + nq)
        group_of = rng.integers(0, 17, nq).astype(np.uint32)
        want = values[group_of]
        q = Q[:nq]

        def by_label(mode):
            d_q, d_want = dev(q, np.float32), dev(want, np.int32)
            return (gpu.search_batch_by_label(q, k, ef, want, mode, route_c),
                    on_device(lambda ids, dist, cnt, route: gpu.search_batch_by_label_device(
                        d_q.data_ptr(), nq, k, ef, d_want.data_ptr(), ids, dist, cnt, route, mode, route_c), nq, True))

        def groups_auto():
            d_q, d_tables, d_groups = dev(q, np.float32), dev(bitmaps, np.int64), dev(group_of, np.int32)
            return (gpu.search_batch_filtered_groups_auto(q, k, ef, bitmaps, n, group_of, route_c),
                    on_device(lambda ids, dist, cnt, route: gpu.search_batch_filtered_groups_auto_device(
                        d_q.data_ptr(), nq, k, ef, d_tables.data_ptr(), 17, n, d_groups.data_ptr(), ids, dist, cnt, route, route_c),
                        nq, True))

        def groups_exact_bitmap_0():
            d_q, d_tables = dev(q, np.float32), dev(bitmaps, np.int64)
            return (gpu.search_exact_batch_filtered_groups(q, k, bitmaps, n, None),
                    on_device(lambda ids, dist, cnt, route: gpu.search_exact_batch_filtered_groups_device(
                        d_q.data_ptr(), nq, k, d_tables.data_ptr(), 17, n, None, ids, dist, cnt), nq, False))

        def groups_graph():
            d_q, d_tables, d_groups = dev(q, np.float32), dev(bitmaps, np.int64), dev(group_of, np.int32)
            return (gpu.search_batch_filtered_groups(q, k, ef, bitmaps, n, group_of),
                    on_device(lambda ids, dist, cnt, route: gpu.search_batch_filtered_groups_device(
                        d_q.data_ptr(), nq, k, ef, d_tables.data_ptr(), 17, n, d_groups.data_ptr(), ids, dist, cnt), nq, False))

        calls = [("by label, auto", lambda: by_label("auto")), ("groups, auto", groups_auto),
                 ("groups, exact, bitmap 0", groups_exact_bitmap_0), ("by label, exact", lambda: by_label("exact")),
                 ("groups, graph", groups_graph), ("by label, graph", lambda: by_label("graph")),
                 ("by label, auto again", lambda: by_label("auto"))]
        for name, call in calls:
            where = "%d queries, %s" % (nq, name)
            host, device = call()
            assert len(host) == len(device), where
            assert_same(host[:3], device[:3], where)
            if len(host) == 4:
                assert np.array_equal(host[3], device[3]), where + ": routes"
                both_routes |= name == "by label, auto" and set(host[3]) == {0, 1}
    assert both_routes  # (len^2 <= route_c * live rows: the eight small tenants are scanned, tenant 100 is walked)
