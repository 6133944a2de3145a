"""-m gpu: vss_search_batch_by_label_range — per-query inclusive ranges over the index's resident label column
(csrc/label_filter.h; the walkers' admission in csrc/hnsw_kernels.h, the listing kernels in csrc/exact_filtered_kernels.h).

Contract, and the only yardstick here: let p_0 < p_1 < ... be the distinct RAW pairs (lo[q], hi[q]) of the call, ascending
lexicographically (nothing canonicalised: two different empty pairs are two groups), bitmap g have bit r set iff
r < labelled_rows, labels[r] != NO_LABEL and lo_g <= labels[r] <= hi_g as unsigned values, and group_of[q] be the index of query
q's pair.  Then the call in mode graph / exact / auto returns cell for cell — row ids, f32 distance bits, counts, routes — what
vss_search_batch_filtered_groups / vss_search_exact_batch_filtered_groups / vss_search_batch_filtered_groups_auto return for
that table, and leaves the same counters behind.  No tolerance, no cell left out.  (The bitmap calls' own answers are held to
a CPU brute force in tests/test_gpu_exact_filtered.py, test_gpu_filter_groups.py and test_gpu_filter_route.py.)
"""
import numpy as np
import pytest

import gpu_common as gc
from test_gpu_exact_filtered import _bitmap, _words, assert_same, keys_against_slot_order
from test_gpu_label_search import MODES, NO_LABEL, assert_nothing, bitmap_call, build, counters

pytestmark = pytest.mark.gpu

TOP = 0xFFFFFFFF  # as hi: no upper bound


def derived_table(labels, lo, hi):
    """the table of the contract: (bitmaps, n_bits, group_of), and the pairs"""
    labels = np.asarray(labels, dtype=np.uint64)
    packed = (np.asarray(lo, dtype=np.uint64) << np.uint64(32)) | np.asarray(hi, dtype=np.uint64)  # ascending = lexicographic
    pairs, group_of = np.unique(packed, return_inverse=True)
    n_bits = len(labels)
    bitmaps = np.zeros((len(pairs), _words(n_bits)), dtype=np.uint64)
    for g, p in enumerate(pairs):
        g_lo, g_hi = p >> np.uint64(32), p & np.uint64(0xFFFFFFFF)
        bitmaps[g] = _bitmap(n_bits, np.nonzero((labels != NO_LABEL) & (g_lo <= labels) & (labels <= g_hi))[0])
    return (bitmaps, n_bits, group_of.astype(np.uint32)), pairs


def check(gpu, Q, k, ef, labels, lo, hi, route_c, what, modes=MODES):
    """every mode against the bitmap call of that mode on the derived table: answers, routes, counters.  Returns
    {mode: (the by-range answer, the bitmap call's counters)}"""
    assert gpu.labelled_rows() == len(labels), what
    lo, hi = np.asarray(lo, dtype=np.uint32), np.asarray(hi, dtype=np.uint32)
    table, _ = derived_table(labels, lo, hi)
    out = {}
    for mode in modes:
        where = "%s, mode %s, route_c %d" % (what, mode, route_c)
        ref = bitmap_call(gpu, mode, Q, k, ef, table, route_c)
        ref_counters = counters(gpu, mode)
        got = gpu.search_batch_by_label_range(Q, k, ef, lo, hi, mode, route_c)
        got_counters = counters(gpu, mode)
        assert_same(got[:3], ref[:3], where)
        assert np.array_equal(got[3], ref[3]), where + ": routes"
        assert got_counters == ref_counters, where + ": counters %r, the bitmap call's %r" % (got_counters, ref_counters)
        out[mode] = (got, ref_counters)
    return out


def live_lengths(labels, keys, lo, hi):
    """rows each query's range admits among the live row ids `keys` (NumPy's restatement of the rule)"""
    keys = keys[keys < len(labels)]
    mine = labels[keys].astype(np.uint64)
    mine = mine[mine != NO_LABEL]
    return np.array([int(((a <= mine) & (mine <= b)).sum()) for a, b in zip(lo.astype(np.uint64), hi.astype(np.uint64))])


# ------------------------------------------------------------------------------------------------- 1. the mixed chunk
@pytest.mark.parametrize("metric,dim", [("l2sq", 100), ("cosine", 100), ("ip", 100), ("l2sq", 3), ("l2sq", 768)])
def test_mixed_chunk(metric, dim):
    n, nq, labelled, k, ef = 6000, 37, 8000, 10, 64
    X, Q = gc.make_data(n, dim, metric, 1900 + dim, nq=nq)
    keys = keys_against_slot_order(n, 9000)  # row id != slot; row ids 3001 .. 9000, those from 8000 on without a cell
    rng = np.random.default_rng(19)
    labels = rng.integers(0, 10000, labelled).astype(np.uint32)
    labels[rng.choice(np.arange(3001, labelled), 20, replace=False)] = NO_LABEL
    v = int(labels[5000])
    assert v != NO_LABEL
    ranges = ([(0, 4999)] * 4 + [(1000, 1999)] * 3 + [(3000, 6000)] * 3 + [(5000, 8000)] * 3 + [(v, v)] * 2     # half, nested, two that overlap
              + [(0, TOP)] * 3 + [(TOP, TOP)] * 2 + [(9, 2)] * 2 + [(7000, 100)] * 2 + [(9000, TOP)] * 3         # all, NO_LABEL only, two empties
              + [(20000, 30000)] * 2 + [(2500, 2600)] * 3 + [(0, 0x7FFFFFFF), (0x80000000, TOP), (4000, 4100)]   # no row; narrow ones
              + [(1000, 1999), (0, 4999)])
    assert len(ranges) == nq
    ranges = np.array(ranges, dtype=np.uint32)[rng.permutation(nq)]
    lo, hi = np.ascontiguousarray(ranges[:, 0]), np.ascontiguousarray(ranges[:, 1])
    gpu = build(dim, metric, X, keys)
    gpu.set_labels(0, labels)
    what = "%s dim %d" % (metric, dim)
    lens = live_lengths(labels, keys, lo, hi)
    assert 2300 < lens[(lo == 0) & (hi == 4999)][0] < 2700 and lens[(lo == 0) & (hi == TOP)][0] == 4999 - 20
    got = check(gpu, Q, k, ef, labels, lo, hi, 0, what)
    nothing = (lo > hi) | (lo == TOP) | (lo == 20000) | (lo == 0x80000000)
    assert np.array_equal(nothing, lens == 0)
    for mode in MODES:
        assert_nothing(got[mode][0], nothing, what + " " + mode)
    assert np.array_equal(got["exact"][0][2], np.minimum(lens, k))  # the scan returns min(k, admitted live rows)
    # the rule (csrc/filter_route.h): a group is scanned iff len^2 * 64 <= C * limit * L, limit = max(k, ef), L = live rows
    limit, L = max(k, ef), n
    distinct = np.unique(lens[lens > 0])
    largest, second = int(distinct[-1]), int(distinct[-2])
    # ... a C between the two largest groups: the largest is walked, every other group scanned
    c_between = -(-second * second * 64 // (limit * L))
    assert second * second * 64 <= c_between * limit * L < largest * largest * 64
    route = check(gpu, Q, k, ef, labels, lo, hi, c_between, what, modes=("auto",))["auto"][0][3]
    assert set(route.tolist()) == {0, 1}
    assert np.array_equal(route, np.where(lens == largest, 0, 1))
    # ... and the largest group ON the boundary where an integer C puts it there, else the nearest C on each side
    num, den = largest * largest * 64, limit * L
    for c in ([num // den] if num % den == 0 else [num // den, num // den + 1]):
        route = check(gpu, Q, k, ef, labels, lo, hi, c, what, modes=("auto",))["auto"][0][3]
        assert np.array_equal(route, np.where(lens.astype(object) ** 2 * 64 <= c * den, 1, 0).astype(np.uint8)), c


# ------------------------------------------------------------------------------------------------- 2. equality
def test_equality_is_the_call_by_label():
    """lo = hi = want over the label tests' mixed labels: the answer and the counters of vss_search_batch_by_label"""
    from test_gpu_label_search import mixed_labels
    n, nq, labelled, dim = 6000, 37, 8000, 100
    X, Q = gc.make_data(n, dim, "l2sq", 1700 + dim, nq=nq)
    keys = keys_against_slot_order(n, 9000)
    rng = np.random.default_rng(17)
    labels = mixed_labels(keys, labelled, rng)
    want = np.array([1] * 5 + [2] * 6 + [10, 11, 11, 12, 13, 14, 15] * 2 + [100, 101, 102, 103, 104] + [NO_LABEL, 7, 4_000_000_000]
                    + [1, 2, 10, 100], dtype=np.uint32)[rng.permutation(nq)]
    gpu = build(dim, "l2sq", X, keys)
    gpu.set_labels(0, labels)
    for route_c in (1500, 1499, 3):
        for mode in MODES:
            where = "mode %s, route_c %d" % (mode, route_c)
            ref = gpu.search_batch_by_label(Q, 10, 64, want, mode, route_c)
            ref_counters = counters(gpu, mode)
            got = gpu.search_batch_by_label_range(Q, 10, 64, want, want, mode, route_c)
            assert_same(got[:3], ref[:3], where)
            assert np.array_equal(got[3], ref[3]), where + ": routes"
            assert counters(gpu, mode) == ref_counters, where
    check(gpu, Q, 10, 64, labels, want, want, 1499, "equality against the bitmaps")


# ------------------------------------------------------------------------------------------------- 3. listing edges
@pytest.mark.parametrize("n", [1, 511, 512, 513, 1025])  # FL_WAVE_SLOTS = 512
def test_listing_edges(n):
    """labels laid out BY SLOT (label = slot; a listing wave owns 512 consecutive slots, a row of it 64), so a range's ends name
    lanes: lanes 0 and 63, a whole row of 64, ranges across a row's edge and across the 512-slot block's, one of the last slot only"""
    dim = 8
    X, Q = gc.make_data(n, dim, "l2sq", 1910 + n, nq=24)
    keys = keys_against_slot_order(n, 2000)
    labels = np.full(2001, NO_LABEL, dtype=np.uint32)
    labels[keys] = np.arange(n, dtype=np.uint32)
    ranges = np.array([(0, 0), (63, 63), (0, 63), (64, 127), (63, 64), (1, 62), (448, 511), (511, 511), (511, 512), (512, 512),
                       (512, 575), (0, 511), (512, 1023), (1023, 1024), (1024, 1024), (n - 1, n - 1), (n - 1, TOP), (n, TOP),
                       (0, TOP), (5, 4), (TOP, 0), (100, 900), (0, n - 1), (0, 0)], dtype=np.uint32)
    lo, hi = np.ascontiguousarray(ranges[:, 0]), np.ascontiguousarray(ranges[:, 1])
    gpu = build(dim, "l2sq", X, keys, M=4, M0=8, efc=16)
    gpu.set_labels(0, labels)
    got = check(gpu, Q, 10, 64, labels, lo, hi, 1, "n %d" % n)
    cnt = got["exact"][0][2]
    expect = np.array([max(0, min(int(b), n - 1) - int(a) + 1) if a <= b else 0 for a, b in ranges])  # label = slot
    assert np.array_equal(cnt, np.minimum(expect, 10))
    last = got["exact"][0][0][15]
    assert cnt[15] == 1 and last[0] == keys[n - 1]  # the range of the last slot only: that row
    distinct = {(int(a), int(b)): e for (a, b), e in zip(ranges, expect)}
    assert got["exact"][1]["exact"][0] == sum(distinct.values())  # listed: every group's rows, overlaps counted per group


# ------------------------------------------------------------------------------------------------- 4. several passes
def test_overlapping_ranges_take_several_passes(monkeypatch):
    """ranges overlap, so the lists of one call can together exceed max(budget, rows) entries — which a partition by labels never
    does — and the plan packs them into several passes; as many as the bitmap call's"""
    n, dim, nq = 3000, 16, 24
    X, Q = gc.make_data(n, dim, "l2sq", 1930, nq=nq)
    keys = keys_against_slot_order(n, 5000)
    rng = np.random.default_rng(1931)
    labels = rng.integers(0, 12, 5001).astype(np.uint32)
    ranges = np.array([(0, 11), (0, 5), (3, 9), (6, 11), (0, TOP), (2, 10)] * 4, dtype=np.uint32)
    lo, hi = np.ascontiguousarray(ranges[:, 0]), np.ascontiguousarray(ranges[:, 1])
    monkeypatch.setenv("VSS_EXACT_FILTER_LIST_ENTRIES", "1000")
    gpu = build(dim, "l2sq", X, keys, M=4, M0=8, efc=16)
    gpu.set_labels(0, labels)
    got = check(gpu, Q, 10, 64, labels, lo, hi, 0, "budget 1000", modes=("exact", "auto"))
    listed, _, passes = got["exact"][1]["exact"]
    assert listed == live_lengths(labels, keys, lo[:6], hi[:6]).sum() > n and passes >= 2


# ------------------------------------------------------------------------------------------------- 5. kernel shapes
class Base:
    def __init__(self):
        self.metric, self.n, self.dim = "l2sq", 6000, 32
        self.X, self.Q = gc.make_data(self.n, self.dim, self.metric, 1740, nq=300)
        self.keys = keys_against_slot_order(self.n, 9000)
        rng = np.random.default_rng(1941)
        by_slot = rng.integers(0, 10000, self.n).astype(np.uint32)
        by_slot[rng.choice(self.n, 3, replace=False)] = NO_LABEL
        self.labels = np.full(9001, NO_LABEL, dtype=np.uint32)
        self.labels[self.keys] = by_slot
        self.sorted = np.sort(by_slot[by_slot != NO_LABEL])
        self.gpu = build(self.dim, self.metric, self.X, self.keys)
        self.gpu.set_labels(0, self.labels)

    def check(self, Q, k, ef, lo, hi, route_c, what, modes=MODES):
        return check(self.gpu, Q, k, ef, self.labels, lo, hi, route_c, what, modes)


@pytest.fixture(scope="module")
def base():
    return Base()


SEVEN = np.array([(0, 5999), (2000, 4499), (5000, 6199), (7000, 7499), (100, 109), (0, TOP), (10000, 20000)], dtype=np.uint32)


@pytest.mark.parametrize("ef", [64, 300, 600])  # lists in registers (2 and 8 per lane) and outside them
def test_list_widths(base, ef):
    ranges = SEVEN[np.arange(21) % 7]
    route_c = {64: 1000, 300: 300, 600: 160}[ef]  # len^2 * 64 <= route_c * limit * 6000 ends near 3000 rows at each limit
    got = base.check(base.Q[:21], 100, ef, ranges[:, 0], ranges[:, 1], route_c, "ef %d" % ef)
    assert (got["graph"][1]["shape"][4] != 0) == (ef == 600)  # beyond 512 the list has left the registers (the bitmap call's shape)
    route = got["auto"][0][3]
    wide = np.isin(np.arange(21) % 7, [0, 5])  # 3600 and 5997 rows are walked, 1500 and fewer scanned
    assert np.all(route[wide] == 0) and np.all(route[~wide] == 1)


def test_one_query_takes_the_solo_kernel():
    n, dim = 2000, 128
    X, Q = gc.make_data(n, dim, "l2sq", 1950, nq=4)
    keys = keys_against_slot_order(n, 3000)
    labels = (np.arange(3001) % 30).astype(np.uint32)
    gpu = build(dim, "l2sq", X, keys, M=8, M0=16, efc=32)
    gpu.set_labels(0, labels)
    for q, (a, b) in enumerate([(0, 9), (20, TOP)]):
        got = check(gpu, Q[q:q + 1], 10, 64, labels, [a], [b], 1, "one query")
        assert got["graph"][1]["shape"][6] == 1 and got["graph"][0][2][0] == 10


@pytest.mark.parametrize("nq", [204, 300])  # the join's chunk; more than a launch of one query per compute unit
def test_host_batches(base, nq):
    rng = np.random.default_rng(1960 + nq)
    lo = rng.integers(0, 9000, nq).astype(np.uint32)  # nearly every query its own range, of 0 to 8000 labels
    hi = (lo + rng.integers(0, 8000, nq) * (rng.integers(0, 4, nq) > 0)).astype(np.uint32)
    lo[::50], hi[::50] = 5, 1
    got = base.check(base.Q[:nq], 10, 64, lo, hi, 1500, "%d queries" % nq)
    assert set(got["auto"][0][3]) == {0, 1}


def test_rare_predicate_reruns(base):
    """ranges of six rows and of one: the walk rejects nearly every row it meets, its pending candidates outgrow the register
    queue, and the queries are re-run through the unbounded one — reading the same table of ranges again, through a.work[idx]"""
    s = base.sorted
    six, one = (int(s[1000]), int(s[1005])), (int(s[3000]), int(s[3000]))
    n_six, n_one = int(((s >= six[0]) & (s <= six[1])).sum()), int((s == one[0]).sum())
    assert 6 <= n_six <= 8 and 1 <= n_one <= 3
    ranges = np.array([six, one] * 8, dtype=np.uint32)
    got = base.check(base.Q[:16], 10, 64, ranges[:, 0], ranges[:, 1], 1500, "rare ranges", modes=("graph",))
    _, _, cnt, _ = got["graph"][0]
    assert np.all(cnt[0::2] <= n_six) and np.all(cnt[1::2] <= n_one) and cnt.sum() > 0  # (a walk may miss a row; it invents none)
    assert got["graph"][1]["stats"][3] > 0  # (the bitmap call's counter, and by check() this call's: queries were re-run)


def test_device_form(base):
    import torch
    nq, k = 35, 10
    Q = base.Q[:nq]
    ranges = SEVEN[np.arange(nq) % 7].copy()
    ranges[3] = (9, 2)
    lo, hi = np.ascontiguousarray(ranges[:, 0]), np.ascontiguousarray(ranges[:, 1])
    d_Q = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    d_lo, d_hi = torch.from_numpy(lo.view(np.int32)).cuda(), torch.from_numpy(hi.view(np.int32)).cuda()
    for mode in MODES:
        ref = base.check(Q, k, 64, lo, hi, 1500, "host form", modes=(mode,))[mode][0]
        for bare in (False, True):
            d_keys = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
            d_dist = None if bare else torch.zeros((nq, k), dtype=torch.float32, device="cuda")
            d_cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
            d_route = None if bare else torch.full((nq,), 9, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            base.gpu.search_batch_by_label_range_device(d_Q.data_ptr(), nq, k, 64, d_lo.data_ptr(), d_hi.data_ptr(), d_keys.data_ptr(),
                                                        None if bare else d_dist.data_ptr(), d_cnt.data_ptr(),
                                                        None if bare else d_route.data_ptr(), mode, 1500)
            assert np.array_equal(d_keys.cpu().numpy(), ref[0]), mode
            assert np.array_equal(d_cnt.cpu().numpy().astype(np.uint32), ref[2]), mode
            if not bare:
                assert np.array_equal(d_dist.cpu().numpy().view(np.uint32), ref[1].view(np.uint32)), mode
                assert np.array_equal(d_route.cpu().numpy(), ref[3]), mode


# ------------------------------------------------------------------------------------------------- 6. lifecycle
def test_lifecycle():
    n, dim, nq = 3000, 16, 24
    rng = np.random.default_rng(1970)
    X, Q = gc.make_data(n + 400, dim, "l2sq", 1971, nq=nq)
    keys = keys_against_slot_order(n, 5000)            # ids 2001 .. 5000
    new_keys = np.arange(400, dtype=np.int64) + 100    # the rows added later: ids 100 .. 499, labelled from the start
    labels = rng.integers(0, 1000, 5001).astype(np.uint32)
    labels[rng.choice(5001, 50, replace=False)] = NO_LABEL
    ranges = np.array([(0, 499), (100, 300), (250, 800), (900, TOP), (5000, 6000), (7, 7)] * 4, dtype=np.uint32)
    lo, hi = np.ascontiguousarray(ranges[:, 0]), np.ascontiguousarray(ranges[:, 1])
    gpu = build(dim, "l2sq", X[:n], keys, capacity=n + 400, M=8, M0=16, efc=32)
    gpu.set_labels(0, labels)
    got = check(gpu, Q, 10, 64, labels, lo, hi, 100, "built")
    assert np.all(got["exact"][0][2][lo == 5000] == 0)  # no row carries a label from 5000 on (yet)
    # rows removed, rows added into their slots, compaction: the column is by row id and needs no call
    gone = rng.choice(n, 700, replace=False)
    assert gpu.remove(keys[gone]) == 700
    check(gpu, Q, 10, 64, labels, lo, hi, 100, "700 removed")
    gpu.add(new_keys, X[n:])
    got = check(gpu, Q, 10, 64, labels, lo, hi, 100, "400 added into reused slots")
    assert np.any(np.isin(got["exact"][0][0], new_keys))
    gpu.compact()
    check(gpu, Q, 10, 64, labels, lo, hi, 100, "compacted")
    # cells overwritten: the answers follow the column by row id
    labels[2500:3500] = 5500
    gpu.set_labels(2500, labels[2500:3500])
    got = check(gpu, Q, 10, 64, labels, lo, hi, 100, "overwritten")
    assert np.all(got["exact"][0][2][lo == 5000] == 10)
    assert np.all((got["exact"][0][0][lo == 5000] >= 2500) & (got["exact"][0][0][lo == 5000] < 3500))
    gpu.clear_labels()
    with pytest.raises(gc.pkg().VssError, match="no label column"):
        gpu.search_batch_by_label_range(Q, 10, 64, lo, hi)
    gpu.set_labels(0, labels)
    check(gpu, Q, 10, 64, labels, lo, hi, 100, "cleared and labelled again", modes=("auto",))


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(base):
    g, Q = base.gpu, base.Q[:4]
    lo, hi = np.zeros(4, dtype=np.uint32), np.full(4, 5000, dtype=np.uint32)
    err = gc.pkg().VssError
    for mode in (3, -1, 255):
        with pytest.raises(err, match="mode"):
            g.search_batch_by_label_range(Q, 10, 64, lo, hi, mode)
    bare = gc.gpu_index(base.dim, base.metric)
    for mode in MODES:
        with pytest.raises(err, match="no label column"):
            bare.search_batch_by_label_range(Q, 10, 64, lo, hi, mode)
    with pytest.raises(err, match="mode"):  # the mode is refused first
        bare.search_batch_by_label_range(Q, 10, 64, lo, hi, 3)
    # NULL lo / hi with queries to answer, through the C entry point itself; without queries the call has nothing to read
    out = np.full((4, 10), -1, dtype=np.int64)
    cnt = np.zeros(4, dtype=np.uint32)
    for p_lo, p_hi in ((None, hi.ctypes.data), (lo.ctypes.data, None), (None, None)):
        for mode in (0, 1, 2):
            assert g.lib.vss_search_batch_by_label_range(g.h, Q.ctypes.data, 4, 10, 64, p_lo, p_hi, mode, 0, out.ctypes.data, None,
                                                         cnt.ctypes.data, None) != 0
            assert b"null lo / hi" in g.lib.vss_last_error(g.h)
    assert g.lib.vss_search_batch_by_label_range(g.h, Q.ctypes.data, 0, 10, 64, None, None, 2, 0, out.ctypes.data, None,
                                                 cnt.ctypes.data, None) == 0
    assert g.lib.vss_search_batch_by_label_range(g.h, Q.ctypes.data, 4, 0, 64, lo.ctypes.data, hi.ctypes.data, 2, 0, out.ctypes.data,
                                                 None, cnt.ctypes.data, None) == 0
    assert np.all(out == -1) and np.all(cnt == 0)  # nothing was written by any of them
    base.check(Q, 10, 64, lo, hi, 1500, "after the refusals")
