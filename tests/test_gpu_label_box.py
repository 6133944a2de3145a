"""-m gpu: vss_search_batch_by_label_box — per-query conjunctions of inclusive ranges over up to four resident label columns
(csrc/label_filter.h; the walkers' admission in csrc/hnsw_kernels.h, the listing kernels in csrc/exact_filtered_kernels.h).

Contract, and the only yardstick here: form the n_queries x 2m matrix whose row q is (lo[q,0], hi[q,0], lo[q,1], hi[q,1], ...).
Let b_0 < b_1 < ... be its distinct RAW rows, ascending lexicographically as unsigned words (nothing canonicalised: two different
empty boxes are two groups), bitmap g have bit r set iff for every named column c_j: r < rows(c_j), cell[r] != NO_LABEL and
lo_j <= cell[r] <= hi_j, n_bits be the smallest rows(c_j), and group_of[q] be the index of query q's row.  Then the call in mode
graph / exact / auto returns cell for cell — row ids, f32 distance bits, counts, routes — what vss_search_batch_filtered_groups /
vss_search_exact_batch_filtered_groups / vss_search_batch_filtered_groups_auto return for that table, and leaves the same
counters behind.  No tolerance, no cell left out.
"""
import numpy as np
import pytest

import gpu_common as gc
from test_gpu_exact_filtered import _bitmap, _words, assert_same, keys_against_slot_order
from test_gpu_label_search import MODES, NO_LABEL, assert_nothing, bitmap_call, build, counters

pytestmark = pytest.mark.gpu

TOP = 0xFFFFFFFF  # as hi: no upper bound


def matrix(boxes):
    """[(lo_0, hi_0, lo_1, hi_1, ...), ...] -> the call's lo and hi matrices"""
    boxes = np.asarray(boxes, dtype=np.uint32)
    return np.ascontiguousarray(boxes[:, 0::2]), np.ascontiguousarray(boxes[:, 1::2])


def admitted(cols, columns, lo_row, hi_row):
    """NumPy's restatement of the rule: the mask over row ids below the shortest named column"""
    n_bits = min(len(cols[c]) for c in columns)
    mask = np.ones(n_bits, dtype=bool)
    for c, a, b in zip(columns, lo_row, hi_row):
        cell = cols[c][:n_bits].astype(np.uint64)
        mask &= (cell != NO_LABEL) & (np.uint64(a) <= cell) & (cell <= np.uint64(b))
    return mask


def derived_table(cols, columns, lo, hi):
    """the table of the contract: (bitmaps, n_bits, group_of)"""
    rows = np.empty((len(lo), 2 * len(columns)), dtype=np.uint32)
    rows[:, 0::2], rows[:, 1::2] = lo, hi
    groups, group_of = np.unique(rows, axis=0, return_inverse=True)  # rows ascending lexicographically, as unsigned words
    n_bits = min(len(cols[c]) for c in columns)
    bitmaps = np.zeros((len(groups), _words(n_bits)), dtype=np.uint64)
    for g, row in enumerate(groups):
        bitmaps[g] = _bitmap(n_bits, np.nonzero(admitted(cols, columns, row[0::2], row[1::2]))[0])
    return bitmaps, n_bits, group_of.reshape(-1).astype(np.uint32)


def check(gpu, Q, k, ef, cols, columns, lo, hi, route_c, what, modes=MODES):
    """every mode against the bitmap call of that mode on the derived table: answers, routes, counters.  Returns
    {mode: (the by-box answer, the bitmap call's counters)}"""
    for c in columns:
        assert gpu.label_column_rows(c) == len(cols[c]), what
    lo, hi = np.asarray(lo, dtype=np.uint32).reshape(len(Q), -1), np.asarray(hi, dtype=np.uint32).reshape(len(Q), -1)
    table = derived_table(cols, columns, lo, hi)
    out = {}
    for mode in modes:
        where = "%s, columns %r, mode %s, route_c %d" % (what, list(columns), mode, route_c)
        ref = bitmap_call(gpu, mode, Q, k, ef, table, route_c)
        ref_counters = counters(gpu, mode)
        got = gpu.search_batch_by_label_box(Q, k, ef, columns, lo, hi, mode, route_c)
        got_counters = counters(gpu, mode)
        assert_same(got[:3], ref[:3], where)
        assert np.array_equal(got[3], ref[3]), where + ": routes"
        assert got_counters == ref_counters, where + ": counters %r, the bitmap call's %r" % (got_counters, ref_counters)
        out[mode] = (got, ref_counters)
    return out


def live_lengths(cols, columns, keys, lo, hi):
    """rows each query's box admits among the live row ids `keys`"""
    n_bits = min(len(cols[c]) for c in columns)
    live = np.zeros(n_bits, dtype=bool)
    live[keys[keys < n_bits]] = True
    return np.array([int((admitted(cols, columns, a, b) & live).sum()) for a, b in zip(lo, hi)])


# ------------------------------------------------------------------------------------------------- 1. the mixed chunk
def mixed_chunk():
    """two columns of different length by row id — column 1 a tenant of 12 values with skewed shares over 8000 cells, column 3 a
    timestamp uniform in [0, 10000) over 7000 — about 20 NO_LABEL cells in each at different live rows, and the 37 boxes"""
    n, nq = 6000, 37
    keys = keys_against_slot_order(n, 9000)  # row id != slot; row ids 3001 .. 9000: from 7000 on no timestamp, from 8000 on no tenant
    rng = np.random.default_rng(21)
    shares = [.62, .13, .06, .05, .04, .03, .02, .015, .015, .01, .005, .005]
    tenant = rng.choice(12, 8000, p=shares).astype(np.uint32)
    ts = rng.integers(0, 10000, 7000).astype(np.uint32)
    ts[:7000][tenant[:7000] == 11] %= 5000  # tenant 11 has no row after 5000
    nulls = rng.choice(np.arange(3001, 7000), 40, replace=False)
    tenant[nulls[:20]] = NO_LABEL
    ts[nulls[20:]] = NO_LABEL
    cols = {1: tenant, 3: ts}
    boxes = ([(0, 0, 0, 4999)] * 3 + [(0, 0, 1000, 1999)] * 2 + [(0, 0, 3000, 6000)] * 2 + [(0, 0, 5000, 8000)] * 2  # tenant = x half, nested, overlapping
             + [(0, 0, 0, TOP)] * 3 + [(0, 0, 0, 0x7FFFFFFF)]                                                     # the largest, twice over
             + [(1, 5, 0, TOP)] * 3 + [(2, 11, 0, TOP)] * 2 + [(2, 2, 0, TOP)] * 2                                # tenant range x everything
             + [(1, 1, 0, 4999)] * 2 + [(1, 1, 2000, 2999)]
             + [(9, 2, 0, TOP)] * 2 + [(0, 0, 7000, 100)] * 2 + [(5, 4, 3, 2)]                                    # empty through column 1 only, column 3 only, both
             + [(11, 11, 9000, 9999)] * 2                                                                         # each clause has rows, the box none
             + [(TOP, TOP, 0, TOP), (0x80000000, TOP, 0, TOP)]                                                    # NO_LABEL only; no such tenant
             + [(3, 3, 2500, 3499)] * 2 + [(0, 11, 4000, 4100)]                                                   # narrow ones
             + [(0, 0, 1000, 1999), (0, 0, 0, 4999)])                                                             # repeats
    assert len(boxes) == nq
    boxes = np.array(boxes, dtype=np.uint32)[rng.permutation(nq)]
    lo, hi = matrix(boxes)
    return keys, cols, lo, hi


@pytest.mark.parametrize("metric,dim", [("l2sq", 100), ("cosine", 100), ("ip", 100), ("l2sq", 3), ("l2sq", 768)])
def test_mixed_chunk(metric, dim):
    n, nq, k, ef = 6000, 37, 10, 64
    columns = [1, 3]
    keys, cols, lo, hi = mixed_chunk()
    # on the NumPy restatement, before any GPU call
    lens = live_lengths(cols, columns, keys, lo, hi)
    assert 2300 <= lens.max() <= 2700
    nothing = (np.any(lo > hi, axis=1) | (lo[:, 0] == TOP) | (lo[:, 0] == 0x80000000) | ((lo[:, 0] == 11) & (lo[:, 1] == 9000)))
    assert np.array_equal(nothing, lens == 0)
    each_alone = live_lengths(cols, [1], keys, [[11]], [[11]])[0] > 0 and live_lengths(cols, [3], keys, [[9000]], [[9999]])[0] > 0
    assert each_alone  # ... although each clause of that box alone has rows
    X, Q = gc.make_data(n, dim, metric, 2100 + dim, nq=nq)
    gpu = build(dim, metric, X, keys)
    gpu.set_label_column(1, 0, cols[1])
    gpu.set_label_column(3, 0, cols[3])
    what = "%s dim %d" % (metric, dim)
    got = check(gpu, Q, k, ef, cols, columns, lo, hi, 0, what)
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
    route = check(gpu, Q, k, ef, cols, columns, lo, hi, c_between, what, modes=("auto",))["auto"][0][3]
    assert set(route.tolist()) == {0, 1}
    assert np.array_equal(route, np.where(lens == largest, 0, 1))
    # ... and the largest group ON the boundary where an integer C puts it there, else the nearest C on each side
    num, den = largest * largest * 64, limit * L
    for c in ([num // den] if num % den == 0 else [num // den, num // den + 1]):
        route = check(gpu, Q, k, ef, cols, columns, lo, hi, c, what, modes=("auto",))["auto"][0][3]
        assert np.array_equal(route, np.where(lens.astype(object) ** 2 * 64 <= c * den, 1, 0).astype(np.uint8)), c


# ------------------------------------------------------------------------------------------------- 2. one column
def test_one_column_is_the_range_call():
    """columns = {0}: the answers and counters of vss_search_batch_by_label_range.  columns = {2}: the derived table.  Four named
    columns, three of them under [0, TOP]: the one-column call on the fourth where those three have a label in every live row, and
    without the rows where one of them has a NO_LABEL cell or no cell at all"""
    n, nq, dim, k = 6000, 37, 100, 10
    X, Q = gc.make_data(n, dim, "l2sq", 2200, nq=nq)
    keys = keys_against_slot_order(n, 9000)
    rng = np.random.default_rng(22)
    cols = {0: rng.integers(0, 10000, 8000).astype(np.uint32)}
    cols[0][rng.choice(np.arange(3001, 8000), 20, replace=False)] = NO_LABEL
    for c in (1, 2, 3):  # a label in every cell, and as many cells as column 0
        cols[c] = rng.integers(0, 50, 8000).astype(np.uint32)
    ranges = np.array(([(0, 4999)] * 5 + [(1000, 1999)] * 4 + [(3000, 6000)] * 4 + [(0, TOP)] * 4 + [(9, 2)] * 3 + [(7000, 100)] * 2
                       + [(TOP, TOP)] * 2 + [(2500, 2600)] * 4 + [(9000, TOP)] * 4 + [(20000, 30000)] * 2 + [(4000, 4100)] * 3),
                      dtype=np.uint32)[rng.permutation(nq)]
    lo, hi = np.ascontiguousarray(ranges[:, :1]), np.ascontiguousarray(ranges[:, 1:])
    gpu = build(dim, "l2sq", X, keys)
    gpu.set_labels(0, cols[0])  # column 0 is the column of set_labels
    for c in (1, 2, 3):
        gpu.set_label_column(c, 0, cols[c])
    assert gpu.labelled_rows() == gpu.label_column_rows(0) == 8000
    for route_c in (1500, 3):
        for mode in MODES:
            where = "mode %s, route_c %d" % (mode, route_c)
            ref = gpu.search_batch_by_label_range(Q, k, 64, lo[:, 0], hi[:, 0], mode, route_c)
            ref_counters = counters(gpu, mode)
            got = gpu.search_batch_by_label_box(Q, k, 64, [0], lo, hi, mode, route_c)
            assert_same(got[:3], ref[:3], where)
            assert np.array_equal(got[3], ref[3]), where + ": routes"
            assert counters(gpu, mode) == ref_counters, where
    check(gpu, Q, k, 64, cols, [0], lo, hi, 1500, "column 0 against the bitmaps")
    lo2, hi2 = lo // 200, np.where(hi == TOP, TOP, hi // 200).astype(np.uint32)  # (column 2 holds 0 .. 49)
    check(gpu, Q, k, 64, cols, [2], lo2, hi2, 1500, "column 2 alone")
    # four named columns, the other three unconstrained but for their NULLs: there are none, and the answer is the one-column call's
    four = [1, 0, 3, 2]
    lo4, hi4 = np.zeros((nq, 4), dtype=np.uint32), np.full((nq, 4), TOP, dtype=np.uint32)
    lo4[:, 1], hi4[:, 1] = lo[:, 0], hi[:, 0]
    got = check(gpu, Q, k, 64, cols, four, lo4, hi4, 1500, "four columns, three full")
    for mode in MODES:
        one = gpu.search_batch_by_label_range(Q, k, 64, lo[:, 0], hi[:, 0], mode, 1500)
        assert_same(got[mode][0][:3], one[:3], "four columns, three full, against the one column: " + mode)
        assert np.array_equal(got[mode][0][3], one[3])
    # ... now column 3 ends at row id 6999 and column 1 has NO_LABEL in rows the one-column answer names: those rows are absent
    one = gpu.search_batch_by_label_range(Q, k, 64, lo[:, 0], hi[:, 0], "exact")
    named = np.unique(one[0][one[0] >= 0])
    nulled = named[named < 7000][::3]
    assert len(nulled) > 10 and np.any(named >= 7000)
    cols[1] = cols[1].copy()
    cols[1][nulled] = NO_LABEL
    cols[3] = cols[3][:7000]
    gpu.set_label_column(1, 0, cols[1])
    gpu.clear_label_column(3)
    gpu.set_label_column(3, 0, cols[3])
    got = check(gpu, Q, k, 64, cols, four, lo4, hi4, 1500, "four columns, one short, one with NULLs")
    ids = got["exact"][0][0]
    assert not np.any(np.isin(ids, nulled)) and not np.any(ids >= 7000) and np.any(ids >= 0)
    absent = np.isin(one[0], nulled) | (one[0] >= 7000)
    assert np.any(absent)
    for q in range(nq):  # what the one column admits and the other three do not reject stays, in the scan's order
        kept = one[0][q][~absent[q] & (one[0][q] >= 0)]
        assert np.array_equal(ids[q][:len(kept)], kept), q


# ------------------------------------------------------------------------------------------------- 3. column order
def test_column_order_changes_no_answer():
    n, k, ef = 6000, 10, 64
    keys, cols, lo, hi = mixed_chunk()
    X, Q = gc.make_data(n, 32, "l2sq", 2300, nq=len(lo))
    gpu = build(32, "l2sq", X, keys)
    gpu.set_label_column(1, 0, cols[1])
    gpu.set_label_column(3, 0, cols[3])
    for mode in MODES:
        a = gpu.search_batch_by_label_box(Q, k, ef, [1, 3], lo, hi, mode, 300)
        b = gpu.search_batch_by_label_box(Q, k, ef, [3, 1], lo[:, ::-1], hi[:, ::-1], mode, 300)
        assert_same(a[:3], b[:3], "columns swapped, mode " + mode)
        assert np.array_equal(a[3], b[3]), mode
    assert set(a[3].tolist()) == {0, 1}  # (mode auto took both roads)


# ------------------------------------------------------------------------------------------------- 4. listing edges
@pytest.mark.parametrize("n", [1, 511, 512, 513, 1025])  # FL_WAVE_SLOTS = 512
def test_listing_edges(n):
    """column 1's label is the SLOT and column 2's the slot modulo 64 (a listing wave owns 512 consecutive slots, a row of it 64), so
    a box's ends name lanes: lanes 0 and 63 of every row, a whole row of 64, runs across a row's edge and across the 512-slot
    block's, the last slot only"""
    dim = 8
    X, Q = gc.make_data(n, dim, "l2sq", 2400 + n, nq=26)
    keys = keys_against_slot_order(n, 2000)
    slot = np.arange(n, dtype=np.uint32)
    cols = {1: np.full(2001, NO_LABEL, dtype=np.uint32), 2: np.full(2001, NO_LABEL, dtype=np.uint32)}
    cols[1][keys], cols[2][keys] = slot, slot % 64
    boxes = np.array([(0, TOP, 0, 0), (0, TOP, 63, 63), (0, 511, 63, 63), (64, 127, 0, 63), (64, 127, 0, TOP), (60, 70, 0, 63),
                      (60, 70, 60, 63), (60, 70, 0, 6), (448, 511, 0, 63), (511, 511, 63, 63), (511, 512, 0, TOP), (512, 512, 0, 0),
                      (500, 530, 10, 55), (0, 511, 0, TOP), (512, 1023, 0, TOP), (1023, 1024, 0, TOP), (1024, 1024, 0, 0),
                      (n - 1, n - 1, 0, TOP), (n - 1, TOP, (n - 1) % 64, (n - 1) % 64), (n, TOP, 0, TOP), (0, TOP, 0, TOP),
                      (5, 4, 0, TOP), (0, TOP, 9, 8), (100, 900, 31, 32), (0, n - 1, 0, 63), (0, TOP, 0, 0)], dtype=np.uint32)
    lo, hi = matrix(boxes)
    gpu = build(dim, "l2sq", X, keys, M=4, M0=8, efc=16)
    gpu.set_label_column(1, 0, cols[1])
    gpu.set_label_column(2, 0, cols[2])
    got = check(gpu, Q, 10, 64, cols, [1, 2], lo, hi, 1, "n %d" % n, modes=("exact", "auto"))
    cnt = got["exact"][0][2]
    a, b = slot.astype(np.int64), (slot % 64).astype(np.int64)
    expect = np.array([int(((x0 <= a) & (a <= x1) & (y0 <= b) & (b <= y1)).sum()) for x0, x1, y0, y1 in boxes.astype(np.int64)])
    assert np.array_equal(cnt, np.minimum(expect, 10))
    assert cnt[17] == 1 and got["exact"][0][0][17][0] == keys[n - 1]  # the box of the last slot only: that row
    distinct = {tuple(int(v) for v in box): e for box, e in zip(boxes, expect)}
    assert got["exact"][1]["exact"][0] == sum(distinct.values())  # listed: every group's rows, overlaps counted per group


# ------------------------------------------------------------------------------------------------- 5. several passes
def test_overlapping_boxes_take_several_passes(monkeypatch):
    """boxes overlap, so the lists of one call can together exceed max(budget, rows) entries and the plan packs them into
    several passes; as many as the bitmap call's"""
    n, dim, nq = 3000, 16, 24
    X, Q = gc.make_data(n, dim, "l2sq", 2500, nq=nq)
    keys = keys_against_slot_order(n, 5000)
    rng = np.random.default_rng(25)
    cols = {0: rng.integers(0, 12, 5001).astype(np.uint32), 3: rng.integers(0, 4, 5001).astype(np.uint32)}
    boxes = np.array([(0, 11, 0, 3), (0, 5, 0, 3), (3, 9, 0, TOP), (6, 11, 0, 2), (0, TOP, 1, 3), (2, 10, 0, 3)] * 4, dtype=np.uint32)
    lo, hi = matrix(boxes)
    monkeypatch.setenv("VSS_EXACT_FILTER_LIST_ENTRIES", "1000")
    gpu = build(dim, "l2sq", X, keys, M=4, M0=8, efc=16)
    gpu.set_label_column(0, 0, cols[0])
    gpu.set_label_column(3, 0, cols[3])
    got = check(gpu, Q, 10, 64, cols, [0, 3], lo, hi, 0, "budget 1000", modes=("exact", "auto"))
    listed, _, passes = got["exact"][1]["exact"]
    assert listed == live_lengths(cols, [0, 3], keys, lo[:6], hi[:6]).sum() > n and passes >= 2


# ------------------------------------------------------------------------------------------------- 6. kernel shapes
class Base:
    """6000 x 32, three columns by row id: 0 a tenant of 100 values, 1 a timestamp below 10000, 3 a price below 1000; three
    NO_LABEL cells in each"""

    def __init__(self):
        self.metric, self.n, self.dim = "l2sq", 6000, 32
        self.X, self.Q = gc.make_data(self.n, self.dim, self.metric, 2600, nq=300)
        self.keys = keys_against_slot_order(self.n, 9000)
        rng = np.random.default_rng(26)
        self.cols, self.by_slot = {}, {}
        for c, top in ((0, 100), (1, 10000), (3, 1000)):
            by_slot = rng.integers(0, top, self.n).astype(np.uint32)
            by_slot[rng.choice(self.n, 3, replace=False)] = NO_LABEL
            self.cols[c] = np.full(9001, NO_LABEL, dtype=np.uint32)
            self.cols[c][self.keys] = by_slot
            self.by_slot[c] = by_slot
        self.gpu = build(self.dim, self.metric, self.X, self.keys)
        for c in self.cols:
            self.gpu.set_label_column(c, 0, self.cols[c])

    def check(self, Q, k, ef, columns, lo, hi, route_c, what, modes=MODES):
        return check(self.gpu, Q, k, ef, self.cols, columns, lo, hi, route_c, what, modes)


@pytest.fixture(scope="module")
def base():
    return Base()


# (timestamp, tenant): 3600 rows, 1500, 3000, 300, 6, all, none
SEVEN = np.array([(0, 5999, 0, 99), (2000, 4499, 0, TOP), (0, TOP, 0, 49), (7000, 7499, 0, 99), (100, 109, 0, TOP), (0, TOP, 0, TOP),
                  (10000, 20000, 0, 99)], dtype=np.uint32)


@pytest.mark.parametrize("ef", [64, 300, 600])  # lists in registers (2 and 8 per lane) and outside them
def test_list_widths(base, ef):
    lo, hi = matrix(SEVEN[np.arange(21) % 7])
    route_c = {64: 1000, 300: 300, 600: 160}[ef]  # len^2 * 64 <= route_c * limit * 6000 ends near 3000 rows at each limit
    got = base.check(base.Q[:21], 100, ef, [1, 0], lo, hi, route_c, "ef %d" % ef)
    assert (got["graph"][1]["shape"][4] != 0) == (ef == 600)  # beyond 512 the list has left the registers (the bitmap call's shape)
    assert set(got["auto"][0][3].tolist()) == {0, 1}


def test_one_query_takes_the_solo_kernel(base):
    for q, box in enumerate([(0, 4999, 0, 49), (5000, TOP, 20, TOP)]):
        lo, hi = matrix([box])
        got = base.check(base.Q[q:q + 1], 10, 64, [1, 0], lo, hi, 1, "one query")
        assert got["graph"][1]["shape"][6] == 1 and got["graph"][0][2][0] == 10


@pytest.mark.parametrize("nq", [204, 300])  # the join's chunk; more than a launch of one query per compute unit
def test_host_batches(base, nq):
    rng = np.random.default_rng(2660 + nq)
    lo, hi = np.empty((nq, 2), dtype=np.uint32), np.empty((nq, 2), dtype=np.uint32)
    lo[:, 0] = hi[:, 0] = rng.integers(0, 100, nq)       # tenant = ...
    wide = rng.integers(0, 3, nq) == 0                   # ... a third of them a tenant range of up to 90 values
    hi[wide, 0] = lo[wide, 0] + rng.integers(30, 90, wide.sum())
    lo[:, 1], hi[:, 1] = rng.integers(0, 9000, nq), TOP  # ... AND ts >= since, nearly every query its own box
    lo[::50, 1], hi[::50, 1] = 5, 1
    got = base.check(base.Q[:nq], 10, 64, [0, 1], lo, hi, 1500, "%d queries" % nq)
    assert set(got["auto"][0][3]) == {0, 1}


def test_rare_boxes_rerun(base):
    """boxes of about six rows and of one: the walk rejects nearly every row it meets, its pending candidates outgrow the register
    queue, and the queries are re-run through the unbounded one — reading the same table of boxes again, through a.work[idx]"""
    ts, tenant = base.by_slot[1], base.by_slot[0]
    s = np.sort(ts[ts != NO_LABEL])
    at = int(np.nonzero((ts == s[3000]) & (tenant != NO_LABEL))[0][0])
    six, one = (int(s[1000]), int(s[1005]), 0, TOP), (int(ts[at]), int(ts[at]), int(tenant[at]), int(tenant[at]))
    lo, hi = matrix([six, one] * 8)
    lens = live_lengths(base.cols, [1, 0], base.keys, lo[:2], hi[:2])
    assert 3 <= lens[0] <= 8 and 1 <= lens[1] <= 3
    got = base.check(base.Q[:16], 10, 64, [1, 0], lo, hi, 1500, "rare boxes", modes=("graph",))
    _, _, cnt, _ = got["graph"][0]
    assert np.all(cnt[0::2] <= lens[0]) and np.all(cnt[1::2] <= lens[1]) and cnt.sum() > 0  # (a walk may miss a row; it invents none)
    assert got["graph"][1]["stats"][3] > 0  # (the bitmap call's counter, and by check() this call's: queries were re-run)


def test_one_two_and_four_columns(base):
    """m = 1, 2 and 4 on one index (column 2 is set here; no other test of this module names it)"""
    rng = np.random.default_rng(264)
    base.cols[2] = np.full(8500, NO_LABEL, dtype=np.uint32)  # shorter than the others: row ids from 8500 on have no cell
    live = base.keys[base.keys < 8500]
    base.cols[2][live] = rng.integers(0, 8, len(live))
    base.gpu.set_label_column(2, 0, base.cols[2])
    nq = 21
    lo, hi = np.zeros((nq, 4), dtype=np.uint32), np.full((nq, 4), TOP, dtype=np.uint32)
    lo[:, 0], hi[:, 0] = (np.arange(nq) % 7) * 1000, (np.arange(nq) % 7) * 1000 + 4999  # column 1: a time window
    lo[:, 1], hi[:, 1] = 10 * (np.arange(nq) % 3), 10 * (np.arange(nq) % 3) + 69        # column 0: a tenant range
    lo[:, 2], hi[:, 2] = 0, 5                                                            # column 2
    lo[:, 3], hi[:, 3] = 100, 899                                                        # column 3
    lo[5, 2], hi[5, 2] = 6, 5
    for columns in ([1], [1, 0], [1, 0, 2, 3]):
        m = len(columns)
        base.check(base.Q[:nq], 10, 64, columns, lo[:, :m], hi[:, :m], 300, "%d columns" % m)


# ------------------------------------------------------------------------------------------------- 7. device form
def test_device_form(base):
    import torch
    nq, k = 35, 10
    Q = base.Q[:nq]
    boxes = SEVEN[np.arange(nq) % 7].copy()
    boxes[3] = (9, 2, 0, 99)
    lo, hi = matrix(boxes)
    d_Q = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    d_lo, d_hi = torch.from_numpy(lo.view(np.int32)).cuda(), torch.from_numpy(hi.view(np.int32)).cuda()
    for mode in MODES:
        ref = base.check(Q, k, 64, [1, 0], lo, hi, 1500, "host form", modes=(mode,))[mode][0]
        for bare in (False, True):
            d_keys = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
            d_dist = None if bare else torch.zeros((nq, k), dtype=torch.float32, device="cuda")
            d_cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
            d_route = None if bare else torch.full((nq,), 9, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            base.gpu.search_batch_by_label_box_device(d_Q.data_ptr(), nq, k, 64, [1, 0], d_lo.data_ptr(), d_hi.data_ptr(),
                                                      d_keys.data_ptr(), None if bare else d_dist.data_ptr(), d_cnt.data_ptr(),
                                                      None if bare else d_route.data_ptr(), mode, 1500)
            assert np.array_equal(d_keys.cpu().numpy(), ref[0]), mode
            assert np.array_equal(d_cnt.cpu().numpy().astype(np.uint32), ref[2]), mode
            if not bare:
                assert np.array_equal(d_dist.cpu().numpy().view(np.uint32), ref[1].view(np.uint32)), mode
                assert np.array_equal(d_route.cpu().numpy(), ref[3]), mode


# ------------------------------------------------------------------------------------------------- 8. lifecycle
def test_lifecycle(tmp_path):
    n, dim, nq = 3000, 16, 24
    rng = np.random.default_rng(28)
    X, Q = gc.make_data(n + 400, dim, "l2sq", 2800, nq=nq)
    keys = keys_against_slot_order(n, 5000)            # ids 2001 .. 5000
    new_keys = np.arange(400, dtype=np.int64) + 100    # the rows added later: ids 100 .. 499, labelled from the start
    cols = {0: rng.integers(0, 10, 5001).astype(np.uint32), 2: rng.integers(0, 1000, 5001).astype(np.uint32)}
    for c in cols:
        cols[c][rng.choice(5001, 50, replace=False)] = NO_LABEL
    columns = [2, 0]
    boxes = np.array([(0, 499, 0, 9), (100, 300, 0, 4), (250, 800, 3, 3), (900, TOP, 0, TOP), (5000, 6000, 0, TOP), (7, 7, 0, 9)] * 4,
                     dtype=np.uint32)
    lo, hi = matrix(boxes)
    gpu = build(dim, "l2sq", X[:n], keys, capacity=n + 400, M=8, M0=16, efc=32)
    before = gpu.memory_usage()
    gpu.set_labels(0, cols[0])  # column 0, by its first name
    gpu.set_label_column(2, 0, cols[2])
    assert gpu.memory_usage() >= before + 4 * (len(cols[0]) + len(cols[2]))
    assert gpu.labelled_rows() == gpu.label_column_rows(0) == 5001 and gpu.label_column_rows(2) == 5001
    assert gpu.label_column_rows(1) == gpu.label_column_rows(3) == 0
    got = check(gpu, Q, 10, 64, cols, columns, lo, hi, 100, "built")
    assert np.all(got["exact"][0][2][lo[:, 0] == 5000] == 0)  # no row carries a label from 5000 on in column 2 (yet)
    # rows removed, rows added into their slots, compaction: the columns are by row id and need no call
    gone = rng.choice(n, 700, replace=False)
    assert gpu.remove(keys[gone]) == 700
    check(gpu, Q, 10, 64, cols, columns, lo, hi, 100, "700 removed")
    gpu.add(new_keys, X[n:])
    got = check(gpu, Q, 10, 64, cols, columns, lo, hi, 100, "400 added into reused slots")
    assert np.any(np.isin(got["exact"][0][0], new_keys))
    gpu.compact()
    check(gpu, Q, 10, 64, cols, columns, lo, hi, 100, "compacted")
    # cells of ONE column overwritten: the answers follow that column by row id, the other column is as it was
    cols[2][2500:3500] = 5500
    gpu.set_label_column(2, 2500, cols[2][2500:3500])
    got = check(gpu, Q, 10, 64, cols, columns, lo, hi, 100, "overwritten")
    ids = got["exact"][0][0][lo[:, 0] == 5000]
    assert np.all(got["exact"][0][2][lo[:, 0] == 5000] == 10) and np.all((ids >= 2500) & (ids < 3500))
    # one column cleared: boxes that name it fail, boxes that do not still answer
    err = gc.pkg().VssError
    gpu.clear_label_column(2)
    assert gpu.label_column_rows(2) == 0 and gpu.labelled_rows() == 5001
    with pytest.raises(err, match="no label column 2"):
        gpu.search_batch_by_label_box(Q, 10, 64, columns, lo, hi)
    check(gpu, Q, 10, 64, cols, [0], lo[:, 1:], hi[:, 1:], 100, "column 2 cleared, column 0 alone", modes=("auto",))
    gpu.set_label_column(2, 0, cols[2])
    check(gpu, Q, 10, 64, cols, columns, lo, hi, 100, "column 2 set again", modes=("auto",))
    # clear_labels clears every column
    gpu.clear_labels()
    assert [gpu.label_column_rows(c) for c in range(4)] == [0, 0, 0, 0] and gpu.labelled_rows() == 0
    for named in ([0], [2]):
        with pytest.raises(err, match="no label column %d" % named[0]):
            gpu.search_batch_by_label_box(Q, 10, 64, named, lo[:, :1], hi[:, :1])
    # ... and so does save + load; the columns set again, the answers return
    gpu.set_label_column(0, 0, cols[0])
    gpu.set_label_column(2, 0, cols[2])
    ref = gpu.search_batch_by_label_box(Q, 10, 64, columns, lo, hi, "exact")
    blob = gpu.save()
    gpu.load(blob)
    assert [gpu.label_column_rows(c) for c in range(4)] == [0, 0, 0, 0]
    with pytest.raises(err, match="no label column"):
        gpu.search_batch_by_label_box(Q, 10, 64, columns, lo, hi)
    gpu.set_label_column(0, 0, cols[0])
    gpu.set_label_column(2, 0, cols[2])
    again = gpu.search_batch_by_label_box(Q, 10, 64, columns, lo, hi, "exact")
    assert_same(again[:3], ref[:3], "after save and load")
    check(gpu, Q, 10, 64, cols, columns, lo, hi, 100, "loaded and labelled again", modes=("auto",))


# ------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals(base):
    g, Q = base.gpu, np.ascontiguousarray(base.Q[:4])
    lo, hi = np.zeros((4, 2), dtype=np.uint32), np.full((4, 2), 5000, dtype=np.uint32)
    err = gc.pkg().VssError
    out = np.full((4, 10), -1, dtype=np.int64)
    cnt = np.zeros(4, dtype=np.uint32)

    def call(lib_index, nq, k, columns, n_columns, p_lo, p_hi, mode):
        """the C entry point itself; returns (status, message)"""
        cols = None if columns is None else np.asarray(columns, dtype=np.uint32)
        rc = lib_index.lib.vss_search_batch_by_label_box(lib_index.h, Q.ctypes.data, nq, k, 64, None if cols is None else cols.ctypes.data,
                                                         n_columns, p_lo, p_hi, mode, 0, out.ctypes.data, None, cnt.ctypes.data, None)
        return rc, lib_index.lib.vss_last_error(lib_index.h)

    L, H = lo.ctypes.data, hi.ctypes.data
    bare = gc.gpu_index(base.dim, base.metric)
    # 1. the mode, first: even on an index without columns, with no columns named, NULL everywhere
    for mode in (3, -1, 255):
        with pytest.raises(err, match="mode"):
            g.search_batch_by_label_box(Q, 10, 64, [1, 0], lo, hi, mode)
        for index in (g, bare):
            rc, msg = call(index, 4, 10, None, 0, None, None, mode)
            assert rc != 0 and b"mode" in msg
    # 2. n_columns 0 or above 4, before the NULL columns pointer
    for m in (0, 5, 1 << 40):
        rc, msg = call(g, 4, 10, None, m, L, H, 2)
        assert rc != 0 and b"n_columns" in msg
    # 3. columns NULL
    rc, msg = call(g, 4, 10, None, 2, L, H, 2)
    assert rc != 0 and b"null columns" in msg
    # 4. a column number >= 4, or one named twice — the message names it — before NULL lo / hi
    rc, msg = call(g, 4, 10, [1, 4], 2, None, None, 2)
    assert rc != 0 and b"column 4" in msg
    rc, msg = call(g, 4, 10, [3, 1, 3], 3, None, None, 2)
    assert rc != 0 and b"column 3 is named twice" in msg
    with pytest.raises(err, match="column 1 is named twice"):
        g.search_batch_by_label_box(Q, 10, 64, [1, 1], lo, hi)
    # 5. NULL lo / hi with queries to answer, before the column that was never set
    for p_lo, p_hi in ((None, H), (L, None), (None, None)):
        for mode in (0, 1, 2):
            rc, msg = call(bare, 4, 10, [1, 0], 2, p_lo, p_hi, mode)
            assert rc != 0 and b"null lo / hi" in msg
    # 6. a named column that was never set, with its number
    for mode in MODES:
        with pytest.raises(err, match="no label column 1"):
            bare.search_batch_by_label_box(Q, 10, 64, [1, 0], lo, hi, mode)
    bare.set_label_column(1, 0, np.zeros(10, dtype=np.uint32))
    with pytest.raises(err, match="no label column 0"):
        bare.search_batch_by_label_box(Q, 10, 64, [1, 0], lo, hi)
    # the column calls refuse a column >= 4 too
    with pytest.raises(err, match="column 4"):
        g.set_label_column(4, 0, np.zeros(3, dtype=np.uint32))
    with pytest.raises(err, match="column 7"):
        g.clear_label_column(7)
    assert g.label_column_rows(4) == 0
    # the two no-ops: no queries (nothing to read), k == 0
    assert call(g, 0, 10, [1, 0], 2, None, None, 2)[0] == 0
    assert call(g, 4, 0, [1, 0], 2, L, H, 2)[0] == 0
    assert np.all(out == -1) and np.all(cnt == 0)  # nothing was written by any of them
    base.check(Q, 10, 64, [1, 0], lo, hi, 1500, "after the refusals")
