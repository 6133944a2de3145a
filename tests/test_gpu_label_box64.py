"""-m gpu: vss_search_batch_by_label_box64 — per-query conjunctions of inclusive ranges with 64-BIT ENDS over up to four resident
label columns of either width, 32 or 64 bits, mixed (csrc/label_filter.h; the walkers' admission in csrc/hnsw_kernels.h, the
listing kernels in csrc/exact_filtered_kernels.h).

Contract, and the only yardstick here: form the n_queries x 2m matrix of 64-bit words whose row q is (lo[q,0], hi[q,0], lo[q,1],
hi[q,1], ...).  Let b_0 < b_1 < ... be its distinct RAW rows, ascending lexicographically as unsigned 64-bit words (nothing
canonicalised), bitmap g have bit r set iff for every named column c_j: r < rows(c_j), the cell — a 32-bit cell zero-extended, its
NO_LABEL read as NO_LABEL64 — is not NO_LABEL64 and lo_j <= cell <= hi_j, n_bits be the smallest rows(c_j), and group_of[q] be the
index of query q's row.  Then the call in mode graph / exact / auto returns cell for cell — row ids, f32 distance bits, counts,
routes — what the bitmap call of that mode returns for that table, and leaves the same counters behind.  No tolerance, no cell
left out.
"""
import numpy as np
import pytest

import gpu_common as gc
from test_gpu_exact_filtered import _bitmap, _words, assert_same, keys_against_slot_order
from test_gpu_label_box import SEVEN, mixed_chunk
from test_gpu_label_search import MODES, NO_LABEL, assert_nothing, bitmap_call, build, counters

pytestmark = pytest.mark.gpu

TOP = 0xFFFFFFFF             # in the 32-bit test's boxes: no upper bound
NO_LABEL64 = (1 << 64) - 1
TOP64 = np.uint64(NO_LABEL64)  # as hi: no upper bound
T32 = 1 << 32
BASE = (1 << 63) + 10 ** 15  # a mapped TIMESTAMP of our days: every comparison needs the high word


def widen(column):
    """a column's cells as the rule reads them"""
    if column.dtype == np.uint64:
        return column
    assert column.dtype == np.uint32
    return np.where(column == NO_LABEL, TOP64, column.astype(np.uint64))


def shifted(values, base):
    """32-bit cells or ends moved up by `base`; NO_LABEL / "no upper bound" stays what it is, 64 bits wide"""
    values = np.asarray(values, dtype=np.uint32)
    return np.where(values == TOP, TOP64, values.astype(np.uint64) + np.uint64(base))


def matrix64(boxes, bases):
    """the 32-bit tests' [(lo_0, hi_0, lo_1, hi_1, ...), ...] -> the call's lo and hi matrices, named column j moved up by bases[j]"""
    boxes = np.asarray(boxes, dtype=np.uint32)
    lo = np.stack([shifted(boxes[:, 2 * j], b) for j, b in enumerate(bases)], axis=1)
    hi = np.stack([shifted(boxes[:, 2 * j + 1], b) for j, b in enumerate(bases)], axis=1)
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


def admitted(cols, columns, lo_row, hi_row):
    """NumPy's restatement of the rule: the mask over row ids below the shortest named column"""
    n_bits = min(len(cols[c]) for c in columns)
    mask = np.ones(n_bits, dtype=bool)
    for c, a, b in zip(columns, lo_row, hi_row):
        cell = widen(cols[c][:n_bits])
        mask &= (cell != TOP64) & (np.uint64(a) <= cell) & (cell <= np.uint64(b))
    return mask


def derived_table(cols, columns, lo, hi):
    """the table of the contract: (bitmaps, n_bits, group_of)"""
    rows = np.empty((len(lo), 2 * len(columns)), dtype=np.uint64)
    rows[:, 0::2], rows[:, 1::2] = lo, hi
    groups, group_of = np.unique(rows, axis=0, return_inverse=True)  # rows ascending lexicographically, as unsigned 64-bit words
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
        assert gpu.label_column_width(c) == 8 * cols[c].dtype.itemsize, what
    lo, hi = np.asarray(lo, dtype=np.uint64).reshape(len(Q), -1), np.asarray(hi, dtype=np.uint64).reshape(len(Q), -1)
    table = derived_table(cols, columns, lo, hi)
    out = {}
    for mode in modes:
        where = "%s, columns %r, mode %s, route_c %d" % (what, list(columns), mode, route_c)
        ref = bitmap_call(gpu, mode, Q, k, ef, table, route_c)
        ref_counters = counters(gpu, mode)
        got = gpu.search_batch_by_label_box64(Q, k, ef, columns, lo, hi, mode, route_c)
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


def set_column(gpu, c, column, first=0):
    if column.dtype == np.uint64:
        gpu.set_label_column64(c, first, column)
    else:
        gpu.set_label_column(c, first, column)


# ------------------------------------------------------------------------------------------------- 1. the mixed chunk
def mixed_chunk64():
    """the mixed chunk of test_gpu_label_box.py — 6000 rows, row id != slot, 37 boxes — with column 1 the 32-bit tenant as it is
    and column 3 a 64-bit timestamp, BASE + what the 32-bit column holds: NO_LABEL cells become NO_LABEL64, "no upper bound" stays
    no upper bound, every other end moves up with the cells"""
    keys, cols32, lo32, hi32 = mixed_chunk()
    cols = {1: cols32[1], 3: shifted(cols32[3], BASE)}
    boxes = np.empty((len(lo32), 4), dtype=np.uint32)
    boxes[:, 0::2], boxes[:, 1::2] = lo32, hi32
    lo, hi = matrix64(boxes, (0, BASE))
    return keys, cols, lo, hi, cols32, lo32, hi32


@pytest.mark.parametrize("metric,dim", [("l2sq", 100), ("cosine", 100), ("ip", 100), ("l2sq", 3), ("l2sq", 768)])
def test_mixed_chunk(metric, dim):
    n, nq, k, ef = 6000, 37, 10, 64
    columns = [1, 3]
    keys, cols, lo, hi, _, _, _ = mixed_chunk64()
    # on the NumPy restatement, before any GPU call
    assert cols[1].dtype == np.uint32 and cols[3].dtype == np.uint64
    assert (cols[1] == NO_LABEL).sum() == 20 and (cols[3] == TOP64).sum() == 20
    has_ts = cols[3] != TOP64
    assert np.all(cols[3][has_ts] >> np.uint64(32) == np.uint64(BASE >> 32)) and BASE >> 32 > 1 << 31
    lens = live_lengths(cols, columns, keys, lo, hi)
    assert 2300 <= lens.max() <= 2700
    nothing = (np.any(lo > hi, axis=1) | (lo[:, 0] == TOP64) | (lo[:, 0] == np.uint64(0x80000000))
               | ((lo[:, 0] == np.uint64(11)) & (lo[:, 1] == np.uint64(BASE + 9000))))
    assert np.array_equal(nothing, lens == 0)
    assert nothing.sum() == 9
    each_alone = (live_lengths(cols, [1], keys, [[11]], [[11]])[0] > 0
                  and live_lengths(cols, [3], keys, [[BASE + 9000]], [[BASE + 9999]])[0] > 0)
    assert each_alone  # ... although each clause of that box alone has rows
    X, Q = gc.make_data(n, dim, metric, 2100 + dim, nq=nq)
    gpu = build(dim, metric, X, keys)
    gpu.set_label_column(1, 0, cols[1])
    gpu.set_label_column64(3, 0, cols[3])
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


# ------------------------------------------------------------------------------------------------- 2. against the 32-bit calls
def test_narrow_columns_and_low_ends_are_the_box_call():
    """every named column 32 bits wide, every end below 2^32 (hi = 2^32 - 1 is then an ordinary end that no cell reaches, and
    admits what the 32-bit "no upper bound" admits): answers and counters of vss_search_batch_by_label_box"""
    n, k, ef = 6000, 10, 64
    keys, cols, lo, hi = mixed_chunk()
    X, Q = gc.make_data(n, 32, "l2sq", 2300, nq=len(lo))
    gpu = build(32, "l2sq", X, keys)
    gpu.set_label_column(1, 0, cols[1])
    gpu.set_label_column(3, 0, cols[3])
    assert gpu.label_column_width(1) == gpu.label_column_width(3) == 32
    for route_c in (0, 300):
        for mode in MODES:
            where = "mode %s, route_c %d" % (mode, route_c)
            ref = gpu.search_batch_by_label_box(Q, k, ef, [1, 3], lo, hi, mode, route_c)
            ref_counters = counters(gpu, mode)
            got = gpu.search_batch_by_label_box64(Q, k, ef, [1, 3], lo.astype(np.uint64), hi.astype(np.uint64), mode, route_c)
            assert_same(got[:3], ref[:3], where)
            assert np.array_equal(got[3], ref[3]), where + ": routes"
            assert counters(gpu, mode) == ref_counters, where
    assert set(got[3].tolist()) == {0, 1}  # (mode auto took both roads)
    check(gpu, Q, k, ef, cols, [1, 3], lo.astype(np.uint64), hi.astype(np.uint64), 300, "narrow columns against the bitmaps")


def test_one_narrow_column_0_is_the_range_call():
    n, nq, dim, k = 6000, 37, 100, 10
    X, Q = gc.make_data(n, dim, "l2sq", 2200, nq=nq)
    keys = keys_against_slot_order(n, 9000)
    rng = np.random.default_rng(22)
    labels = rng.integers(0, 10000, 8000).astype(np.uint32)
    labels[rng.choice(np.arange(3001, 8000), 20, replace=False)] = NO_LABEL
    ranges = np.array(([(0, 4999)] * 5 + [(1000, 1999)] * 4 + [(3000, 6000)] * 4 + [(0, TOP)] * 4 + [(9, 2)] * 3 + [(7000, 100)] * 2
                       + [(TOP, TOP)] * 2 + [(2500, 2600)] * 4 + [(9000, TOP)] * 4 + [(20000, 30000)] * 2 + [(4000, 4100)] * 3),
                      dtype=np.uint32)[rng.permutation(nq)]
    gpu = build(dim, "l2sq", X, keys)
    gpu.set_labels(0, labels)
    lo, hi = ranges[:, :1].astype(np.uint64), ranges[:, 1:].astype(np.uint64)
    for route_c in (1500, 3):
        for mode in MODES:
            where = "mode %s, route_c %d" % (mode, route_c)
            ref = gpu.search_batch_by_label_range(Q, k, 64, ranges[:, 0], ranges[:, 1], mode, route_c)
            ref_counters = counters(gpu, mode)
            got = gpu.search_batch_by_label_box64(Q, k, 64, [0], lo, hi, mode, route_c)
            assert_same(got[:3], ref[:3], where)
            assert np.array_equal(got[3], ref[3]), where + ": routes"
            assert counters(gpu, mode) == ref_counters, where
    # ... and hi = NO_LABEL64 is what the range call's hi = NO_LABEL is
    hi[ranges[:, 1] == TOP] = TOP64
    for mode in MODES:
        ref = gpu.search_batch_by_label_range(Q, k, 64, ranges[:, 0], ranges[:, 1], mode, 1500)
        got = gpu.search_batch_by_label_box64(Q, k, 64, [0], lo, hi, mode, 1500)
        assert_same(got[:3], ref[:3], "no upper bound, mode " + mode)


# ------------------------------------------------------------------------------------------------- 3. the high word
def test_a_pair_that_differs_only_in_the_high_word():
    """cells 5 .. 9 and 2^32 + 5 .. 2^32 + 9, ends (2^32 + 5, 2^32 + 9): only the latter are inside.  Any truncation to 32 bits —
    of the cells, of the ends, in the walker, in the listing, in the groups — admits the former too"""
    n, dim, k = 2000, 16, 10
    X, Q = gc.make_data(n, dim, "l2sq", 6600, nq=8)
    keys = keys_against_slot_order(n, 4000)
    rng = np.random.default_rng(66)
    low = rng.integers(5, 10, 4001).astype(np.uint64)
    high = rng.integers(0, 2, 4001).astype(bool)
    cols = {2: np.where(high, low + np.uint64(T32), low)}
    lo = np.array([[T32 + 5], [T32 + 5], [5], [5], [T32 + 7], [7], [T32 + 9], [T32 + 5]], dtype=np.uint64)
    hi = np.array([[T32 + 9], [T32 + 9], [9], [T32 + 9], [T32 + 7], [T32 + 6], [T32 + 5], [2 * T32 + 9]], dtype=np.uint64)
    lens = live_lengths(cols, [2], keys, lo, hi)
    assert lens[0] == high[keys].sum() and lens[2] == (~high[keys]).sum() and lens[3] == n and lens[6] == 0 and lens[7] == lens[0]
    assert 0 < lens[4] < lens[0] and lens[5] > lens[2] // 2
    gpu = build(dim, "l2sq", X, keys, M=8, M0=16, efc=32)
    gpu.set_label_column64(2, 0, cols[2])
    got = check(gpu, Q, k, 64, cols, [2], lo, hi, 30, "high word")
    for mode in MODES:
        ids = [row[row >= 0] for row in got[mode][0][0]]
        assert len(ids[0]) and len(ids[2]) and len(ids[4]), mode
        assert np.all(high[ids[0]]) and np.all(high[ids[1]]) and np.all(~high[ids[2]]), mode
        assert np.all(cols[2][ids[4]] == np.uint64(T32 + 7)) and got[mode][0][2][6] == 0, mode
    assert np.array_equal(got["exact"][0][2], np.minimum(lens, k))


# ------------------------------------------------------------------------------------------------- 4. column order
def test_column_order_changes_no_answer():
    n, k, ef = 6000, 10, 64
    keys, cols, lo, hi, _, _, _ = mixed_chunk64()
    X, Q = gc.make_data(n, 32, "l2sq", 2300, nq=len(lo))
    gpu = build(32, "l2sq", X, keys)
    gpu.set_label_column(1, 0, cols[1])
    gpu.set_label_column64(3, 0, cols[3])
    for mode in MODES:
        a = gpu.search_batch_by_label_box64(Q, k, ef, [1, 3], lo, hi, mode, 300)
        b = gpu.search_batch_by_label_box64(Q, k, ef, [3, 1], lo[:, ::-1], hi[:, ::-1], mode, 300)
        assert_same(a[:3], b[:3], "columns swapped, mode " + mode)
        assert np.array_equal(a[3], b[3]), mode
    assert set(a[3].tolist()) == {0, 1}  # (mode auto took both roads)


# ------------------------------------------------------------------------------------------------- 5. listing edges
@pytest.mark.parametrize("n", [1, 511, 512, 513, 1025])  # FL_WAVE_SLOTS = 512
def test_listing_edges(n):
    """column 1's cell is BASE + the SLOT, 64 bits wide, and column 2's the slot modulo 64, 32 bits wide (a listing wave owns 512
    consecutive slots, a row of it 64), so a box's ends name lanes: lanes 0 and 63 of every row, a whole row of 64, runs across a
    row's edge and across the 512-slot block's, the last slot only"""
    dim = 8
    X, Q = gc.make_data(n, dim, "l2sq", 2400 + n, nq=26)
    keys = keys_against_slot_order(n, 2000)
    slot = np.arange(n, dtype=np.uint32)
    cols = {1: np.full(2001, TOP64, dtype=np.uint64), 2: np.full(2001, NO_LABEL, dtype=np.uint32)}
    cols[1][keys], cols[2][keys] = slot.astype(np.uint64) + np.uint64(BASE), slot % 64
    boxes = np.array([(0, TOP, 0, 0), (0, TOP, 63, 63), (0, 511, 63, 63), (64, 127, 0, 63), (64, 127, 0, TOP), (60, 70, 0, 63),
                      (60, 70, 60, 63), (60, 70, 0, 6), (448, 511, 0, 63), (511, 511, 63, 63), (511, 512, 0, TOP), (512, 512, 0, 0),
                      (500, 530, 10, 55), (0, 511, 0, TOP), (512, 1023, 0, TOP), (1023, 1024, 0, TOP), (1024, 1024, 0, 0),
                      (n - 1, n - 1, 0, TOP), (n - 1, TOP, (n - 1) % 64, (n - 1) % 64), (n, TOP, 0, TOP), (0, TOP, 0, TOP),
                      (5, 4, 0, TOP), (0, TOP, 9, 8), (100, 900, 31, 32), (0, n - 1, 0, 63), (0, TOP, 0, 0)], dtype=np.uint32)
    lo, hi = matrix64(boxes, (BASE, 0))
    gpu = build(dim, "l2sq", X, keys, M=4, M0=8, efc=16)
    gpu.set_label_column64(1, 0, cols[1])
    gpu.set_label_column(2, 0, cols[2])
    got = check(gpu, Q, 10, 64, cols, [1, 2], lo, hi, 1, "n %d" % n, modes=("exact", "auto"))
    cnt = got["exact"][0][2]
    a, b = slot.astype(np.int64), (slot % 64).astype(np.int64)
    expect = np.array([int(((x0 <= a) & (a <= x1) & (y0 <= b) & (b <= y1)).sum()) for x0, x1, y0, y1 in boxes.astype(np.int64)])
    assert np.array_equal(cnt, np.minimum(expect, 10))
    assert cnt[17] == 1 and got["exact"][0][0][17][0] == keys[n - 1]  # the box of the last slot only: that row
    distinct = {tuple(int(v) for v in box): e for box, e in zip(boxes, expect)}
    assert got["exact"][1]["exact"][0] == sum(distinct.values())  # listed: every group's rows, overlaps counted per group


# ------------------------------------------------------------------------------------------------- 6. kernel shapes
class Base:
    """6000 x 32, three columns by row id: 0 a tenant of 100 values, 32 bits wide; 1 a timestamp BASE + [0, 10000), 64 bits wide;
    3 a price below 1000, 32 bits wide; three NULL cells in each"""

    def __init__(self):
        self.metric, self.n, self.dim = "l2sq", 6000, 32
        self.X, self.Q = gc.make_data(self.n, self.dim, self.metric, 2600, nq=300)
        self.keys = keys_against_slot_order(self.n, 9000)
        rng = np.random.default_rng(26)  # (the data, keys and cells of test_gpu_label_box.py's base: the timestamps moved up by BASE)
        self.cols, self.by_slot, self.base = {}, {}, {0: 0, 1: BASE, 2: T32 - 4, 3: 0}
        for c, top in ((0, 100), (1, 10000), (3, 1000)):
            by_slot = rng.integers(0, top, self.n).astype(np.uint32)
            by_slot[rng.choice(self.n, 3, replace=False)] = NO_LABEL
            column = np.full(9001, NO_LABEL, dtype=np.uint32)
            column[self.keys] = by_slot
            self.cols[c] = shifted(column, BASE) if c == 1 else column
            self.by_slot[c] = by_slot
        self.gpu = build(self.dim, self.metric, self.X, self.keys)
        for c in self.cols:
            set_column(self.gpu, c, self.cols[c])

    def matrix(self, boxes, columns):
        return matrix64(boxes, [self.base[c] for c in columns])

    def check(self, Q, k, ef, columns, lo, hi, route_c, what, modes=MODES):
        return check(self.gpu, Q, k, ef, self.cols, columns, lo, hi, route_c, what, modes)


@pytest.fixture(scope="module")
def base():
    return Base()


@pytest.mark.parametrize("ef", [64, 300, 600])  # lists in registers (2 and 8 per lane) and outside them
def test_list_widths(base, ef):
    lo, hi = base.matrix(SEVEN[np.arange(21) % 7], [1, 0])  # (timestamp, tenant): 3600 rows, 1500, 3000, 300, 6, all, none
    route_c = {64: 1000, 300: 300, 600: 160}[ef]  # len^2 * 64 <= route_c * limit * 6000 ends near 3000 rows at each limit
    got = base.check(base.Q[:21], 100, ef, [1, 0], lo, hi, route_c, "ef %d" % ef)
    assert (got["graph"][1]["shape"][4] != 0) == (ef == 600)  # beyond 512 the list has left the registers (the bitmap call's shape)
    assert set(got["auto"][0][3].tolist()) == {0, 1}


def test_one_query_takes_the_solo_kernel(base):
    for q, box in enumerate([(0, 4999, 0, 49), (5000, TOP, 20, TOP)]):
        lo, hi = base.matrix([box], [1, 0])
        got = base.check(base.Q[q:q + 1], 10, 64, [1, 0], lo, hi, 1, "one query")
        assert got["graph"][1]["shape"][6] == 1 and got["graph"][0][2][0] == 10


@pytest.mark.parametrize("nq", [204, 300])  # the join's chunk; more than a launch of one query per compute unit
def test_host_batches(base, nq):
    rng = np.random.default_rng(2660 + nq)
    lo, hi = np.empty((nq, 2), dtype=np.uint64), np.empty((nq, 2), dtype=np.uint64)
    lo[:, 0] = hi[:, 0] = rng.integers(0, 100, nq)       # tenant = ...
    wide = rng.integers(0, 3, nq) == 0                   # ... a third of them a tenant range of up to 90 values
    hi[wide, 0] = lo[wide, 0] + rng.integers(30, 90, wide.sum()).astype(np.uint64)
    lo[:, 1], hi[:, 1] = rng.integers(0, 9000, nq).astype(np.uint64) + np.uint64(BASE), TOP64  # ... AND ts >= since
    lo[::50, 1], hi[::50, 1] = BASE + 5, BASE + 1
    got = base.check(base.Q[:nq], 10, 64, [0, 1], lo, hi, 1500, "%d queries" % nq)
    assert set(got["auto"][0][3]) == {0, 1}


def test_rare_boxes_rerun(base):
    """boxes of about six rows and of one: the walk rejects nearly every row it meets, its pending candidates outgrow the register
    queue, and the queries are re-run through the unbounded one — reading the same table of boxes again, through a.work[idx]"""
    ts, tenant = base.by_slot[1], base.by_slot[0]
    s = np.sort(ts[ts != NO_LABEL])
    at = int(np.nonzero((ts == s[3000]) & (tenant != NO_LABEL))[0][0])
    six, one = (int(s[1000]), int(s[1005]), 0, TOP), (int(ts[at]), int(ts[at]), int(tenant[at]), int(tenant[at]))
    lo, hi = base.matrix([six, one] * 8, [1, 0])
    lens = live_lengths(base.cols, [1, 0], base.keys, lo[:2], hi[:2])
    assert 3 <= lens[0] <= 8 and 1 <= lens[1] <= 3
    got = base.check(base.Q[:16], 10, 64, [1, 0], lo, hi, 1500, "rare boxes", modes=("graph",))
    _, _, cnt, _ = got["graph"][0]
    assert np.all(cnt[0::2] <= lens[0]) and np.all(cnt[1::2] <= lens[1]) and cnt.sum() > 0  # (a walk may miss a row; it invents none)
    assert got["graph"][1]["stats"][3] > 0  # (the bitmap call's counter, and by check() this call's: queries were re-run)


def test_one_two_and_four_columns(base):
    """m = 1, 2 and 4 on one index, widths 64 / 32 + 64 / 64 + 32 + 64 + 32 (column 2 is set here, 64 bits wide with cells on both
    sides of 2^32; no other test of this module names it)"""
    rng = np.random.default_rng(264)
    small = np.full(8500, NO_LABEL, dtype=np.uint32)  # shorter than the others: row ids from 8500 on have no cell
    live = base.keys[base.keys < 8500]
    small[live] = rng.integers(0, 8, len(live))
    base.cols[2] = shifted(small, base.base[2])  # 2^32 - 4 .. 2^32 + 3
    base.gpu.set_label_column64(2, 0, base.cols[2])
    nq = 21
    boxes = np.zeros((nq, 8), dtype=np.uint32)
    boxes[:, 0], boxes[:, 1] = (np.arange(nq) % 7) * 1000, (np.arange(nq) % 7) * 1000 + 4999  # column 1: a time window
    boxes[:, 2], boxes[:, 3] = 10 * (np.arange(nq) % 3), 10 * (np.arange(nq) % 3) + 69        # column 0: a tenant range
    boxes[:, 4], boxes[:, 5] = 0, 5                                                            # column 2: across 2^32
    boxes[:, 6], boxes[:, 7] = 100, 899                                                        # column 3
    boxes[5, 4], boxes[5, 5] = 6, 5
    for columns in ([1], [0, 1], [1, 0, 2, 3]):
        m = len(columns)
        order = [1, 0, 2, 3].index
        mine = np.concatenate([boxes[:, 2 * order(c):2 * order(c) + 2] for c in columns], axis=1)
        lo, hi = base.matrix(mine, columns)
        assert [base.gpu.label_column_width(c) for c in columns] == {1: [64], 2: [32, 64], 4: [64, 32, 64, 32]}[m]
        got = base.check(base.Q[:nq], 10, 64, columns, lo, hi, 300, "%d columns" % m)
        assert got["exact"][0][2].sum() > 0
    assert got["exact"][0][2][5] == 0


# ------------------------------------------------------------------------------------------------- 7. device form
def test_device_form(base):
    import torch
    nq, k = 35, 10
    Q = base.Q[:nq]
    boxes = SEVEN[np.arange(nq) % 7].copy()
    boxes[3] = (9, 2, 0, 99)
    lo, hi = base.matrix(boxes, [1, 0])
    d_Q = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    d_lo, d_hi = torch.from_numpy(lo.view(np.int64)).cuda(), torch.from_numpy(hi.view(np.int64)).cuda()
    for mode in MODES:
        ref = base.check(Q, k, 64, [1, 0], lo, hi, 1500, "host form", modes=(mode,))[mode][0]
        for bare in (False, True):
            d_keys = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
            d_dist = None if bare else torch.zeros((nq, k), dtype=torch.float32, device="cuda")
            d_cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
            d_route = None if bare else torch.full((nq,), 9, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            base.gpu.search_batch_by_label_box64_device(d_Q.data_ptr(), nq, k, 64, [1, 0], d_lo.data_ptr(), d_hi.data_ptr(),
                                                        d_keys.data_ptr(), None if bare else d_dist.data_ptr(), d_cnt.data_ptr(),
                                                        None if bare else d_route.data_ptr(), mode, 1500)
            assert np.array_equal(d_keys.cpu().numpy(), ref[0]), mode
            assert np.array_equal(d_cnt.cpu().numpy().astype(np.uint32), ref[2]), mode
            if not bare:
                assert np.array_equal(d_dist.cpu().numpy().view(np.uint32), ref[1].view(np.uint32)), mode
                assert np.array_equal(d_route.cpu().numpy(), ref[3]), mode
    # the setter's device form: the same column from device memory into a free slot
    column = base.cols[1]
    d_column = torch.from_numpy(column.view(np.int64)).cuda()
    torch.cuda.synchronize()
    other = gc.gpu_index(base.dim, base.metric)
    other.set_label_column64_device(2, 0, d_column.data_ptr(), len(column))
    assert other.label_column_width(2) == 64 and other.label_column_rows(2) == len(column)


# ------------------------------------------------------------------------------------------------- 8. lifecycle
def test_lifecycle():
    n, dim, nq = 3000, 16, 24
    rng = np.random.default_rng(28)
    X, Q = gc.make_data(n + 400, dim, "l2sq", 2800, nq=nq)
    keys = keys_against_slot_order(n, 5000)            # ids 2001 .. 5000
    new_keys = np.arange(400, dtype=np.int64) + 100    # the rows added later: ids 100 .. 499, labelled from the start
    narrow = {0: rng.integers(0, 10, 5001).astype(np.uint32), 2: rng.integers(0, 1000, 5001).astype(np.uint32)}
    for c in narrow:
        narrow[c][rng.choice(5001, 50, replace=False)] = NO_LABEL
    cols = {0: narrow[0], 2: shifted(narrow[2], BASE)}
    columns = [2, 0]
    boxes = np.array([(0, 499, 0, 9), (100, 300, 0, 4), (250, 800, 3, 3), (900, TOP, 0, TOP), (5000, 6000, 0, TOP), (7, 7, 0, 9)] * 4,
                     dtype=np.uint32)
    lo, hi = matrix64(boxes, (BASE, 0))
    gpu = build(dim, "l2sq", X[:n], keys, capacity=n + 400, M=8, M0=16, efc=32)
    assert [gpu.label_column_width(c) for c in range(5)] == [0, 0, 0, 0, 0]
    before = gpu.memory_usage()
    gpu.set_labels(0, cols[0])
    # set in two writes with a gap between them: cells 0 .. 1999, then 3000 .. 5000; the gap reads as NULL until it is written
    gpu.set_label_column64(2, 0, cols[2][:2000])
    assert gpu.label_column_rows(2) == 2000 and gpu.label_column_width(2) == 64
    gpu.set_label_column64(2, 3000, cols[2][3000:])
    assert gpu.label_column_rows(2) == 5001
    assert gpu.memory_usage() >= before + 4 * len(cols[0]) + 8 * len(cols[2])  # 8 bytes a cell
    gapped = dict(cols)
    gapped[2] = cols[2].copy()
    gapped[2][2000:3000] = TOP64
    got = check(gpu, Q, 10, 64, gapped, columns, lo, hi, 100, "written around a gap")
    assert not np.any((got["exact"][0][0] >= 2000) & (got["exact"][0][0] < 3000))
    gpu.set_label_column64(2, 2000, cols[2][2000:3000])
    assert [gpu.label_column_width(c) for c in range(4)] == [32, 0, 64, 0]
    got = check(gpu, Q, 10, 64, cols, columns, lo, hi, 100, "built")
    assert np.all(got["exact"][0][2][boxes[:, 0] == 5000] == 0)  # no row carries a cell from BASE + 5000 on in column 2 (yet)
    # rows removed, rows added into their slots, compaction: the columns are by row id and need no call
    gone = rng.choice(n, 700, replace=False)
    assert gpu.remove(keys[gone]) == 700
    check(gpu, Q, 10, 64, cols, columns, lo, hi, 100, "700 removed")
    gpu.add(new_keys, X[n:])
    got = check(gpu, Q, 10, 64, cols, columns, lo, hi, 100, "400 added into reused slots")
    assert np.any(np.isin(got["exact"][0][0], new_keys))
    gpu.compact()
    check(gpu, Q, 10, 64, cols, columns, lo, hi, 100, "compacted")
    # cells of the wide column overwritten: the answers follow it by row id
    cols[2][2500:3500] = BASE + 5500
    gpu.set_label_column64(2, 2500, cols[2][2500:3500])
    got = check(gpu, Q, 10, 64, cols, columns, lo, hi, 100, "overwritten")
    ids = got["exact"][0][0][boxes[:, 0] == 5000]
    assert np.all(got["exact"][0][2][boxes[:, 0] == 5000] == 10) and np.all((ids >= 2500) & (ids < 3500))
    # cleared: the width is forgotten, the memory returned, and the slot takes the OTHER width
    err = gc.pkg().VssError
    with_both = gpu.memory_usage()
    gpu.clear_label_column(2)
    assert gpu.label_column_rows(2) == 0 and gpu.label_column_width(2) == 0 and gpu.memory_usage() <= with_both - 8 * 5001
    with pytest.raises(err, match="no label column 2"):
        gpu.search_batch_by_label_box64(Q, 10, 64, columns, lo, hi)
    gpu.set_label_column(2, 0, narrow[2])
    assert gpu.label_column_width(2) == 32
    now = {0: cols[0], 2: narrow[2]}
    lo32, hi32 = matrix64(boxes, (0, 0))
    check(gpu, Q, 10, 64, now, columns, lo32, hi32, 100, "column 2 set again, 32 bits wide", modes=("auto",))
    # ... and column 0 likewise: cleared, then 64 bits wide
    gpu.clear_label_column(0)
    gpu.set_label_column64(0, 0, shifted(narrow[0], T32))
    assert gpu.label_column_width(0) == 64 and gpu.labelled_rows() == 5001
    now = {0: shifted(narrow[0], T32), 2: narrow[2]}
    lo_w, hi_w = matrix64(boxes, (0, T32))
    check(gpu, Q, 10, 64, now, columns, lo_w, hi_w, 100, "column 0 64 bits wide", modes=("auto", "graph"))
    # clear_labels clears every column, wide ones included
    gpu.clear_labels()
    assert [gpu.label_column_rows(c) for c in range(4)] == [0, 0, 0, 0] and [gpu.label_column_width(c) for c in range(4)] == [0] * 4
    # ... and so does save + load; the columns set again, the answers return
    gpu.set_labels(0, cols[0])
    gpu.set_label_column64(2, 0, cols[2])
    ref = gpu.search_batch_by_label_box64(Q, 10, 64, columns, lo, hi, "exact")
    blob = gpu.save()
    gpu.load(blob)
    assert [gpu.label_column_rows(c) for c in range(4)] == [0, 0, 0, 0] and [gpu.label_column_width(c) for c in range(4)] == [0] * 4
    with pytest.raises(err, match="no label column"):
        gpu.search_batch_by_label_box64(Q, 10, 64, columns, lo, hi)
    gpu.set_label_column64(0, 0, shifted(cols[0], 0))  # the other width now, the same values
    gpu.set_label_column64(2, 0, cols[2])
    again = gpu.search_batch_by_label_box64(Q, 10, 64, columns, lo, hi, "exact")
    assert_same(again[:3], ref[:3], "after save and load")
    check(gpu, Q, 10, 64, {0: shifted(cols[0], 0), 2: cols[2]}, columns, lo, hi, 100, "loaded and labelled again", modes=("auto",))


# ------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals(base):
    g, Q = base.gpu, np.ascontiguousarray(base.Q[:4])
    lo, hi = np.zeros((4, 2), dtype=np.uint64), np.full((4, 2), BASE + 5000, dtype=np.uint64)
    err = gc.pkg().VssError
    out = np.full((4, 10), -1, dtype=np.int64)
    cnt = np.zeros(4, dtype=np.uint32)

    def call(lib_index, nq, k, columns, n_columns, p_lo, p_hi, mode):
        """the C entry point itself; returns (status, message)"""
        cols = None if columns is None else np.asarray(columns, dtype=np.uint32)
        rc = lib_index.lib.vss_search_batch_by_label_box64(lib_index.h, Q.ctypes.data, nq, k, 64,
                                                           None if cols is None else cols.ctypes.data, n_columns, p_lo, p_hi, mode, 0,
                                                           out.ctypes.data, None, cnt.ctypes.data, None)
        return rc, lib_index.lib.vss_last_error(lib_index.h)

    L, H = lo.ctypes.data, hi.ctypes.data
    bare = gc.gpu_index(base.dim, base.metric)
    # the widths: a setter of the other width on a column that has cells names BOTH widths, in both directions, column 0 and
    # set_labels included; nothing changes
    assert [g.label_column_width(c) for c in (0, 1, 3)] == [32, 64, 32]
    with pytest.raises(err, match="(?s)64-bit.*32-bit"):
        g.set_label_column(1, 0, np.zeros(3, dtype=np.uint32))
    with pytest.raises(err, match="(?s)32-bit.*64-bit"):
        g.set_label_column64(3, 0, np.zeros(3, dtype=np.uint64))
    with pytest.raises(err, match="(?s)32-bit.*64-bit"):
        g.set_label_column64(0, 0, np.zeros(3, dtype=np.uint64))
    bare.set_label_column64(0, 0, np.arange(10, dtype=np.uint64))
    with pytest.raises(err, match="(?s)64-bit.*32-bit"):
        bare.set_labels(0, np.zeros(3, dtype=np.uint32))
    assert [g.label_column_width(c) for c in (0, 1, 3)] == [32, 64, 32] and bare.label_column_width(0) == 64
    assert g.label_column_rows(1) == 9001 and bare.labelled_rows() == 10
    # the four existing calls by label refuse a column that is 64 bits wide
    want = np.zeros(4, dtype=np.uint32)
    for mode in MODES:
        with pytest.raises(err, match="64-bit"):
            bare.search_batch_by_label(Q, 10, 64, want, mode)
        with pytest.raises(err, match="64-bit"):
            bare.search_batch_by_label_range(Q, 10, 64, want, want, mode)
        with pytest.raises(err, match="64-bit"):
            bare.search_batch_by_label_set(Q, 10, 64, want.reshape(4, 1), mode)
        with pytest.raises(err, match="column 1 holds 64-bit"):
            g.search_batch_by_label_box(Q, 10, 64, [0, 1], lo.astype(np.uint32), lo.astype(np.uint32), mode)
    bare.clear_label_column(0)
    assert bare.label_column_width(0) == 0
    # 1. the mode, first
    for mode in (3, -1, 255):
        with pytest.raises(err, match="mode"):
            g.search_batch_by_label_box64(Q, 10, 64, [1, 0], lo, hi, mode)
        for index in (g, bare):
            rc, msg = call(index, 4, 10, None, 0, None, None, mode)
            assert rc != 0 and b"mode" in msg
    # 2. n_columns 0 or 5, before the NULL columns pointer
    for m in (0, 5, 1 << 40):
        rc, msg = call(g, 4, 10, None, m, L, H, 2)
        assert rc != 0 and b"n_columns" in msg
    rc, msg = call(g, 4, 10, None, 2, L, H, 2)
    assert rc != 0 and b"null columns" in msg
    # 3. a column >= 4, or one named twice, before NULL ends
    rc, msg = call(g, 4, 10, [1, 4], 2, None, None, 2)
    assert rc != 0 and b"column 4" in msg
    rc, msg = call(g, 4, 10, [3, 1, 3], 3, None, None, 2)
    assert rc != 0 and b"column 3 is named twice" in msg
    with pytest.raises(err, match="column 1 is named twice"):
        g.search_batch_by_label_box64(Q, 10, 64, [1, 1], lo, hi)
    # 4. NULL ends with queries to answer, before the column that was never set
    for p_lo, p_hi in ((None, H), (L, None), (None, None)):
        for mode in (0, 1, 2):
            rc, msg = call(bare, 4, 10, [1, 0], 2, p_lo, p_hi, mode)
            assert rc != 0 and b"null lo / hi" in msg
    # 5. a named column that was never set, with its number
    for mode in MODES:
        with pytest.raises(err, match="no label column 1"):
            bare.search_batch_by_label_box64(Q, 10, 64, [1, 0], lo, hi, mode)
    bare.set_label_column64(1, 0, np.zeros(10, dtype=np.uint64))
    with pytest.raises(err, match="no label column 0"):
        bare.search_batch_by_label_box64(Q, 10, 64, [1, 0], lo, hi)
    # the column calls refuse a column >= 4 too
    with pytest.raises(err, match="column 4"):
        g.set_label_column64(4, 0, np.zeros(3, dtype=np.uint64))
    assert g.label_column_width(4) == 0
    # the two no-ops: no queries (nothing to read), k == 0
    assert call(g, 0, 10, [1, 0], 2, None, None, 2)[0] == 0
    assert call(g, 4, 0, [1, 0], 2, L, H, 2)[0] == 0
    assert np.all(out == -1) and np.all(cnt == 0)  # nothing was written by any of them
    base.check(Q, 10, 64, [1, 0], lo, hi, 1500, "after the refusals")
