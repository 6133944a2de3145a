"""-m gpu: vss_search_batch_by_label_set_box — a per-query IN-list on one resident label column inside a box of inclusive ranges
with 64-bit ends over up to three more, columns of either width, mixed (csrc/label_filter.h; the walkers' admission in
csrc/hnsw_kernels.h, the listing kernels in csrc/exact_filtered_kernels.h).

Contract, and the only yardstick here: form the n_queries x (w + 2m) matrix of 64-bit words whose row q is (sets[q,0], ...,
sets[q,w-1], lo[q,0], hi[q,0], lo[q,1], hi[q,1], ...).  Its distinct RAW rows, ascending lexicographically as unsigned 64-bit
words (nothing canonicalised), are the groups; bitmap g has bit r set iff r is below the rows of the set column and of every range
column, the widened cell of the set column is not NO_LABEL64 and is one of the row's words, and every range column's widened cell
is not NO_LABEL64 and lies within its ends; n_bits is the smallest of those row counts.  The call in mode graph / exact / auto
returns cell for cell — row ids, f32 distance bits, counts, routes — what the bitmap call of that mode returns for that table, and
leaves the same counters behind.  No tolerance, no cell left out.
"""
import numpy as np
import pytest

import gpu_common as gc
from test_gpu_exact_filtered import _bitmap, _words, assert_same, keys_against_slot_order
from test_gpu_label_box64 import BASE, NO_LABEL64, T32, TOP64, set_column, shifted, widen
from test_gpu_label_search import MODES, NO_LABEL, assert_nothing, bitmap_call, build, counters

pytestmark = pytest.mark.gpu

PAD = NO_LABEL64


def padded64(rows, width):
    """the matrix of a call: every row's words, then NO_LABEL64 up to `width`"""
    m = np.full((len(rows), width), PAD, dtype=np.uint64)
    for q, r in enumerate(rows):
        m[q, :len(r)] = np.asarray(r, dtype=np.uint64)
    return m


def ends(lo, hi, nq, m):
    """the call's two matrices, nq x m (m may be 0)"""
    if m == 0:
        return np.zeros((nq, 0), dtype=np.uint64), np.zeros((nq, 0), dtype=np.uint64)
    return (np.ascontiguousarray(np.asarray(lo, dtype=np.uint64).reshape(nq, m)),
            np.ascontiguousarray(np.asarray(hi, dtype=np.uint64).reshape(nq, m)))


def set_mask(cols, set_col, words, n_bits):
    cell = widen(cols[set_col][:n_bits])
    return (cell != TOP64) & np.isin(cell, np.asarray(words, dtype=np.uint64))


def range_mask(cols, columns, lo_row, hi_row, n_bits):
    mask = np.ones(n_bits, dtype=bool)
    for c, a, b in zip(columns, lo_row, hi_row):
        cell = widen(cols[c][:n_bits])
        mask &= (cell != TOP64) & (np.uint64(a) <= cell) & (cell <= np.uint64(b))
    return mask


def admitted(cols, set_col, words, columns, lo_row, hi_row):
    """NumPy's restatement of the rule: the mask over row ids below the shortest of the set column and the range columns"""
    n_bits = min(len(cols[c]) for c in [set_col] + list(columns))
    return set_mask(cols, set_col, words, n_bits) & range_mask(cols, columns, lo_row, hi_row, n_bits)


def derived_table(cols, set_col, sets, columns, lo, hi):
    """the table of the contract: (bitmaps, n_bits, group_of)"""
    w, m = sets.shape[1], len(columns)
    rows = np.empty((len(sets), w + 2 * m), dtype=np.uint64)
    rows[:, :w] = sets
    rows[:, w::2], rows[:, w + 1::2] = lo, hi
    groups, group_of = np.unique(rows, axis=0, return_inverse=True)  # ascending lexicographically, as unsigned 64-bit words
    n_bits = min(len(cols[c]) for c in [set_col] + list(columns))
    bitmaps = np.zeros((len(groups), _words(n_bits)), dtype=np.uint64)
    for g, row in enumerate(groups):
        bitmaps[g] = _bitmap(n_bits, np.nonzero(admitted(cols, set_col, row[:w], columns, row[w::2], row[w + 1::2]))[0])
    return bitmaps, n_bits, group_of.reshape(-1).astype(np.uint32)


def check(gpu, Q, k, ef, cols, set_col, sets, columns, lo, hi, route_c, what, modes=MODES):
    """every mode against the bitmap call of that mode on the derived table: answers, routes, counters.  Returns
    {mode: (the call's answer, the bitmap call's counters)}"""
    columns = list(columns)
    for c in [set_col] + columns:
        assert gpu.label_column_rows(c) == len(cols[c]), what
        assert gpu.label_column_width(c) == 8 * cols[c].dtype.itemsize, what
    sets = np.ascontiguousarray(sets, dtype=np.uint64)
    lo, hi = ends(lo, hi, len(Q), len(columns))
    table = derived_table(cols, set_col, sets, columns, lo, hi)
    out = {}
    for mode in modes:
        where = "%s, set column %d, range columns %r, mode %s, route_c %d" % (what, set_col, columns, mode, route_c)
        ref = bitmap_call(gpu, mode, Q, k, ef, table, route_c)
        ref_counters = counters(gpu, mode)
        got = gpu.search_batch_by_label_set_box(Q, k, ef, set_col, sets, columns, lo, hi, mode, route_c)
        got_counters = counters(gpu, mode)
        assert_same(got[:3], ref[:3], where)
        assert np.array_equal(got[3], ref[3]), where + ": routes"
        assert got_counters == ref_counters, where + ": counters %r, the bitmap call's %r" % (got_counters, ref_counters)
        out[mode] = (got, ref_counters)
    return out


def live_lengths(cols, set_col, sets, columns, keys, lo, hi):
    """rows each query's predicate admits among the live row ids `keys`"""
    n_bits = min(len(cols[c]) for c in [set_col] + list(columns))
    live = np.zeros(n_bits, dtype=bool)
    live[keys[keys < n_bits]] = True
    lo, hi = ends(lo, hi, len(sets), len(columns))
    return np.array([int((admitted(cols, set_col, s, columns, a, b) & live).sum()) for s, a, b in zip(sets, lo, hi)])


# ------------------------------------------------------------------------------------------------- 1. the mixed chunk
def mixed_chunk():
    """3000 rows, row id != slot (ids 2001 .. 5000).  Column 1, `grp`, 32 bits wide, 5001 cells: ten groups, 20 NULL cells.  Column
    3, `ts`, 64 bits wide, 4900 cells — the shorter one: ids from 4900 on have no cell — BASE + [0, 1000), 20 NULL cells.  204
    queries, eight distinct predicates, lists four words wide."""
    n, nq = 3000, 204
    keys = keys_against_slot_order(n, 5000)
    rng = np.random.default_rng(2310)
    grp = rng.integers(0, 10, 5001).astype(np.uint32)
    grp[rng.choice(np.arange(2001, 5001), 20, replace=False)] = NO_LABEL
    ts = rng.integers(0, 1000, 4900).astype(np.uint64) + np.uint64(BASE)
    ts[rng.choice(np.arange(2001, 4900), 20, replace=False)] = TOP64
    cols = {1: grp, 3: ts}
    predicates = [([1, 2, 3], BASE + 200, NO_LABEL64),          # no upper bound
                  ([3, 1, 2], BASE + 200, NO_LABEL64),          # a permuted duplicate of the first: another group, the same rows
                  ([], 0, NO_LABEL64),                          # all padding
                  ([4, 5], BASE + 600, BASE + 599),             # lo > hi
                  ([6, 6, 7], BASE + 100, BASE + 899),          # a repeated member
                  ([0, 1, 2, 3], BASE, BASE + 499),
                  ([8], BASE + 50, NO_LABEL64),
                  ([9, T32 + 1], BASE + 500, NO_LABEL64)]       # a word beyond the 32-bit column's cells beside a member
    pick = rng.integers(0, len(predicates), nq)
    pick[:len(predicates)] = np.arange(len(predicates))
    sets = padded64([predicates[p][0] for p in pick], 4)
    lo = np.array([[predicates[p][1]] for p in pick], dtype=np.uint64)
    hi = np.array([[predicates[p][2]] for p in pick], dtype=np.uint64)
    return keys, cols, sets, lo, hi, pick


@pytest.mark.parametrize("metric,dim", [("l2sq", 100), ("cosine", 100), ("ip", 100), ("l2sq", 3), ("l2sq", 768)])
def test_mixed_chunk(metric, dim):
    n, k, ef = 3000, 10, 64
    keys, cols, sets, lo, hi, pick = mixed_chunk()
    nq = len(sets)
    # on the NumPy restatement, before any GPU call
    assert cols[1].dtype == np.uint32 and cols[3].dtype == np.uint64 and nq == 204
    assert len(np.unique(np.concatenate([sets, lo, hi], axis=1), axis=0)) == 8
    n_bits = 4900
    live = np.zeros(n_bits, dtype=bool)
    live[keys[keys < n_bits]] = True
    lens = live_lengths(cols, 1, sets, [3], keys, lo, hi)
    nothing = (pick == 2) | (pick == 3)
    assert np.array_equal(nothing, lens == 0)
    assert np.all(lens[~nothing] >= k)  # every non-empty predicate admits at least k rows
    for q in np.nonzero(~nothing)[0][:40]:
        by_set, by_range = set_mask(cols, 1, sets[q], n_bits) & live, range_mask(cols, [3], lo[q], hi[q], n_bits) & live
        assert (by_range & ~by_set).any(), "a row the set alone rejects"   # a kernel that ignores the set admits it
        assert (by_set & ~by_range).any(), "a row the range alone rejects"  # a kernel that ignores the range admits it
    assert np.array_equal(lens[pick == 0], lens[pick == 1][:1].repeat((pick == 0).sum()))  # order inside a list changes nothing
    X, Q = gc.make_data(n, dim, metric, 2300 + dim, nq=nq)
    gpu = build(dim, metric, X, keys)
    gpu.set_label_column(1, 0, cols[1])
    gpu.set_label_column64(3, 0, cols[3])
    what = "%s dim %d" % (metric, dim)
    # the rule (csrc/filter_route.h): a group is scanned iff len^2 * 64 <= C * limit * L; C = 100 puts the boundary near 547 rows
    got = check(gpu, Q, k, ef, cols, 1, sets, [3], lo, hi, 100, what)
    for mode in MODES:
        assert_nothing(got[mode][0], nothing, what + " " + mode)
    assert np.array_equal(got["exact"][0][2], np.minimum(lens, k))  # the scan returns min(k, admitted live rows)
    route = got["auto"][0][3]
    assert set(route.tolist()) == {0, 1}
    assert np.array_equal(route, np.where(lens.astype(np.int64) ** 2 * 64 <= 100 * max(k, ef) * n, 1, 0).astype(np.uint8))
    # the admitted ids carry a member of the list and a timestamp within the ends
    for mode in MODES:
        ids = got[mode][0][0]
        for q in range(0, nq, 17):
            mine = ids[q][ids[q] >= 0]
            assert np.all(admitted(cols, 1, sets[q], [3], lo[q], hi[q])[mine]), (mode, q)


# ------------------------------------------------------------------------------------------------- 2. widths, columns, slots
class Slots:
    """2000 x 16, row id != slot (ids 2001 .. 4000).  Every slot's data exists in both widths: narrow, values 0 .. 39 with ten NULL
    cells, and wide, the same moved up by 2^32 - 20, so that its cells lie on both sides of 2^32.  Slot 2 is the shorter one."""

    def __init__(self):
        self.n, self.dim = 2000, 16
        self.X, self.Q = gc.make_data(self.n, self.dim, "l2sq", 2320, nq=12)
        self.keys = keys_against_slot_order(self.n, 4000)
        rng = np.random.default_rng(2321)
        self.narrow, self.wide = {}, {}
        for c in range(4):
            column = rng.integers(0, 40, 3900 if c == 2 else 4001).astype(np.uint32)
            column[rng.choice(np.arange(2001, len(column)), 10, replace=False)] = NO_LABEL
            self.narrow[c], self.wide[c] = column, shifted(column, T32 - 20)
        self.gpu = build(self.dim, "l2sq", self.X, self.keys, M=8, M0=16, efc=32)
        self.cols = {}

    def use(self, c, wide):
        """slot c holds its data `wide` bits wide"""
        column = self.wide[c] if wide else self.narrow[c]
        if c in self.cols and self.cols[c].dtype != column.dtype:
            self.gpu.clear_label_column(c)
        if c not in self.cols or self.cols[c].dtype != column.dtype:
            set_column(self.gpu, c, column)
        self.cols[c] = column
        return np.uint64(T32 - 20 if wide else 0)


@pytest.fixture(scope="module")
def slots():
    return Slots()


WIDTHS = [1, 2, 3, 4, 5, 31, 32]


def slot_plan(i, m):
    """for set width WIDTHS[i] and m range columns: (set slot, is it wide, range slots, are they wide)"""
    set_slot = (i + m) % 4
    others = [(set_slot + 1 + j) % 4 for j in range(m)]
    return set_slot, (i + (i + m) // 4) % 2 == 1, others, [(i + j + m) % 2 == 0 for j in range(m)]


def test_slot_plan_covers_every_slot_of_each_width():
    seen = {(slot_plan(i, m)[0], slot_plan(i, m)[1]) for i in range(len(WIDTHS)) for m in range(4)}
    assert seen == {(s, w) for s in range(4) for w in (False, True)}


@pytest.mark.parametrize("i", range(len(WIDTHS)))
def test_set_widths_and_range_columns(slots, i):
    """set widths with odd and even padding and the cap, 0 to 3 range columns, the set column in every slot and of each width.  The
    hit sits in word 0 only, in the last word only, or among junk no row holds; some lists are padded"""
    width, nq, k = WIDTHS[i], 12, 10
    rng = np.random.default_rng(2330 + i)
    for m in range(4):
        set_slot, set_wide, others, others_wide = slot_plan(i, m)
        base = slots.use(set_slot, set_wide)
        bases = [slots.use(c, w) for c, w in zip(others, others_wide)]
        junk = np.uint64(1000) + base + np.arange(width, dtype=np.uint64)
        sets = np.tile(junk, (nq, 1))
        for q in range(nq):
            members = rng.choice(40, min(width, 1 + q % 5), replace=False).astype(np.uint64) + base
            if q % 4 == 0:
                sets[q, 0] = members[0]                      # the hit in word 0 only
            elif q % 4 == 1:
                sets[q, width - 1] = members[0]              # ... in the last word only
            elif q % 4 == 2:
                sets[q] = PAD
                sets[q, :len(members)] = members             # a padded list
            else:
                sets[q, rng.choice(width, len(members), replace=False)] = members  # members among junk
        lo = np.stack([b + rng.integers(0, 15, nq).astype(np.uint64) for b in bases], axis=1) if m else None
        hi = np.stack([b + rng.integers(25, 40, nq).astype(np.uint64) for b in bases], axis=1) if m else None
        if m:
            hi[5, m - 1] = TOP64  # no upper bound in the last range column
        what = "width %d, %d range columns" % (width, m)
        got = check(slots.gpu, slots.Q, k, 64, slots.cols, set_slot, sets, others, lo, hi, 40, what)
        lens = live_lengths(slots.cols, set_slot, sets, others, slots.keys, lo, hi)
        assert np.array_equal(got["exact"][0][2], np.minimum(lens, k)), what
        assert lens.max() > 0, what


# ------------------------------------------------------------------------------------------------- 3. high and low words
def test_words_that_differ_in_one_half():
    """a 64-bit set column whose cells are {7, 9} x {0, 2^32, 2^33}: a word admits exactly the rows of its own value, whichever half
    it shares with another; on a 32-bit column a word of 2^32 or above and the word 0xFFFFFFFF admit nothing"""
    n, dim, k = 2000, 16, 10
    X, Q = gc.make_data(n, dim, "l2sq", 2340, nq=8)
    keys = keys_against_slot_order(n, 4000)
    rng = np.random.default_rng(2341)
    low = rng.choice(np.array([7, 9], dtype=np.uint64), 4001)
    high = rng.integers(0, 3, 4001).astype(np.uint64)
    wide = low + (high << np.uint64(32))
    narrow = low.astype(np.uint32)
    narrow[rng.choice(np.arange(2001, 4001), 30, replace=False)] = NO_LABEL
    cols = {2: wide, 0: narrow}
    gpu = build(dim, "l2sq", X, keys, M=8, M0=16, efc=32)
    gpu.set_label_column64(2, 0, wide)
    gpu.set_label_column(0, 0, narrow)
    sets = padded64([[T32 + 7], [2 * T32 + 7], [T32 + 9], [7], [T32 + 7, 2 * T32 + 9], [3 * T32 + 7], [T32 + 8], [9, T32 + 9]], 2)
    got = check(gpu, Q, k, 64, cols, 2, sets, [], None, None, 30, "one half")
    lens = live_lengths(cols, 2, sets, [], keys, None, None)
    for q in range(8):
        words = sets[q][sets[q] != PAD]
        assert lens[q] == np.isin(wide[keys], words).sum()
    assert lens[5] == 0 and lens[6] == 0 and np.all(lens[[0, 1, 2, 3, 4, 7]] > 0)
    for mode in MODES:
        ids = got[mode][0][0]
        for q in (0, 1, 2, 3, 4, 7):
            mine = ids[q][ids[q] >= 0]
            assert len(mine) and np.all(np.isin(wide[mine], sets[q][sets[q] != PAD])), (mode, q)  # exactly its own rows
        assert_nothing(got[mode][0], np.array([5, 6]), mode)
    assert np.array_equal(got["exact"][0][2], np.minimum(lens, k))
    # the 32-bit column: 2^32 + 7 must not match the cell 7, and 0xFFFFFFFF must not match the NULL cell
    sets = padded64([[T32 + 7], [0xFFFFFFFF], [7], [T32 + 7, 9], [0xFFFFFFFF, T32 + 9], [2 * T32 + 9]], 2)
    got = check(gpu, Q[:6], k, 64, cols, 0, sets, [], None, None, 30, "narrow column")
    lens = live_lengths(cols, 0, sets, [], keys, None, None)
    assert list(lens == 0) == [True, True, False, False, True, True] and (narrow[keys] == NO_LABEL).sum() > 0
    for mode in MODES:
        assert_nothing(got[mode][0], np.array([0, 1, 4, 5]), mode)
        assert np.all(narrow[got[mode][0][0][3][:k]] == 9), mode


# ------------------------------------------------------------------------------------------------- 6. kernel shapes
class Base:
    """3000 x 16, row id != slot (ids 6001 .. 9000), three columns by row id: 0 a group of ten values, 32 bits wide; 1 a timestamp
    BASE + [0, 10000), 64 bits wide; 3 a price below 1000, 32 bits wide; three NULL cells in each"""

    def __init__(self):
        self.metric, self.n, self.dim = "l2sq", 3000, 16
        self.X, self.Q = gc.make_data(self.n, self.dim, self.metric, 2360, nq=300)
        self.keys = keys_against_slot_order(self.n, 9000)
        rng = np.random.default_rng(2361)
        self.cols, self.by_slot = {}, {}
        for c, top in ((0, 10), (1, 10000), (3, 1000)):
            by_slot = rng.integers(0, top, self.n).astype(np.uint32)
            by_slot[rng.choice(self.n, 3, replace=False)] = NO_LABEL
            column = np.full(9001, NO_LABEL, dtype=np.uint32)
            column[self.keys] = by_slot
            self.cols[c] = shifted(column, BASE) if c == 1 else column
            self.by_slot[c] = by_slot
        self.gpu = build(self.dim, self.metric, self.X, self.keys)
        for c in self.cols:
            set_column(self.gpu, c, self.cols[c])

    def check(self, Q, k, ef, set_col, sets, columns, lo, hi, route_c, what, modes=MODES):
        return check(self.gpu, Q, k, ef, self.cols, set_col, sets, columns, lo, hi, route_c, what, modes)


@pytest.fixture(scope="module")
def base():
    return Base()


# (groups, since, until): 2400 rows, 960, 2400 in another order, some 30, a handful, none, none
SEVEN = [([0, 1, 2, 3, 4, 5, 6, 7], 0, NO_LABEL64), ([0, 1, 2, 3], BASE + 2000, NO_LABEL64), ([5, 6, 7, 8, 9, 4, 3, 2], BASE, NO_LABEL64),
         ([9], BASE + 1000, BASE + 1999), ([1, 2], BASE + 5000, BASE + 5099), ([], 0, NO_LABEL64), ([0, 1, 2, 3, 4, 5, 6, 7], BASE + 9, BASE + 2)]


def seven(nq):
    pick = np.arange(nq) % 7
    return (padded64([SEVEN[p][0] for p in pick], 8), np.array([[SEVEN[p][1]] for p in pick], dtype=np.uint64),
            np.array([[SEVEN[p][2]] for p in pick], dtype=np.uint64))


@pytest.mark.parametrize("ef", [64, 300, 600])  # lists in registers (2 and 8 per lane) and outside them
def test_list_widths(base, ef):
    sets, lo, hi = seven(21)
    route_c = {64: 480, 300: 160, 600: 80}[ef]  # len^2 * 64 <= route_c * limit * 3000 ends near 1500 rows at each limit
    got = base.check(base.Q[:21], 100, ef, 0, sets, [1], lo, hi, route_c, "ef %d" % ef)
    assert (got["graph"][1]["shape"][4] != 0) == (ef == 600)  # beyond 512 the list has left the registers (the bitmap call's shape)
    assert set(got["auto"][0][3].tolist()) == {0, 1}


def test_one_query_takes_the_solo_kernel(base):
    for q, (groups, since) in enumerate([([0, 1, 2, 3, 4], BASE), ([7, 8, 9], BASE + 3000)]):
        sets, lo, hi = padded64([groups], 5), [[since]], [[NO_LABEL64]]
        got = base.check(base.Q[q:q + 1], 10, 64, 0, sets, [1], lo, hi, 1, "one query")
        assert got["graph"][1]["shape"][6] == 1 and got["graph"][0][2][0] == 10


@pytest.mark.parametrize("nq", [204, 300])  # the join's chunk; more than a launch of one query per compute unit
def test_host_batches(base, nq):
    rng = np.random.default_rng(2370 + nq)
    sets = np.full((nq, 8), PAD, dtype=np.uint64)
    for q in range(nq):  # one to eight groups this user may see ...
        mine = rng.choice(10, 1 + q % 8, replace=False)
        sets[q, :len(mine)] = mine
    lo = (rng.integers(0, 9000, (nq, 1)).astype(np.uint64) + np.uint64(BASE))  # ... AND ts >= since
    hi = np.full((nq, 1), TOP64, dtype=np.uint64)
    lo[::50], hi[::50] = BASE + 5, BASE + 1
    got = base.check(base.Q[:nq], 10, 64, 0, sets, [1], lo, hi, 300, "%d queries" % nq)
    assert set(got["auto"][0][3].tolist()) == {0, 1}


def test_rare_predicates_rerun(base):
    """predicates of a handful of rows and of one: the walk rejects nearly every row it meets, its pending candidates outgrow the
    register queue, and the queries are re-run through the unbounded one — reading the same table again, through a.work[idx]"""
    ts, grp = base.by_slot[1], base.by_slot[0]
    s = np.sort(ts[ts != NO_LABEL])
    at = int(np.nonzero((ts == s[1500]) & (grp != NO_LABEL))[0][0])
    few = ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9], BASE + int(s[500]), BASE + int(s[505]))
    one = ([int(grp[at])], BASE + int(ts[at]), BASE + int(ts[at]))
    sets = padded64([few[0], one[0]] * 8, 10)
    lo = np.array([[few[1]], [one[1]]] * 8, dtype=np.uint64)
    hi = np.array([[few[2]], [one[2]]] * 8, dtype=np.uint64)
    lens = live_lengths(base.cols, 0, sets[:2], [1], base.keys, lo[:2], hi[:2])
    assert 3 <= lens[0] <= 9 and 1 <= lens[1] <= 3
    got = base.check(base.Q[:16], 10, 64, 0, sets, [1], lo, hi, 1500, "rare predicates", modes=("graph",))
    _, _, cnt, _ = got["graph"][0]
    assert np.all(cnt[0::2] <= lens[0]) and np.all(cnt[1::2] <= lens[1]) and cnt.sum() > 0  # (a walk may miss a row; it invents none)
    assert got["graph"][1]["stats"][3] > 0  # (the bitmap call's counter, and by check() this call's: queries were re-run)


def test_device_form(base):
    import torch
    nq, k = 35, 10
    Q = base.Q[:nq]
    sets, lo, hi = seven(nq)
    d_Q = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    d_sets = torch.from_numpy(sets.view(np.int64)).cuda()
    d_lo, d_hi = torch.from_numpy(lo.view(np.int64)).cuda(), torch.from_numpy(hi.view(np.int64)).cuda()
    for mode in MODES:
        ref = base.check(Q, k, 64, 0, sets, [1], lo, hi, 480, "host form", modes=(mode,))[mode][0]
        ref0 = base.check(Q, k, 64, 0, sets, [], None, None, 480, "host form, no range column", modes=(mode,))[mode][0]
        for bare in (False, True):
            for m, want in ((1, ref), (0, ref0)):
                d_keys = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
                d_dist = None if bare else torch.zeros((nq, k), dtype=torch.float32, device="cuda")
                d_cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
                d_route = None if bare else torch.full((nq,), 9, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                base.gpu.search_batch_by_label_set_box_device(d_Q.data_ptr(), nq, k, 64, 0, d_sets.data_ptr(), 8, [1][:m],
                                                              d_lo.data_ptr() if m else None, d_hi.data_ptr() if m else None,
                                                              d_keys.data_ptr(), None if bare else d_dist.data_ptr(), d_cnt.data_ptr(),
                                                              None if bare else d_route.data_ptr(), mode, 480)
                assert np.array_equal(d_keys.cpu().numpy(), want[0]), mode
                assert np.array_equal(d_cnt.cpu().numpy().astype(np.uint32), want[2]), mode
                if not bare:
                    assert np.array_equal(d_dist.cpu().numpy().view(np.uint32), want[1].view(np.uint32)), mode
                    assert np.array_equal(d_route.cpu().numpy(), want[3]), mode


# ------------------------------------------------------------------------------------------------- 4. equivalences
def test_no_range_column_on_narrow_column_0_is_the_set_call(base):
    """(a) n_columns = 0, set column 0 narrow, words below 2^32, padding NO_LABEL mapped to NO_LABEL64: answers AND counters of
    vss_search_batch_by_label_set"""
    nq = 21
    sets64 = seven(nq)[0]
    sets32 = np.where(sets64 == PAD, np.uint64(NO_LABEL), sets64).astype(np.uint32)
    for route_c in (480, 3):
        for mode in MODES:
            where = "mode %s, route_c %d" % (mode, route_c)
            ref = base.gpu.search_batch_by_label_set(base.Q[:nq], 10, 64, sets32, mode, route_c)
            ref_counters = counters(base.gpu, mode)
            got = base.gpu.search_batch_by_label_set_box(base.Q[:nq], 10, 64, 0, sets64, mode=mode, route_c=route_c)
            assert_same(got[:3], ref[:3], where)
            assert np.array_equal(got[3], ref[3]), where + ": routes"
            assert counters(base.gpu, mode) == ref_counters, where
    base.check(base.Q[:nq], 10, 64, 0, sets64, [], None, None, 480, "no range column against the bitmaps")


def test_width_one_is_the_box64_call_with_the_set_column_first(base):
    """(b) set_width = 1: answers and counters of vss_search_batch_by_label_box64 with the set column named FIRST and [v, v]"""
    nq = 24
    rng = np.random.default_rng(2380)
    v = rng.integers(0, 11, (nq, 1)).astype(np.uint64)  # (group 10 does not exist)
    v[3] = PAD
    lo = rng.integers(0, 5000, (nq, 2)).astype(np.uint64) + np.array([BASE, 0], dtype=np.uint64)
    hi = lo + np.array([4000, 600], dtype=np.uint64)
    hi[::5, 0] = TOP64
    for route_c in (100, 3):
        for mode in MODES:
            where = "mode %s, route_c %d" % (mode, route_c)
            ref = base.gpu.search_batch_by_label_box64(base.Q[:nq], 10, 64, [0, 1, 3], np.concatenate([v, lo], axis=1),
                                                       np.concatenate([v, hi], axis=1), mode, route_c)
            ref_counters = counters(base.gpu, mode)
            got = base.gpu.search_batch_by_label_set_box(base.Q[:nq], 10, 64, 0, v, [1, 3], lo, hi, mode, route_c)
            assert_same(got[:3], ref[:3], where)
            assert np.array_equal(got[3], ref[3]), where + ": routes"
            assert counters(base.gpu, mode) == ref_counters, where
    assert got[2].sum() > 0 and got[2][3] == 0


@pytest.mark.parametrize("w", [1, 2, 5, 8])
def test_consecutive_values_are_the_range(base, w):
    """(c) {a, ..., a + w - 1} admits what [a, a + w - 1] admits: the answers of the box64 call (the groups differ)"""
    nq = 24
    rng = np.random.default_rng(2390 + w)
    a = rng.integers(0, 10, nq).astype(np.uint64)
    sets = a[:, None] + np.arange(w, dtype=np.uint64)[None, :]
    sets = sets[:, rng.permutation(w)]
    since = rng.integers(0, 8000, nq).astype(np.uint64) + np.uint64(BASE)
    lo, hi = np.stack([a, since], axis=1), np.stack([a + np.uint64(w - 1), np.full(nq, TOP64)], axis=1)
    for mode in ("exact", "graph"):
        ref = base.gpu.search_batch_by_label_box64(base.Q[:nq], 10, 64, [0, 1], lo, hi, mode)
        got = base.gpu.search_batch_by_label_set_box(base.Q[:nq], 10, 64, 0, sets, [1], lo[:, 1:], hi[:, 1:], mode)
        assert_same(got[:3], ref[:3], "w %d, mode %s" % (w, mode))
    assert got[2].sum() > 0


def test_range_column_order_changes_no_answer(base):
    """(d)"""
    nq = 21
    sets = seven(nq)[0]
    rng = np.random.default_rng(2395)
    lo = rng.integers(0, 400, (nq, 2)).astype(np.uint64) + np.array([BASE, 0], dtype=np.uint64)
    hi = np.stack([np.full(nq, TOP64), lo[:, 1] + np.uint64(500)], axis=1)
    for mode in MODES:
        a = base.gpu.search_batch_by_label_set_box(base.Q[:nq], 10, 64, 0, sets, [1, 3], lo, hi, mode, 100)
        b = base.gpu.search_batch_by_label_set_box(base.Q[:nq], 10, 64, 0, sets, [3, 1], lo[:, ::-1], hi[:, ::-1], mode, 100)
        assert_same(a[:3], b[:3], "range columns swapped, mode " + mode)
        assert np.array_equal(a[3], b[3]), mode
    assert a[2].sum() > 0


# ------------------------------------------------------------------------------------------------- 5. listing edges
@pytest.mark.parametrize("n", [1, 511, 512, 513, 1025])  # FL_WAVE_SLOTS = 512
def test_listing_edges(n):
    """column 2's cell is the slot modulo 64, 32 bits wide, and column 1's BASE + the SLOT, 64 bits wide (a listing wave owns 512
    consecutive slots, a row of it 64): a list's words name lanes, a range's ends blocks and rows of them — lanes 0 and 63 of every
    row, both sides of a row's edge and of the block's, the last slot only"""
    dim = 8
    keys = keys_against_slot_order(n, 2000)
    slot = np.arange(n, dtype=np.uint32)
    cols = {2: np.full(2001, NO_LABEL, dtype=np.uint32), 1: np.full(2001, TOP64, dtype=np.uint64)}
    cols[2][keys], cols[1][keys] = slot % 64, slot.astype(np.uint64) + np.uint64(BASE)
    last = n - 1
    predicates = [([0], 0, None), ([63], 0, None), ([0, 63], 0, 511), ([63, 0], 64, 127), (list(range(64)), 64, 127), ([60, 61, 62, 63, 0, 1], 60, 70),
                  ([0, 1, 2], 448, 511), ([63], 511, 511), ([63, 0], 511, 512), ([0], 512, 512), ([10, 20, 30], 500, 530), (list(range(32)), 0, 511),
                  (list(range(32, 64)), 512, 1023), ([63, 0], 1023, 1024), ([0], 1024, 1024), ([last % 64], last, last), ([last % 64], last, None),
                  ([0, 1], n, None), ([], 0, None), ([5], 5, 4), ([31, 32], 100, 900), (list(range(0, 64, 2)), 0, last)]
    predicates = [(p[0][:32], p[1], p[2]) for p in predicates]  # (the cap: 32 words)
    nq = len(predicates)
    X, Q = gc.make_data(n, dim, "l2sq", 2400 + n, nq=nq)
    sets = padded64([p[0] for p in predicates], 32)
    lo = np.array([[BASE + p[1]] for p in predicates], dtype=np.uint64)
    hi = np.array([[TOP64 if p[2] is None else BASE + p[2]] for p in predicates], dtype=np.uint64)
    gpu = build(dim, "l2sq", X, keys, M=4, M0=8, efc=16)
    gpu.set_label_column(2, 0, cols[2])
    gpu.set_label_column64(1, 0, cols[1])
    got = check(gpu, Q, 10, 64, cols, 2, sets, [1], lo, hi, 1, "n %d" % n, modes=("exact", "auto"))
    cnt = got["exact"][0][2]
    a, b = slot.astype(np.int64), (slot % 64).astype(np.int64)
    expect = np.array([int((np.isin(b, p[0]) & (p[1] <= a) & (a <= (1 << 40 if p[2] is None else p[2]))).sum()) for p in predicates])
    assert np.array_equal(cnt, np.minimum(expect, 10))
    assert cnt[15] == 1 and got["exact"][0][0][15][0] == keys[n - 1]  # the predicate of the last slot only: that row
    distinct = {(tuple(p[0]), p[1], p[2]): e for p, e in zip(predicates, expect)}
    assert got["exact"][1]["exact"][0] == sum(distinct.values())  # listed: every group's rows, overlaps counted per group


# ------------------------------------------------------------------------------------------------- 7. lifecycle
def test_lifecycle():
    n, dim, nq = 3000, 16, 24
    rng = np.random.default_rng(2410)
    X, Q = gc.make_data(n + 400, dim, "l2sq", 2411, nq=nq)
    keys = keys_against_slot_order(n, 5000)            # ids 2001 .. 5000
    new_keys = np.arange(400, dtype=np.int64) + 100    # the rows added later: ids 100 .. 499, labelled from the start
    grp = rng.integers(0, 10, 5001).astype(np.uint32)
    ts = rng.integers(0, 1000, 5001).astype(np.uint32)
    for column in (grp, ts):
        column[rng.choice(5001, 50, replace=False)] = NO_LABEL
    cols = {0: grp, 2: shifted(ts, BASE)}
    predicates = [([1, 2, 3], 0, 499), ([4], 100, 300), ([5, 6, 7, 8], 250, 800), ([0, 9], 900, None), ([], 0, None), ([1, 2, 3], 7, 7)] * 4
    sets = padded64([p[0] for p in predicates], 4)
    lo = np.array([[BASE + p[1]] for p in predicates], dtype=np.uint64)
    hi = np.array([[TOP64 if p[2] is None else BASE + p[2]] for p in predicates], dtype=np.uint64)
    gpu = build(dim, "l2sq", X[:n], keys, capacity=n + 400, M=8, M0=16, efc=32)
    gpu.set_labels(0, cols[0])
    gpu.set_label_column64(2, 0, cols[2])
    check(gpu, Q, 10, 64, cols, 0, sets, [2], lo, hi, 100, "built")
    # rows removed, rows added into their slots, compaction: the columns are by row id and need no call
    gone = rng.choice(n, 700, replace=False)
    assert gpu.remove(keys[gone]) == 700
    got = check(gpu, Q, 10, 64, cols, 0, sets, [2], lo, hi, 100, "700 removed")
    assert not np.any(np.isin(got["exact"][0][0], keys[gone]))
    gpu.add(new_keys, X[n:])
    got = check(gpu, Q, 10, 64, cols, 0, sets, [2], lo, hi, 100, "400 added into reused slots")
    assert np.any(np.isin(got["exact"][0][0], new_keys))
    gpu.compact()
    check(gpu, Q, 10, 64, cols, 0, sets, [2], lo, hi, 100, "compacted")
    # a named column shorter than the others sets n_bits: row ids from 4000 on have no cell in column 3, set OR range column
    short = rng.integers(0, 4, 4000).astype(np.uint32)
    gpu.set_label_column(3, 0, short)
    cols[3] = short
    lo2, hi2 = np.concatenate([lo, np.zeros((nq, 1), np.uint64)], axis=1), np.concatenate([hi, np.full((nq, 1), 2, np.uint64)], axis=1)
    got = check(gpu, Q, 10, 64, cols, 0, sets, [2, 3], lo2, hi2, 100, "a shorter range column")
    assert got["exact"][0][2].sum() > 0 and np.all(got["exact"][0][0] < 4000)
    short_sets = padded64([[0, 1], [2], [3, 0, 1]] * 8, 3)
    got = check(gpu, Q, 10, 64, cols, 3, short_sets, [0], np.zeros((nq, 1), np.uint64), np.full((nq, 1), 8, np.uint64), 100,
                "a shorter set column")
    assert got["exact"][0][2].sum() > 0 and np.all(got["exact"][0][0] < 4000)
    # a named column cleared: "no label column" with its number, whichever role it had
    err = gc.pkg().VssError
    gpu.clear_label_column(2)
    with pytest.raises(err, match="no label column 2"):
        gpu.search_batch_by_label_set_box(Q, 10, 64, 0, sets, [2], lo, hi)
    with pytest.raises(err, match="no label column 2"):
        gpu.search_batch_by_label_set_box(Q, 10, 64, 2, sets)
    gpu.set_label_column64(2, 0, cols[2])
    ref = gpu.search_batch_by_label_set_box(Q, 10, 64, 0, sets, [2], lo, hi, "exact")
    # vss_load clears the columns; set again, the answers return
    blob = gpu.save()
    gpu.load(blob)
    assert [gpu.label_column_rows(c) for c in range(4)] == [0, 0, 0, 0]
    with pytest.raises(err, match="no label column 0"):
        gpu.search_batch_by_label_set_box(Q, 10, 64, 0, sets, [2], lo, hi)
    gpu.set_labels(0, cols[0])
    gpu.set_label_column64(2, 0, cols[2])
    again = gpu.search_batch_by_label_set_box(Q, 10, 64, 0, sets, [2], lo, hi, "exact")
    assert_same(again[:3], ref[:3], "after save and load")
    check(gpu, Q, 10, 64, {0: cols[0], 2: cols[2]}, 0, sets, [2], lo, hi, 100, "loaded and labelled again", modes=("auto",))


# ------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(base):
    g, Q = base.gpu, np.ascontiguousarray(base.Q[:4])
    sets = padded64([[0, 1], [2], [], [7, 3]], 4)
    lo, hi = np.zeros((4, 2), dtype=np.uint64), np.full((4, 2), BASE + 5000, dtype=np.uint64)
    err = gc.pkg().VssError
    out = np.full((4, 10), -1, dtype=np.int64)
    cnt = np.zeros(4, dtype=np.uint32)

    def call(index, nq, k, set_col, p_sets, width, columns, n_columns, p_lo, p_hi, mode):
        """the C entry point itself; returns (status, message)"""
        cols = None if columns is None else np.asarray(columns, dtype=np.uint32)
        rc = index.lib.vss_search_batch_by_label_set_box(index.h, Q.ctypes.data, nq, k, 64, set_col, p_sets, width,
                                                         None if cols is None else cols.ctypes.data, n_columns, p_lo, p_hi, mode, 0,
                                                         out.ctypes.data, None, cnt.ctypes.data, None)
        return rc, index.lib.vss_last_error(index.h)

    S, L, H = sets.ctypes.data, lo.ctypes.data, hi.ctypes.data
    bare = gc.gpu_index(base.dim, base.metric)
    # 1. the mode, first: before a width of 0, too many columns, null pointers, a bad column, an index without columns
    for mode in (3, -1, 255):
        with pytest.raises(err, match="mode"):
            g.search_batch_by_label_set_box(Q, 10, 64, 0, sets, [1, 3], lo, hi, mode)
        for index in (g, bare):
            rc, msg = call(index, 4, 10, 9, None, 0, None, 7, None, None, mode)
            assert rc != 0 and b"mode" in msg
    # 2. set_width 0 or above 32, before n_columns
    for width in (0, 33, 1 << 20):
        rc, msg = call(g, 4, 10, 9, None, width, None, 7, None, None, 2)
        assert rc != 0 and b"set_width" in msg
    # 3. n_columns above 3, before the null pointers
    for m in (4, 5, 1 << 40):
        rc, msg = call(g, 4, 10, 9, None, 4, None, m, None, None, 2)
        assert rc != 0 and b"n_columns" in msg
    # 4. null sets, null lo / hi with range columns, before a bad column
    rc, msg = call(g, 4, 10, 9, None, 4, [1, 9], 2, L, H, 2)
    assert rc != 0 and b"null sets" in msg
    for p_lo, p_hi in ((None, H), (L, None), (None, None)):
        rc, msg = call(g, 4, 10, 9, S, 4, [1, 9], 2, p_lo, p_hi, 2)
        assert rc != 0 and b"null lo / hi" in msg
    ran = g.lib.vss_search_batch_by_label_set_box(g.h, Q.ctypes.data, 4, 10, 64, 0, S, 4, None, 0, None, None, 2, 0,
                                                  np.empty((4, 10), np.int64).ctypes.data, None, np.empty(4, np.uint32).ctypes.data, None)
    assert ran == 0  # (without range columns lo and hi are not read)
    # 5. a bad column, named in the message, before a column that was never set
    rc, msg = call(bare, 4, 10, 4, S, 4, [1, 3], 2, L, H, 2)
    assert rc != 0 and b"set column 4" in msg
    rc, msg = call(bare, 4, 10, 0, S, 4, [1, 4], 2, L, H, 2)
    assert rc != 0 and b"column 4" in msg and b"set column" not in msg
    rc, msg = call(bare, 4, 10, 0, S, 4, [3, 1, 3], 3, L, H, 2)
    assert rc != 0 and b"column 3 is named twice" in msg
    rc, msg = call(bare, 4, 10, 1, S, 4, [3, 1], 2, L, H, 2)
    assert rc != 0 and b"column 1 is the set column" in msg
    with pytest.raises(err, match="column 0 is the set column"):
        g.search_batch_by_label_set_box(Q, 10, 64, 0, sets, [1, 0], lo, hi)
    # 6. a column that was never set, with its number: the set column, then a range column
    for mode in MODES:
        with pytest.raises(err, match="no label column 2"):
            bare.search_batch_by_label_set_box(Q, 10, 64, 2, sets, [1, 3], lo, hi, mode)
    bare.set_label_column64(2, 0, np.zeros(10, dtype=np.uint64))
    with pytest.raises(err, match="no label column 1"):
        bare.search_batch_by_label_set_box(Q, 10, 64, 2, sets, [1, 3], lo, hi)
    with pytest.raises(err, match="no label column 2"):
        g.search_batch_by_label_set_box(Q, 10, 64, 0, sets, [1, 2], lo, hi)
    # 7. then the errors every call by label has: the null query / answer pointers
    rc = g.lib.vss_search_batch_by_label_set_box(g.h, None, 4, 10, 64, 0, S, 4, None, 0, None, None, 2, 0, out.ctypes.data, None,
                                                 cnt.ctypes.data, None)
    assert rc != 0 and b"null query" in g.lib.vss_last_error(g.h)
    # the two no-ops: no queries (nothing to read), k == 0
    assert call(g, 0, 10, 0, None, 4, [1, 3], 2, None, None, 2)[0] == 0
    assert call(g, 4, 0, 0, S, 4, [1, 3], 2, L, H, 2)[0] == 0
    assert np.all(out == -1) and np.all(cnt == 0)  # nothing was written by any of them
    base.check(Q, 10, 64, 0, sets, [1, 3], lo, hi, 1500, "after the refusals")


def test_the_five_calls_by_label_are_as_they_were():
    """a fresh index: each of the five existing calls by label answers the same before and after a call by label set box"""
    n, dim, nq, k = 2000, 16, 16, 10
    X, Q = gc.make_data(n, dim, "l2sq", 2420, nq=nq)
    keys = keys_against_slot_order(n, 4000)
    rng = np.random.default_rng(2421)
    grp = rng.integers(0, 8, 4001).astype(np.uint32)
    price = rng.integers(0, 100, 4001).astype(np.uint32)
    ts = rng.integers(0, 1000, 4001).astype(np.uint64) + np.uint64(BASE)
    gpu = build(dim, "l2sq", X, keys, M=8, M0=16, efc=32)
    gpu.set_labels(0, grp)
    gpu.set_label_column(1, 0, price)
    gpu.set_label_column64(2, 0, ts)
    want = rng.integers(0, 9, nq).astype(np.uint32)
    lo32, hi32 = np.stack([want, np.full(nq, 10, np.uint32)], axis=1), np.stack([want + 2, np.full(nq, 80, np.uint32)], axis=1)
    lo64 = np.stack([want.astype(np.uint64), np.full(nq, BASE + 100, np.uint64)], axis=1)
    hi64 = np.stack([want.astype(np.uint64) + np.uint64(2), np.full(nq, TOP64)], axis=1)
    sets32 = np.stack([want, (want + 3) % 8, np.full(nq, NO_LABEL, np.uint32)], axis=1).astype(np.uint32)

    def five(mode):
        return [gpu.search_batch_by_label(Q, k, 64, want, mode, 30), gpu.search_batch_by_label_range(Q, k, 64, want, want + 2, mode, 30),
                gpu.search_batch_by_label_set(Q, k, 64, sets32, mode, 30), gpu.search_batch_by_label_box(Q, k, 64, [0, 1], lo32, hi32, mode, 30),
                gpu.search_batch_by_label_box64(Q, k, 64, [0, 2], lo64, hi64, mode, 30)]

    for mode in MODES:
        before = five(mode)
        got = gpu.search_batch_by_label_set_box(Q, k, 64, 0, sets32.astype(np.uint64), [2], lo64[:, 1:], hi64[:, 1:], mode, 30)
        assert got[2].sum() > 0
        for a, b in zip(before, five(mode)):
            assert_same(a[:3], b[:3], "mode " + mode)
            assert np.array_equal(a[3], b[3]), mode
