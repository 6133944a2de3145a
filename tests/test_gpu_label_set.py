"""-m gpu: vss_search_batch_by_label_set — per-query IN-lists over the index's resident label column (csrc/label_filter.h; the
walkers' admission in csrc/hnsw_kernels.h, the listing kernels in csrc/exact_filtered_kernels.h).

Contract, and the only yardstick here: let s_0 < s_1 < ... be the distinct RAW rows of the call's n_queries x width matrix,
ascending lexicographically as unsigned words (nothing canonicalised: the same members in another order are another group),
bitmap g have bit r set iff r < labelled_rows, labels[r] != NO_LABEL and labels[r] is a word of s_g, and group_of[q] be the index
of query q's row.  Then the call in mode graph / exact / auto returns cell for cell — row ids, f32 distance bits, counts, routes —
what vss_search_batch_filtered_groups / vss_search_exact_batch_filtered_groups / vss_search_batch_filtered_groups_auto return for
that table, and leaves the same counters behind.  No tolerance, no cell left out.  (The bitmap calls' own answers are held to a
CPU brute force in tests/test_gpu_exact_filtered.py, test_gpu_filter_groups.py and test_gpu_filter_route.py.)
"""
import numpy as np
import pytest

import gpu_common as gc
from test_gpu_exact_filtered import _bitmap, _words, assert_same, keys_against_slot_order
from test_gpu_label_search import MODES, NO_LABEL, assert_nothing, bitmap_call, build, counters

pytestmark = pytest.mark.gpu

SET_MAX = 32  # VSS_LABEL_SET_MAX


def padded(rows, width):
    """the matrix of a call: every row's values, then NO_LABEL up to `width`"""
    m = np.full((len(rows), width), NO_LABEL, dtype=np.uint32)
    for q, r in enumerate(rows):
        assert len(r) <= width
        m[q, :len(r)] = r
    return m


def derived_table(labels, sets):
    """the table of the contract: (bitmaps, n_bits, group_of), and the distinct raw rows"""
    labels = np.asarray(labels, dtype=np.uint32)
    rows, group_of = np.unique(sets, axis=0, return_inverse=True)  # rows ascending lexicographically, as unsigned words
    n_bits = len(labels)
    bitmaps = np.zeros((len(rows), _words(n_bits)), dtype=np.uint64)
    for g, row in enumerate(rows):
        bitmaps[g] = _bitmap(n_bits, np.nonzero((labels != NO_LABEL) & np.isin(labels, row))[0])
    return (bitmaps, n_bits, np.asarray(group_of).reshape(-1).astype(np.uint32)), rows


def check(gpu, Q, k, ef, labels, sets, route_c, what, modes=MODES):
    """every mode against the bitmap call of that mode on the derived table: answers, routes, counters.  Returns
    {mode: (the by-set answer, the bitmap call's counters)}"""
    assert gpu.labelled_rows() == len(labels), what
    sets = np.ascontiguousarray(sets, dtype=np.uint32)
    table, _ = derived_table(labels, sets)
    out = {}
    for mode in modes:
        where = "%s, mode %s, route_c %d" % (what, mode, route_c)
        ref = bitmap_call(gpu, mode, Q, k, ef, table, route_c)
        ref_counters = counters(gpu, mode)
        got = gpu.search_batch_by_label_set(Q, k, ef, sets, mode, route_c)
        got_counters = counters(gpu, mode)
        assert_same(got[:3], ref[:3], where)
        assert np.array_equal(got[3], ref[3]), where + ": routes"
        assert got_counters == ref_counters, where + ": counters %r, the bitmap call's %r" % (got_counters, ref_counters)
        out[mode] = (got, ref_counters)
    return out


def live_lengths(labels, keys, sets):
    """rows each query's set admits among the live row ids `keys` (NumPy's restatement of the rule)"""
    keys = keys[keys < len(labels)]
    mine = labels[keys]
    mine = mine[mine != NO_LABEL]
    return np.array([int(np.isin(mine, row).sum()) for row in sets])


def listed_entries(labels, keys, sets):
    """what one exact call lists: every distinct raw row's rows, overlaps counted per group"""
    return int(live_lengths(labels, keys, np.unique(sets, axis=0)).sum())


# ------------------------------------------------------------------------------------------------- 1. the mixed chunk
@pytest.mark.parametrize("metric,dim", [("l2sq", 100), ("cosine", 100), ("ip", 100), ("l2sq", 3), ("l2sq", 768)])
def test_mixed_chunk(metric, dim):
    n, nq, labelled, k, ef, width = 6000, 37, 8000, 10, 64, 8
    X, Q = gc.make_data(n, dim, metric, 2000 + dim, nq=nq)
    keys = keys_against_slot_order(n, 9000)  # row id != slot; row ids 3001 .. 9000, those from 8000 on without a cell
    rng = np.random.default_rng(20)
    labels = rng.integers(0, 10000, labelled).astype(np.uint32)
    big = rng.choice(np.arange(3001, labelled), 2500, replace=False)  # large groups: values 0 .. 3, about 625 live rows each
    labels[big] = rng.integers(0, 4, 2500)
    labels[rng.choice(np.arange(3001, labelled), 20, replace=False)] = NO_LABEL
    v, w = int(labels[5000]), int(labels[6000])
    assert v != NO_LABEL and w != NO_LABEL
    junk = [20001, 20002, 20003, 20004, 20005, 20006, 20007]  # values no row holds
    rows = ([[v]] * 2 + [[w], [0], [3]]                                          # singletons
            + [[0, 1]] * 3 + [[0, 1, 2, 3]] * 3 + [[1, 0]] * 3                     # {1,0}: the members of {0,1}, another group
            + [[2, 2, 2]] * 2 + [[]] * 3 + [[20000, 30000]] * 2                    # a repeat; all padding; values no row holds
            + [junk + [3]] * 2 + [[3] + junk] * 2                                  # the only hit is the LAST word / the first
            + [[1, 2]] * 3 + [[2, 3]] * 3                                          # two that overlap
            + [[NO_LABEL, 0], [0, NO_LABEL, NO_LABEL, 1], [v, w, 0x80000000, 0x7FFFFFFF]]  # padding ahead of a value; the sign bit
            + [[0, 1], [0, 1, 2, 3], [9999, 9998, 9997, 9996, 9995, 9994, 9993, 9992]])
    assert len(rows) == nq
    perm = rng.permutation(nq)
    sets = padded(rows, width)[perm]
    # the first {0,1} and the first {1,0} query ask with the same vector: same members, so the same answer
    q01, q10 = int(np.nonzero(perm == 5)[0][0]), int(np.nonzero(perm == 11)[0][0])
    Q = Q.copy()
    Q[q10] = Q[q01]
    gpu = build(dim, metric, X, keys)
    gpu.set_labels(0, labels)
    what = "%s dim %d" % (metric, dim)
    lens = live_lengths(labels, keys, sets)
    assert 2300 < lens.max() < 2700 and lens[q01] == lens[q10] > 1000
    got = check(gpu, Q, k, ef, labels, sets, 0, what)
    nothing = np.all(sets == NO_LABEL, axis=1) | (sets[:, 0] == 20000)
    assert nothing.sum() == 5 and np.all(lens[nothing] == 0)
    for mode in MODES:
        assert_nothing(got[mode][0], nothing, what + " " + mode)
        assert_same(tuple(a[q10] for a in got[mode][0][:3]), tuple(a[q01] for a in got[mode][0][:3]), what + " {1,0} against {0,1}")
    assert not np.array_equal(sets[q01], sets[q10])
    assert np.array_equal(got["exact"][0][2], np.minimum(lens, k))  # the scan returns min(k, admitted live rows)
    # the rule (csrc/filter_route.h): a group is scanned iff len^2 * 64 <= C * limit * L, limit = max(k, ef), L = live rows
    limit, L = max(k, ef), n
    distinct = np.unique(lens[lens > 0])
    largest, second = int(distinct[-1]), int(distinct[-2])
    # ... a C between the two largest groups: the largest is walked, every other group scanned
    c_between = -(-second * second * 64 // (limit * L))
    assert second * second * 64 <= c_between * limit * L < largest * largest * 64
    route = check(gpu, Q, k, ef, labels, sets, c_between, what, modes=("auto",))["auto"][0][3]
    assert set(route.tolist()) == {0, 1}
    assert np.array_equal(route, np.where(lens == largest, 0, 1))
    # ... and the largest group ON the boundary where an integer C puts it there, else the nearest C on each side
    num, den = largest * largest * 64, limit * L
    for c in ([num // den] if num % den == 0 else [num // den, num // den + 1]):
        route = check(gpu, Q, k, ef, labels, sets, c, what, modes=("auto",))["auto"][0][3]
        assert np.array_equal(route, np.where(lens.astype(object) ** 2 * 64 <= c * den, 1, 0).astype(np.uint8)), c


# ------------------------------------------------------------------------------------------------- 2. width 1
def test_width_one_is_the_call_by_label():
    """sets = want as a column, over the label tests' mixed labels: the answer and the counters of vss_search_batch_by_label"""
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
            got = gpu.search_batch_by_label_set(Q, 10, 64, want[:, None], mode, route_c)
            assert_same(got[:3], ref[:3], where)
            assert np.array_equal(got[3], ref[3]), where + ": routes"
            assert counters(gpu, mode) == ref_counters, where
    check(gpu, Q, 10, 64, labels, want[:, None], 1499, "width 1 against the bitmaps")


# ------------------------------------------------------------------------------------------------- 5. listing edges
@pytest.mark.parametrize("n", [1, 511, 512, 513, 1025])  # FL_WAVE_SLOTS = 512
def test_listing_edges(n):
    """labels laid out BY SLOT (label = slot; a listing wave owns 512 consecutive slots, a row of it 64), so a set's words name
    lanes: lane 0, lane 63, both sides of a row's edge and of the 512-slot block's, slots of three blocks at once, the last slot"""
    dim = 8
    X, Q = gc.make_data(n, dim, "l2sq", 2010 + n, nq=16)
    keys = keys_against_slot_order(n, 2000)
    labels = np.full(2001, NO_LABEL, dtype=np.uint32)
    labels[keys] = np.arange(n, dtype=np.uint32)
    rows = [[0], [63], [63, 64], [511, 512], [0, 511, 512, 1024], [n - 1], [n], [1024, 512, 511, 0]] * 2
    sets = padded(rows, 4)
    gpu = build(dim, "l2sq", X, keys, M=4, M0=8, efc=16)
    gpu.set_labels(0, labels)
    got = check(gpu, Q, 10, 64, labels, sets, 1, "n %d" % n)
    cnt = got["exact"][0][2]
    expect = np.array([len({x for x in r if x < n}) for r in rows])  # label = slot
    assert np.array_equal(cnt, np.minimum(expect, 10))
    assert cnt[5] == 1 and got["exact"][0][0][5][0] == keys[n - 1]  # the set of the last slot only: that row
    distinct = {tuple(r): e for r, e in zip(rows, expect)}
    assert got["exact"][1]["exact"][0] == sum(distinct.values())  # listed: every group's rows, overlaps counted per group


# ------------------------------------------------------------------------------------------------- 4. width edges
def edge_index():
    n, dim = 3000, 16
    X, Q = gc.make_data(n, dim, "l2sq", 2020, nq=12)
    keys = keys_against_slot_order(n, 5000)
    labels = np.random.default_rng(2021).integers(0, 12, 5001).astype(np.uint32)
    gpu = build(dim, "l2sq", X, keys, M=4, M0=8, efc=16)
    gpu.set_labels(0, labels)
    return gpu, Q, keys, labels


@pytest.fixture(scope="module")
def edges():
    return edge_index()


@pytest.mark.parametrize("width", [1, 31, SET_MAX])
def test_width_edges(edges, width):
    """the hit in word 0 only and in the last word only, every other word a value no row holds"""
    gpu, Q, keys, labels = edges
    junk = 1000 + np.arange(width - 1, dtype=np.uint32)
    rows = []
    for q in range(12):
        hit = np.array([q % 6], dtype=np.uint32)
        rows.append(np.concatenate([hit, junk + 100 * q]) if q % 2 == 0 else np.concatenate([junk + 100 * q, hit]))
    sets = np.array(rows, dtype=np.uint32)
    assert sets.shape == (12, width)
    got = check(gpu, Q, 10, 64, labels, sets, 3, "width %d" % width)
    assert np.all(got["exact"][0][2] == 10) and np.all(got["graph"][0][2] > 0)
    lens = live_lengths(labels, keys, sets)
    assert np.array_equal(lens, [int((labels[keys] == q % 6).sum()) for q in range(12)])


@pytest.mark.parametrize("width", [0, SET_MAX + 1])
def test_width_refused(edges, width):
    gpu, Q, _, _ = edges
    Q = np.ascontiguousarray(Q[:4])
    sets = np.zeros((4, max(width, 1)), dtype=np.uint32)
    out = np.full((4, 10), -7, dtype=np.int64)
    dist = np.full((4, 10), 3.0, dtype=np.float32)
    cnt = np.full(4, 77, dtype=np.uint32)
    route = np.full(4, 9, dtype=np.uint8)
    for mode in (0, 1, 2):
        assert gpu.lib.vss_search_batch_by_label_set(gpu.h, Q.ctypes.data, 4, 10, 64, sets.ctypes.data, width, mode, 0, out.ctypes.data,
                                                     dist.ctypes.data, cnt.ctypes.data, route.ctypes.data) != 0
        assert b"width" in gpu.lib.vss_last_error(gpu.h)
    assert np.all(out == -7) and np.all(dist == 3.0) and np.all(cnt == 77) and np.all(route == 9)  # nothing was written
    with pytest.raises(gc.pkg().VssError, match="width"):
        gpu.search_batch_by_label_set(Q, 10, 64, np.zeros((4, width), dtype=np.uint32))


# ------------------------------------------------------------------------------------------------- 6. several passes
def test_overlapping_sets_take_several_passes(monkeypatch):
    """sets overlap, so the lists of one call can together exceed max(budget, rows) entries — which a partition by labels never
    does — and the plan packs them into several passes; as many as the bitmap call's"""
    n, dim, nq = 3000, 16, 24
    X, Q = gc.make_data(n, dim, "l2sq", 2030, nq=nq)
    keys = keys_against_slot_order(n, 5000)
    rng = np.random.default_rng(2031)
    labels = rng.integers(0, 12, 5001).astype(np.uint32)
    rows = [[0, 1, 2, 3, 4, 5, 6, 7], [4, 5, 6, 7, 8, 9, 10, 11], [0, 2, 4, 6, 8, 10], [1, 2, 3, 4, 5, 6], [11, 0, 5], [3, 9]] * 4
    sets = padded(rows, 8)
    monkeypatch.setenv("VSS_EXACT_FILTER_LIST_ENTRIES", "1000")
    gpu = build(dim, "l2sq", X, keys, M=4, M0=8, efc=16)
    gpu.set_labels(0, labels)
    got = check(gpu, Q, 10, 64, labels, sets, 0, "budget 1000", modes=("exact", "auto"))
    listed, _, passes = got["exact"][1]["exact"]
    assert listed == listed_entries(labels, keys, sets) > n and passes >= 2


# ------------------------------------------------------------------------------------------------- 7. kernel shapes
class Base:
    def __init__(self):
        self.metric, self.n, self.dim = "l2sq", 6000, 32
        self.X, self.Q = gc.make_data(self.n, self.dim, self.metric, 2040, nq=300)
        self.keys = keys_against_slot_order(self.n, 9000)
        rng = np.random.default_rng(2041)
        by_slot = rng.integers(8, 10000, self.n).astype(np.uint32)
        big = rng.choice(self.n, 4800, replace=False)  # values 0 .. 7: 600 rows each
        by_slot[big] = np.arange(4800) % 8
        by_slot[rng.choice(self.n, 3, replace=False)] = NO_LABEL
        self.labels = np.full(9001, NO_LABEL, dtype=np.uint32)
        self.labels[self.keys] = by_slot
        self.sorted = np.sort(by_slot[by_slot != NO_LABEL])
        self.gpu = build(self.dim, self.metric, self.X, self.keys)
        self.gpu.set_labels(0, self.labels)

    def check(self, Q, k, ef, sets, route_c, what, modes=MODES):
        return check(self.gpu, Q, k, ef, self.labels, sets, route_c, what, modes)


@pytest.fixture(scope="module")
def base():
    return Base()


# about 4800, 3600, 1200 and 600 rows, a handful, none, none
SEVEN = padded([[0, 1, 2, 3, 4, 5, 6, 7], [5, 4, 3, 2, 1, 0], [6, 7], [7], [100, 101, 102, 103, 104, 105, 106, 107], [], [20000]], 8)


@pytest.mark.parametrize("ef", [64, 300, 600])  # lists in registers (2 and 8 per lane) and outside them
def test_list_widths(base, ef):
    sets = SEVEN[np.arange(21) % 7]
    route_c = {64: 1000, 300: 300, 600: 160}[ef]  # len^2 * 64 <= route_c * limit * 6000 ends near 3000 rows at each limit
    got = base.check(base.Q[:21], 100, ef, sets, route_c, "ef %d" % ef)
    assert (got["graph"][1]["shape"][4] != 0) == (ef == 600)  # beyond 512 the list has left the registers (the bitmap call's shape)
    route = got["auto"][0][3]
    wide = np.isin(np.arange(21) % 7, [0, 1])  # 4800 and 3600 rows are walked, 1200 and fewer scanned
    assert np.all(route[wide] == 0) and np.all(route[~wide] == 1)


def test_one_query_takes_the_solo_kernel():
    n, dim = 2000, 128
    X, Q = gc.make_data(n, dim, "l2sq", 2050, nq=4)
    keys = keys_against_slot_order(n, 3000)
    labels = (np.arange(3001) % 30).astype(np.uint32)
    gpu = build(dim, "l2sq", X, keys, M=8, M0=16, efc=32)
    gpu.set_labels(0, labels)
    for q, row in enumerate([np.arange(10), np.arange(20, 30)[::-1]]):
        for width in (10, SET_MAX):
            got = check(gpu, Q[q:q + 1], 10, 64, labels, padded([row], width), 1, "one query, width %d" % width)
            assert got["graph"][1]["shape"][6] == 1 and got["graph"][0][2][0] == 10


@pytest.mark.parametrize("nq", [204, 300])  # the join's chunk; more than a launch of one query per compute unit
def test_host_batches(base, nq):
    rng = np.random.default_rng(2060 + nq)
    sets = rng.integers(8, 10000, (nq, 8)).astype(np.uint32)  # nearly every query its own set, of a handful of rows ...
    wide = np.nonzero(rng.integers(0, 4, nq) == 0)[0]          # ... or of 3600 and more
    for q in wide:
        sets[q, :6] = rng.permutation(6)
    sets[::50] = NO_LABEL
    sets[1::50, 3:] = NO_LABEL
    got = base.check(base.Q[:nq], 10, 64, sets, 1500, "%d queries" % nq)
    assert set(got["auto"][0][3]) == {0, 1}
    assert len(np.unique(sets, axis=0)) > nq * 9 // 10


def test_rare_predicate_reruns(base):
    """sets of six rows and of one: the walk rejects nearly every row it meets, its pending candidates outgrow the register
    queue, and the queries are re-run through the unbounded one — reading the same table of sets again, through a.work[idx]"""
    s = base.sorted
    six, one = np.unique(s[5000:5006]), s[5500:5501]
    assert six[0] >= 8 and one[0] >= 8
    n_six, n_one = int(np.isin(s, six).sum()), int((s == one[0]).sum())
    assert 6 <= n_six <= 9 and 1 <= n_one <= 3
    sets = padded([six, one] * 8, 8)
    got = base.check(base.Q[:16], 10, 64, sets, 1500, "rare sets", modes=("graph",))
    _, _, cnt, _ = got["graph"][0]
    assert np.all(cnt[0::2] <= n_six) and np.all(cnt[1::2] <= n_one) and cnt.sum() > 0  # (a walk may miss a row; it invents none)
    assert got["graph"][1]["stats"][3] > 0  # (the bitmap call's counter, and by check() this call's: queries were re-run)


@pytest.mark.parametrize("w", [2, 8, SET_MAX])
def test_consecutive_values_are_the_range(base, w):
    """{a, a + 1, ..., a + w - 1} admits what the range [a, a + w - 1] admits: its answers and routes"""
    nq = 24
    rng = np.random.default_rng(2070 + w)
    a = rng.integers(8, 9900, nq).astype(np.uint32)
    a[:4] = [0, 0, 3, 7]  # the large groups: w values from 0 on hold 600 rows each up to 7
    sets = (a[:, None] + np.arange(w, dtype=np.uint32)[None, :]).astype(np.uint32)
    for mode in MODES:
        where = "w %d, mode %s" % (w, mode)
        ref = base.gpu.search_batch_by_label_range(base.Q[:nq], 10, 64, a, a + np.uint32(w - 1), mode, 300)
        got = base.gpu.search_batch_by_label_set(base.Q[:nq], 10, 64, sets, mode, 300)
        assert_same(got[:3], ref[:3], where)
        assert np.array_equal(got[3], ref[3]), where + ": routes"


def test_device_form(base):
    import torch
    nq, k = 35, 10
    Q = base.Q[:nq]
    sets = SEVEN[np.arange(nq) % 7].copy()
    sets[3] = NO_LABEL
    d_Q = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    d_sets = torch.from_numpy(sets.view(np.int32)).cuda()
    for mode in MODES:
        ref = base.check(Q, k, 64, sets, 1500, "host form", modes=(mode,))[mode][0]
        for bare in (False, True):
            d_keys = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
            d_dist = None if bare else torch.zeros((nq, k), dtype=torch.float32, device="cuda")
            d_cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
            d_route = None if bare else torch.full((nq,), 9, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            base.gpu.search_batch_by_label_set_device(d_Q.data_ptr(), nq, k, 64, d_sets.data_ptr(), sets.shape[1], d_keys.data_ptr(),
                                                      None if bare else d_dist.data_ptr(), d_cnt.data_ptr(),
                                                      None if bare else d_route.data_ptr(), mode, 1500)
            assert np.array_equal(d_keys.cpu().numpy(), ref[0]), mode
            assert np.array_equal(d_cnt.cpu().numpy().astype(np.uint32), ref[2]), mode
            if not bare:
                assert np.array_equal(d_dist.cpu().numpy().view(np.uint32), ref[1].view(np.uint32)), mode
                assert np.array_equal(d_route.cpu().numpy(), ref[3]), mode


# ------------------------------------------------------------------------------------------------- 8. lifecycle
def test_lifecycle():
    n, dim, nq = 3000, 16, 24
    rng = np.random.default_rng(2080)
    X, Q = gc.make_data(n + 400, dim, "l2sq", 2081, nq=nq)
    keys = keys_against_slot_order(n, 5000)            # ids 2001 .. 5000
    new_keys = np.arange(400, dtype=np.int64) + 100    # the rows added later: ids 100 .. 499, labelled from the start
    labels = rng.integers(0, 20, 5001).astype(np.uint32)
    labels[rng.choice(5001, 50, replace=False)] = NO_LABEL
    sets = padded([[0, 1, 2, 3, 4, 5, 6, 7, 8, 9], [5], [4, 5, 6], [19, 18], [5500, 5000], [7, 7]] * 4, 12)
    late = sets[:, 0] == 5500
    gpu = build(dim, "l2sq", X[:n], keys, capacity=n + 400, M=8, M0=16, efc=32)
    gpu.set_labels(0, labels)
    got = check(gpu, Q, 10, 64, labels, sets, 100, "built")
    assert np.all(got["exact"][0][2][late] == 0)  # no row carries a label from 5000 on (yet)
    # rows removed, rows added into their slots, compaction: the column is by row id and needs no call
    gone = rng.choice(n, 700, replace=False)
    assert gpu.remove(keys[gone]) == 700
    check(gpu, Q, 10, 64, labels, sets, 100, "700 removed")
    gpu.add(new_keys, X[n:])
    got = check(gpu, Q, 10, 64, labels, sets, 100, "400 added into reused slots")
    assert np.any(np.isin(got["exact"][0][0], new_keys))
    gpu.compact()
    check(gpu, Q, 10, 64, labels, sets, 100, "compacted")
    # cells overwritten: the answers follow the column by row id
    labels[2500:3500] = 5500
    gpu.set_labels(2500, labels[2500:3500])
    got = check(gpu, Q, 10, 64, labels, sets, 100, "overwritten")
    assert np.all(got["exact"][0][2][late] == 10)
    assert np.all((got["exact"][0][0][late] >= 2500) & (got["exact"][0][0][late] < 3500))
    gpu.clear_labels()
    with pytest.raises(gc.pkg().VssError, match="no label column"):
        gpu.search_batch_by_label_set(Q, 10, 64, sets)
    gpu.set_labels(0, labels)
    check(gpu, Q, 10, 64, labels, sets, 100, "cleared and labelled again", modes=("auto",))


# ------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals(base):
    g, Q = base.gpu, np.ascontiguousarray(base.Q[:4])
    sets = padded([[0, 1], [2], [], [100, 7]], 4)
    err = gc.pkg().VssError
    for mode in (3, -1, 255):
        with pytest.raises(err, match="mode"):
            g.search_batch_by_label_set(Q, 10, 64, sets, mode)
    bare = gc.gpu_index(base.dim, base.metric)
    for mode in MODES:
        with pytest.raises(err, match="no label column"):
            bare.search_batch_by_label_set(Q, 10, 64, sets, mode)
    # the order: the mode first, then the width, then null sets, then the missing column
    with pytest.raises(err, match="mode"):
        bare.search_batch_by_label_set(Q, 10, 64, np.zeros((4, 40), dtype=np.uint32), 3)
    with pytest.raises(err, match="width"):
        bare.search_batch_by_label_set(Q, 10, 64, np.zeros((4, 40), dtype=np.uint32))
    out = np.full((4, 10), -1, dtype=np.int64)
    cnt = np.zeros(4, dtype=np.uint32)
    for index, width in ((g, 4), (bare, 4), (bare, 0)):
        for mode in (0, 1, 2):
            assert index.lib.vss_search_batch_by_label_set(index.h, Q.ctypes.data, 4, 10, 64, None, width, mode, 0, out.ctypes.data, None,
                                                           cnt.ctypes.data, None) != 0
            assert (b"width" if width == 0 else b"null sets") in index.lib.vss_last_error(index.h)
    # without queries, or without results to return, the call has nothing to read: VSS_OK, nothing written
    assert g.lib.vss_search_batch_by_label_set(g.h, Q.ctypes.data, 0, 10, 64, None, 4, 2, 0, out.ctypes.data, None, cnt.ctypes.data,
                                               None) == 0
    assert g.lib.vss_search_batch_by_label_set(g.h, Q.ctypes.data, 4, 0, 64, sets.ctypes.data, 4, 2, 0, out.ctypes.data, None,
                                               cnt.ctypes.data, None) == 0
    assert np.all(out == -1) and np.all(cnt == 0)  # nothing was written by any of them
    # the wrapper: a wrong shape is a ValueError; per-query sequences are padded to the longest
    with pytest.raises(ValueError):
        g.search_batch_by_label_set(Q, 10, 64, sets[:3])
    with pytest.raises(ValueError):
        g.search_batch_by_label_set(Q, 10, 64, sets.reshape(-1))
    as_lists = g.search_batch_by_label_set(Q, 10, 64, [[0, 1], [2], [], (100, 7)], "exact")
    assert_same(as_lists[:3], g.search_batch_by_label_set(Q, 10, 64, sets[:, :2], "exact")[:3], "lists against the matrix")
    base.check(Q, 10, 64, sets, 1500, "after the refusals")
