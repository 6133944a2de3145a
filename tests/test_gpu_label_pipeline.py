"""-m gpu: label predicates in the pipelined and multi-batch launches — vss_search_by_label_device_begin and
vss_search_multi_by_label_device_begin, completed by vss_search_batch_end (csrc/label_filter.h "several batches"; the resolve
kernels k_resolve_label_batches / k_resolve_label_batches64 in csrc/hnsw_kernels.h).

The only yardstick, throughout: the EXISTING blocking _device call of the same form in mode graph on the same index, for the same
queries and the same per-query words.  "Equal" is row ids, f32 distance bits and counts, cell for cell; no tolerance.

The index: 3000 x 32, l2sq, row ids odd and descending with the slot (6001, 5999, ... 3: non-contiguous, row id != slot), every
13th row removed.  Four label columns by row id, 6002 cells each but column 2, which is the shorter one (5602 cells: row ids from
5602 on have no cell there):
  0  tenant, 32 bits: five common values 0 .. 4, and sixteen rare ones 100 .. 115 on three rows each
  1  group, 32 bits: 0 .. 39
  2  64 BITS: values on both sides of 2^32
  3  timestamp, 64 BITS: BASE + [0, 10000)
Five NULL cells among the rows of each; the cells of the even row ids, which no row has, are NULL too.
EQ, RANGE and SET read column 0; BOX columns 0, 1; BOX64 columns 1, 3, 2; SET_BOX a set on column 0 inside ranges on columns 3, 2.
"""
import numpy as np
import pytest

import gpu_common as gc

pytestmark = pytest.mark.gpu

NO_LABEL = 0xFFFFFFFF
TOP64 = 0xFFFFFFFFFFFFFFFF
T32 = 1 << 32
BASE = (1 << 63) + 10 ** 15
KINDS = ("eq", "range", "set", "box", "box64", "set_box")
SET_WIDTH = {"set": 6, "set_box": 5}  # padded to 8 words of 32 bits, to 6 words of 64
COLUMNS = {"box": [0, 1], "box64": [1, 3, 2], "set_box": [3, 2]}
SET_COLUMN = 0
RARE = 16  # rare tenants 100 .. 115


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
        return self.keys.data_ptr(), self.dist.data_ptr() if self.dist is not None else None, self.cnt.data_ptr()

    def fetch(self):
        import torch
        torch.cuda.synchronize()
        return (self.keys.cpu().numpy(), self.dist.cpu().numpy() if self.dist is not None else None,
                self.cnt.cpu().numpy().view(np.uint32))

    def untouched(self):
        k, d, c = self.fetch()
        return np.all(k == -7) and np.all(c == 99) and (d is None or np.all(d == 0))


def same(got, want, what):
    gk, gd, gcnt = got
    wk, wd, wcnt = want
    bad = [q for q in range(len(wk)) if not (np.array_equal(gk[q], wk[q]) and gcnt[q] == wcnt[q]
                                             and (gd is None or np.array_equal(gd[q].view(np.uint32), wd[q].view(np.uint32))))]
    assert not bad, "%s: %d of %d queries differ; first: query %d, %r / %r" % (what, len(bad), len(wk), bad[0],
                                                                              gk[bad[0]].tolist(), wk[bad[0]].tolist())


class Index:
    def __init__(self, n, dim, M, M0, efc, seed, dead_step, nq):
        self.n, self.dim = n, dim
        self.X, self.Q = gc.make_data(n, dim, "l2sq", seed, nq=nq)
        self.keys = (2 * n + 1 - 2 * np.arange(n)).astype(np.int64)
        cells = 2 * n + 2
        rng = np.random.default_rng(seed + 7)
        tenant = rng.integers(0, 5, n).astype(np.uint32)
        self.rare_slots = rng.choice(n, 3 * RARE, replace=False)
        tenant[self.rare_slots] = 100 + np.arange(3 * RARE, dtype=np.uint32) // 3
        by_slot = {0: tenant, 1: rng.integers(0, 40, n).astype(np.uint32),
                   2: rng.integers(0, 100, n).astype(np.uint64) + np.uint64(T32 - 50),
                   3: rng.integers(0, 10000, n).astype(np.uint64) + np.uint64(BASE)}
        self.cols = {}
        for c, values in by_slot.items():
            none = NO_LABEL if values.dtype == np.uint32 else TOP64
            values[rng.choice(np.setdiff1d(np.arange(n), self.rare_slots), 5, replace=False)] = none
            column = np.full(cells, none, dtype=values.dtype)
            column[self.keys] = values
            self.cols[c] = column[:cells - 400] if c == 2 else column
        self.by_slot = by_slot
        self.gpu = gc.gpu_index(dim, "l2sq", M, M0, efc)
        self.gpu.reserve(n)
        self.gpu.set_build_params(32768, 4)
        self.gpu.add(self.keys, self.X)
        self.removed = self.keys[::dead_step]
        assert self.gpu.remove(self.removed) == len(self.removed)
        for c, column in self.cols.items():
            if column.dtype == np.uint64:
                self.gpu.set_label_column64(c, 0, column)
            else:
                self.gpu.set_label_column(c, 0, column)
        assert [self.gpu.label_column_width(c) for c in range(4)] == [32, 32, 64, 64]
        assert self.gpu.label_column_rows(2) < self.gpu.label_column_rows(3) == cells
        self.ts_sorted = np.sort(by_slot[3][by_slot[3] != np.uint64(TOP64)])

    # ---- one query's words.  style: "mixed" a predicate of some hundred rows, "all" the widest the form can say, "none" an
    # empty one (lo > hi, or a list that is all padding), "rare" one of a handful of rows
    def words(self, kind, style, rng):
        t, v = int(rng.integers(0, 5)), 100 + int(rng.integers(0, RARE))
        at = int(rng.integers(0, len(self.ts_sorted) - 8))
        window = (int(self.ts_sorted[at]), int(self.ts_sorted[at + 5]))
        since = BASE + int(rng.integers(0, 8000))
        if kind == "eq":  # (an equality cannot admit every row: "all" is one common tenant)
            return {"want": {"mixed": t, "all": 0, "none": NO_LABEL, "rare": v}[style]}
        if kind == "range":
            lo, hi = {"mixed": (t, min(t + int(rng.integers(0, 3)), 4)), "all": (0, NO_LABEL), "none": (3, 2), "rare": (v, v)}[style]
            return {"lo": lo, "hi": hi}
        if kind in ("set", "set_box"):
            width, pad = SET_WIDTH[kind], NO_LABEL if kind == "set" else TOP64
            members = {"mixed": list(rng.choice(5, 1 + int(rng.integers(0, 3)), replace=False)), "all": [0, 1, 2, 3, 4], "none": [],
                       "rare": [v] if kind == "set" else [0, 1, 2, 3, 4]}[style]
            row = np.full(width, pad, dtype=np.uint64)
            row[rng.choice(width, len(members), replace=False)] = members  # members among padding, in any position
            if kind == "set":
                return {"sets": row}
            lo, hi = {"mixed": ([since, 0], [TOP64, TOP64]), "all": ([0, 0], [TOP64, TOP64]), "none": ([0, 0], [TOP64, TOP64]),
                      "rare": ([window[0], 0], [window[1], TOP64])}[style]
            return {"sets": row, "lo": lo, "hi": hi}
        if kind == "box":
            a = int(rng.integers(0, 28))
            lo, hi = {"mixed": ([t, a], [t, a + 12]), "all": ([0, 0], [NO_LABEL, NO_LABEL]), "none": ([0, 9], [NO_LABEL, 3]),
                      "rare": ([v, 0], [v, NO_LABEL])}[style]
            return {"lo": lo, "hi": hi}
        a = int(rng.integers(0, 25))  # box64 over columns 1, 3, 2
        lo, hi = {"mixed": ([a, since, 0], [a + 15, TOP64, TOP64]), "all": ([0, 0, 0], [TOP64, TOP64, TOP64]),
                  "none": ([0, BASE + 9, 0], [TOP64, BASE + 2, TOP64]), "rare": ([0, window[0], 0], [TOP64, window[1], T32 + 60])}[style]
        return {"lo": lo, "hi": hi}


class Chunk:
    """One batch: its queries and its per-query words of one kind, on the host and on the device, what the blocking _device call of
    the kind in mode graph answers it with, and the counters that call leaves."""

    def __init__(self, ix, kind, Q, styles, seed, k, ef, yardstick=True):
        self.ix, self.kind, self.k, self.ef = ix, kind, k, ef
        self.Q = np.ascontiguousarray(Q, dtype=np.float32)
        self.nq = len(self.Q)
        rng = np.random.default_rng(seed)
        rows = [ix.words(kind, styles[q % len(styles)], rng) for q in range(self.nq)]
        dtype = np.uint64 if kind in ("box64", "set_box") else np.uint32
        self.words = {name: np.ascontiguousarray(np.array([r[name] for r in rows], dtype=np.uint64).astype(dtype)) for name in rows[0]}
        self.d_Q = _dev(self.Q)
        self.d = {name: _dev(a) for name, a in self.words.items()}
        if yardstick:
            self.want, self.stats = self.blocking()

    def blocking(self, dist=True):
        gpu, d, nq, k, ef = self.ix.gpu, self.d, self.nq, self.k, self.ef
        cells = Cells(nq, k, dist)
        out = cells.ptrs() + (None, "graph")
        q = self.d_Q.data_ptr()
        if self.kind == "eq":
            gpu.search_batch_by_label_device(q, nq, k, ef, d["want"].data_ptr(), *out)
        elif self.kind == "range":
            gpu.search_batch_by_label_range_device(q, nq, k, ef, d["lo"].data_ptr(), d["hi"].data_ptr(), *out)
        elif self.kind == "set":
            gpu.search_batch_by_label_set_device(q, nq, k, ef, d["sets"].data_ptr(), SET_WIDTH["set"], *out)
        elif self.kind == "box":
            gpu.search_batch_by_label_box_device(q, nq, k, ef, COLUMNS["box"], d["lo"].data_ptr(), d["hi"].data_ptr(), *out)
        elif self.kind == "box64":
            gpu.search_batch_by_label_box64_device(q, nq, k, ef, COLUMNS["box64"], d["lo"].data_ptr(), d["hi"].data_ptr(), *out)
        else:
            gpu.search_batch_by_label_set_box_device(q, nq, k, ef, SET_COLUMN, d["sets"].data_ptr(), SET_WIDTH["set_box"], COLUMNS["set_box"],
                                                     d["lo"].data_ptr(), d["hi"].data_ptr(), *out)
        self.shape = gpu.last_search_shape().copy()  # of this call's launch
        return cells.fetch(), gpu.last_search_stats().copy()

    def predicate(self, **changes):
        P, d = gc.pkg().LabelPredicate, dict(self.d, **changes)
        if self.kind == "eq":
            return P.eq(d["want"])
        if self.kind == "range":
            return P.range(d["lo"], d["hi"])
        if self.kind == "set":
            return P.set(d["sets"], d.get("width", SET_WIDTH["set"]))
        if self.kind == "box":
            return P.box(d.get("columns", COLUMNS["box"]), d["lo"], d["hi"])
        if self.kind == "box64":
            return P.box64(d.get("columns", COLUMNS["box64"]), d["lo"], d["hi"])
        return P.set_box(SET_COLUMN, d["sets"], d.get("width", SET_WIDTH["set_box"]), d.get("columns", COLUMNS["set_box"]), d["lo"], d["hi"])


def multi_begin(gpu, context, chunks, cells, predicates=None):
    c0 = chunks[0]
    gpu.search_multi_by_label_begin(context, [c.d_Q.data_ptr() for c in chunks], c0.nq, c0.k, c0.ef,
                                    predicates or [c.predicate() for c in chunks], [c.ptrs()[0] for c in cells],
                                    [c.ptrs()[1] for c in cells], [c.ptrs()[2] for c in cells])


_cache = {}


def base():
    if "base" not in _cache:
        _cache["base"] = Index(3000, 32, 16, 32, 64, 2400, 13, nq=65)
    return _cache["base"]


def test_the_fixture_is_what_the_docstring_says():
    ix = base()
    assert len(np.unique(ix.keys)) == ix.n and np.all(ix.keys % 2 == 1) and np.all(np.diff(ix.keys) == -2)
    assert len(ix.removed) == -(-ix.n // 13)
    for c in range(4):
        none = NO_LABEL if ix.cols[c].dtype == np.uint32 else TOP64
        assert (ix.by_slot[c] == none).sum() == 5
    assert all((ix.by_slot[0] == 100 + j).sum() == 3 for j in range(RARE))
    assert (ix.keys >= len(ix.cols[2])).sum() == 200  # rows without a cell in the shorter column


# ------------------------------------------------------------------------------------------------- 1. one batch, every kind
@pytest.mark.parametrize("kind", KINDS)
def test_1_one_batch(kind):
    ix = base()
    chunk = Chunk(ix, kind, ix.Q[:48], ["mixed", "mixed", "all", "none", "rare", "mixed"], 2410, 10, 64)
    cells = Cells(48, 10)
    ix.gpu.search_by_label_begin(1, chunk.d_Q.data_ptr(), 48, 10, 64, chunk.predicate(), *cells.ptrs())
    ix.gpu.search_end(1)
    stats, shape = ix.gpu.last_search_stats().copy(), ix.gpu.last_search_shape().copy()
    got = cells.fetch()
    same(got, chunk.want, kind)
    print(kind, "counters of the launch:", stats.tolist(), "of the blocking call:", chunk.stats.tolist())
    print(kind, "shape of the launch:", shape.tolist(), "of the blocking call:", chunk.shape.tolist())
    assert stats.tolist() == chunk.stats.tolist()
    assert shape.tolist() == chunk.shape.tolist()
    none = np.arange(48) % 6 == 3
    assert np.all(got[2][none] == 0) and np.all(got[0][none] == -1) and np.all(np.isposinf(got[1][none]))
    assert np.all(got[2][np.arange(48) % 6 == 2] == 10)  # (no comparison of empty answers)


def test_1_set_box_without_range_columns():
    """n_columns == 0 — the set call over 64-bit words: d_lo and d_hi are NULL and nothing reads them.  One batch, and two batches
    in one launch."""
    ix = base()
    gpu, k, ef, nq = ix.gpu, 10, 64, 48
    rng = np.random.default_rng(2415)
    sets = np.full((nq, 5), TOP64, dtype=np.uint64)
    for q in range(nq):  # one to three tenants among padding; every sixth list all padding; a rare tenant; a word beyond 32 bits
        members = [] if q % 6 == 3 else [100 + q % RARE, T32 + 1] if q % 6 == 4 else list(rng.choice(5, 1 + q % 3, replace=False))
        sets[q, rng.choice(5, len(members), replace=False)] = members
    d_Q, d_sets = _dev(np.ascontiguousarray(ix.Q[:nq])), _dev(sets)
    want = Cells(nq, k)
    gpu.search_batch_by_label_set_box_device(d_Q.data_ptr(), nq, k, ef, SET_COLUMN, d_sets.data_ptr(), 5, [], None, None, *want.ptrs(),
                                             None, "graph")
    want_stats = gpu.last_search_stats().tolist()
    want = want.fetch()
    assert np.all(want[2][np.arange(nq) % 6 == 3] == 0) and want[2].sum() > 0
    P = gc.pkg().LabelPredicate
    one = Cells(nq, k)
    gpu.search_by_label_begin(1, d_Q.data_ptr(), nq, k, ef, P.set_box(SET_COLUMN, d_sets, 5), *one.ptrs())
    gpu.search_end(1)
    assert gpu.last_search_stats().tolist() == want_stats
    same(one.fetch(), want, "no range columns, one batch")
    halves = [Cells(24, k), Cells(24, k)]
    gpu.search_multi_by_label_begin(2, [d_Q[:24].data_ptr(), d_Q[24:].data_ptr()], 24, k, ef,
                                    [P.set_box(SET_COLUMN, d_sets[:24], 5), P.set_box(SET_COLUMN, d_sets[24:], 5)],
                                    [c.ptrs()[0] for c in halves], [c.ptrs()[1] for c in halves], [c.ptrs()[2] for c in halves])
    gpu.search_end(2)
    for b in range(2):
        same(halves[b].fetch(), tuple(a[24 * b:24 * b + 24] for a in want), ("no range columns, two batches", b))


# ------------------------------------------------------------------------------------------------- 2. five batches, one launch
def five(kind):
    """5 x 13 queries, k 10 / ef 64: 0 mixed predicates, 1 the widest, 2 mixed ones from another seed, 3 empty ones, 4 rare and mixed
    ones interleaved — neighbouring batches differ"""
    if ("five", kind) not in _cache:
        ix = base()
        styles = [["mixed"], ["all"], ["mixed", "mixed", "none"], ["none"], ["rare", "mixed"]]
        _cache["five", kind] = [Chunk(ix, kind, ix.Q[13 * b:13 * b + 13], styles[b], 2420 + b, 10, 64) for b in range(5)]
    return _cache["five", kind]


@pytest.mark.parametrize("solo,shape6", [(1, None), (0, 0), (2, 1)])
@pytest.mark.parametrize("kind", KINDS)
def test_2_five_batches_one_launch(kind, solo, shape6):
    """every batch equals its own blocking call, the launch's work counters are the sums of the five calls', and both kernel
    families (search.solo 0 and 2) carry such a launch.  Batch 2 has no distance buffer."""
    ix, chunks = base(), five(kind)
    ix.gpu.set_option("search.solo", solo)
    try:
        cells = [Cells(13, 10, dist=b != 2) for b in range(5)]
        multi_begin(ix.gpu, 1, chunks, cells)
        ix.gpu.search_end(1)
        st, shape = ix.gpu.last_search_stats().copy(), ix.gpu.last_search_shape().copy()
    finally:
        ix.gpu.set_option("search.solo", 1)
    for b in range(5):
        got = cells[b].fetch()
        assert (got[1] is None) == (b == 2)
        same(got, chunks[b].want, (kind, "solo", solo, "batch", b))
    assert np.all(cells[3].fetch()[2] == 0) and np.all(cells[1].fetch()[2] > 0)  # (a walk may miss a row; no empty comparison)
    print(kind, "work counters of the launch:", st.tolist(), "of the five calls:", [c.stats.tolist() for c in chunks])
    assert int(st[0]) == sum(int(c.stats[0]) for c in chunks) and int(st[1]) == sum(int(c.stats[1]) for c in chunks)
    assert int(st[2]) == 65
    if shape6 is not None:
        assert shape[6] == shape6, shape


# ------------------------------------------------------------------------------------------------- 3. edges of the batch count
def test_3_edges_of_the_batch_count():
    ix = base()
    gpu, k, ef, err = ix.gpu, 10, 64, gc.pkg().VssError
    # 32 batches x 2 queries
    chunks = [Chunk(ix, "box64", ix.Q[2 * b:2 * b + 2], ["mixed", "rare", "none"], 2440 + b, k, ef) for b in range(32)]
    cells = [Cells(2, k) for _ in range(32)]
    multi_begin(gpu, 2, chunks, cells)
    gpu.search_end(2)
    assert int(gpu.last_search_stats()[2]) == 64
    for b in range(32):
        same(cells[b].fetch(), chunks[b].want, ("32 batches", b))
    # 1 batch through the multi call = the one-batch call
    for kind in ("set_box", "range"):
        one = Chunk(ix, kind, ix.Q[:24], ["mixed", "all", "rare"], 2480, k, ef)
        multi, single = Cells(24, k), Cells(24, k)
        multi_begin(gpu, 0, [one], [multi])
        gpu.search_end(0)
        gpu.search_by_label_begin(0, one.d_Q.data_ptr(), 24, k, ef, one.predicate(), *single.ptrs())
        gpu.search_end(0)
        same(multi.fetch(), single.fetch(), "one batch against the one-batch _begin call")
        same(multi.fetch(), one.want, "one batch")
    # refusals: nothing is enqueued, nothing written, nothing pending
    fresh = [Cells(2, k) for _ in range(33)]
    with pytest.raises(err, match="1 to 32 batches per launch"):
        multi_begin(gpu, 2, chunks + [chunks[0]], fresh)
    three, out = chunks[:3], fresh[:3]
    sb = [Chunk(ix, "set_box", ix.Q[2 * b:2 * b + 2], ["mixed"], 2490 + b, k, ef, yardstick=False) for b in range(3)]

    def refused(match, batches, predicates):
        with pytest.raises(err, match=match):
            multi_begin(gpu, 2, batches, out, predicates)
        gpu.search_end(2)  # (nothing pending)
        assert all(c.untouched() for c in out), match

    refused("batch 2 is of kind 5, batch 0 of kind 4", three, [three[0].predicate(), three[1].predicate(), sb[2].predicate()])
    refused("batch 1 names other label columns", three, [three[0].predicate(), three[1].predicate(columns=[1, 2, 3]), three[2].predicate()])
    refused("batch 1 names other label columns", three, [three[0].predicate(), three[1].predicate(columns=[1, 3]), three[2].predicate()])
    refused("batch 1 has set width 4, batch 0 has 5", sb, [sb[0].predicate(), sb[1].predicate(width=4), sb[2].predicate()])
    refused("batch 1: null lo / hi pointer", three, [three[0].predicate(), three[1].predicate(lo=None), three[2].predicate()])
    refused("batch 2: null sets pointer", sb, [sb[0].predicate(), sb[1].predicate(), sb[2].predicate(sets=None)])
    refused("batch 0: column 7 is not below", three, [c.predicate(columns=[1, 7, 2]) for c in three])
    refused("batch 0: column 3 is named twice", three, [c.predicate(columns=[1, 3, 3]) for c in three])
    refused("kind 6 is none of", three, [gc.pkg().LabelPredicate(6, lo=c.d["lo"], hi=c.d["hi"]) for c in three])
    with pytest.raises(err, match="vss_search_by_label_device_begin: set_width 33 is not within"):
        gpu.search_by_label_begin(2, sb[0].d_Q.data_ptr(), 2, k, ef, sb[0].predicate(width=33), *out[0].ptrs())
    with pytest.raises(err, match="out of range"):
        multi_begin(gpu, 4, three, out)
    with pytest.raises(err, match="null table"):
        gpu.search_multi_by_label_begin(2, [c.d_Q.data_ptr() for c in three], 2, k, ef, None, [c.ptrs()[0] for c in out],
                                        [c.ptrs()[1] for c in out], [c.ptrs()[2] for c in out])
    # a context in flight refuses a second launch, and keeps the first
    flying = Cells(2, k)
    gpu.search_by_label_begin(2, three[0].d_Q.data_ptr(), 2, k, ef, three[0].predicate(), *flying.ptrs())
    with pytest.raises(err, match="already has a batch in flight"):
        multi_begin(gpu, 2, three, out)
    gpu.search_end(2)
    same(flying.fetch(), three[0].want, "the launch that was in flight")
    gpu.search_end(2)  # (nothing pending)
    assert all(c.untouched() for c in fresh)
    # a launch of no queries: nothing to refuse, nothing pending
    gpu.search_multi_by_label_begin(2, [0, 0], 0, k, ef, [three[0].predicate(), three[1].predicate()], [0, 0], [0, 0], [0, 0])
    gpu.search_by_label_begin(2, None, 0, k, ef, three[0].predicate(), None, None, None)
    gpu.search_end(2)
    assert all(c.untouched() for c in fresh)
    # ... but what the blocking calls refuse whatever the number of queries is refused here too
    with pytest.raises(err, match="batch 0: column 9 is not below"):
        gpu.search_multi_by_label_begin(2, [0, 0], 0, k, ef, [three[0].predicate(columns=[1, 9, 2]), three[1].predicate(columns=[1, 9, 2])],
                                        [0, 0], [0, 0], [0, 0])
    with pytest.raises(err, match="set_width 0 is not within"):
        gpu.search_by_label_begin(2, None, 0, k, ef, sb[0].predicate(width=0), None, None, None)
    with pytest.raises(ValueError, match="predicates has 2 entries for 3 batches"):
        multi_begin(gpu, 2, three, out, [three[0].predicate(), three[1].predicate()])
    gpu.search_end(2)


# ------------------------------------------------------------------------------------------------- 4. re-run rounds
@pytest.mark.parametrize("kind", KINDS)
def test_4_rerun_rounds_keep_each_batchs_predicate(kind):
    """predicates of a handful of rows (the inputs of test_rare_predicates_rerun: three rows of a rare tenant, six timestamps) beside
    wide ones, k 10 / ef 64: the walk rejects nearly every row it meets, its pending candidates outgrow the register queue, and the
    queries are re-run through the launch's work list — a re-run query of batch b must read batch b's predicate again.  48 queries
    as one blocking call (the yardstick, which must itself re-run queries), then as 4 batches of 12 in one launch."""
    ix = base()
    styles = ["rare", "all", "rare", "rare"]
    whole = Chunk(ix, kind, ix.Q[:48], styles, 2500, 10, 64)
    reruns = int(whole.stats[3])
    print(kind, "re-run queries of the blocking call:", reruns)
    assert reruns > 0  # the yardstick itself: without re-run rounds this test would show nothing
    chunks = []
    for b in range(4):
        c = Chunk(ix, kind, ix.Q[12 * b:12 * b + 12], styles, 2500, 10, 64, yardstick=False)
        c.words = {name: np.ascontiguousarray(a[12 * b:12 * b + 12]) for name, a in whole.words.items()}  # its own slice, its own memory
        c.d = {name: _dev(a) for name, a in c.words.items()}
        chunks.append(c)
    assert any(not np.array_equal(chunks[0].words[name], chunks[1].words[name]) for name in whole.words)
    cells = [Cells(12, 10) for _ in range(4)]
    multi_begin(ix.gpu, 1, chunks, cells)
    ix.gpu.search_end(1)
    st = ix.gpu.last_search_stats().copy()
    print(kind, "re-run queries of the multi-batch launch:", int(st[3]))
    for b in range(4):
        same(cells[b].fetch(), tuple(a[12 * b:12 * b + 12] for a in whole.want), (kind, "re-run rounds", b))
    assert int(st[3]) == reruns and int(st[2]) == 48


# ------------------------------------------------------------------------------------------------- 5. limits beyond the registers
@pytest.mark.parametrize("kind", ["set", "box64"])
def test_5_limits_beyond_the_register_lists(kind):
    """the M 8 / M0 16 / ef_construction 700 graph with every seventh row removed, k 600 / ef 1024: candidate lists beyond the
    registers and an unbounded queue, rare and wide predicates interleaved, two batches of 12 in one launch"""
    if "limits" not in _cache:
        _cache["limits"] = Index(4000, 32, 8, 16, 700, 2468, 7, nq=24)
    ix = _cache["limits"]
    chunks = [Chunk(ix, kind, ix.Q[12 * b:12 * b + 12], ["rare", "mixed", "all"], 2520 + b, 600, 1024) for b in range(2)]
    cells = [Cells(12, 600) for _ in range(2)]
    multi_begin(ix.gpu, 3, chunks, cells)
    ix.gpu.search_end(3)
    assert ix.gpu.last_search_shape()[4] != 0  # the list has left the registers
    for b in range(2):
        same(cells[b].fetch(), chunks[b].want, (kind, "limits", b))
        assert cells[b].fetch()[2].max() > 100


# ------------------------------------------------------------------------------------------------- 6. two contexts in flight
def test_6_two_contexts_in_flight():
    ix = base()
    gpu, k, ef = ix.gpu, 10, 64
    a = Chunk(ix, "range", ix.Q[:24], ["mixed", "rare", "all"], 2540, k, ef)        # column 0
    b = Chunk(ix, "box64", ix.Q[24:48], ["mixed", "none", "mixed"], 2541, k, ef)    # columns 1, 3, 2
    ca, cb = Cells(24, k), Cells(24, k)
    gpu.search_by_label_begin(1, a.d_Q.data_ptr(), 24, k, ef, a.predicate(), *ca.ptrs())
    with pytest.raises(gc.pkg().VssError, match="while search context 1 still has a batch in flight"):
        gpu.set_label_column(1, 0, np.zeros(len(ix.cols[1]), dtype=np.uint32))
    gpu.search_by_label_begin(2, b.d_Q.data_ptr(), 24, k, ef, b.predicate(), *cb.ptrs())
    with pytest.raises(gc.pkg().VssError, match="still has a batch in flight"):
        gpu.set_label_column64(3, 0, np.zeros(len(ix.cols[3]), dtype=np.uint64))
    gpu.search_end(2)
    gpu.search_end(1)
    same(ca.fetch(), a.want, "context 1")
    same(cb.fetch(), b.want, "context 2")
    assert ca.fetch()[2].sum() > 0 and cb.fetch()[2].sum() > 0
    again, _ = b.blocking()  # the columns are as they were: the blocking call answers as before
    same(again, b.want, "after the refused writes")


# ------------------------------------------------------------------------------------------------- 7. the blocking calls
def test_7_the_blocking_calls_are_as_they_were():
    ix = base()
    chunks = [Chunk(ix, kind, ix.Q[:35], ["mixed", "all", "none", "rare"], 2560, 10, 64) for kind in KINDS]
    for kind in ("set_box", "eq"):  # a pipelined launch and a multi-batch one on other contexts in between
        flown = five(kind)
        cells = [Cells(13, 10) for _ in range(5)]
        multi_begin(ix.gpu, 3, flown, cells)
        ix.gpu.search_end(3)
        one = Cells(13, 10)
        ix.gpu.search_by_label_begin(1, flown[0].d_Q.data_ptr(), 13, 10, 64, flown[0].predicate(), *one.ptrs())
        ix.gpu.search_end(1)
        same(one.fetch(), flown[0].want, kind)
    for c in chunks:
        after, stats = c.blocking()
        same(after, c.want, c.kind)
        assert np.array_equal(after[0], c.want[0]) and np.array_equal(after[1].view(np.uint32), c.want[1].view(np.uint32))
        assert stats.tolist() == c.stats.tolist()
