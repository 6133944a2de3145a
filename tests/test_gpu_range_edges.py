"""-m gpu: the branches of the exact range search (vss_search_range_batch*, vss_search_range_batch_by_label_box64*)
that tests/test_gpu_range_search.py and tests/test_gpu_range_label_box.py never enter: more than one query block and more than
two row chunks per call, tiles whose every pair survives, one / odd counts of K steps, an index that changes between calls,
and the degenerate inputs the contract names.  The comparison is theirs: offsets, total and per query the set of (row id, f32
distance bits), every query of every batch, against gpu_common.ExactReference over the rows live at that moment (slots=None;
it reads nothing from the index).  No tolerance anywhere.  The inputs come from range_edge_cases.py;
tests/test_range_edges_inputs.py checks on the CPU that they reach what each case is for."""
import functools

import numpy as np
import pytest

import gpu_common as gc
import range_edge_cases as rec
import test_gpu_range_label_box as label_suite
import test_gpu_range_search as plain_suite
from range_edge_cases import BLOCK, CHUNK
from test_gpu_range_label_box import admitted_mask, radii_and_answer, raw_call, reference
from test_gpu_range_search import assert_range_answer, build, expected, mixed_radii

pytestmark = pytest.mark.gpu


def plain_raw(gpu, Q, radii, capacity, offsets, ids, d, total):
    ptr = (lambda a: None if a is None else a.ctypes.data)  # (the host form through the C ABI itself; None is a NULL pointer)
    return gpu.lib.vss_search_range_batch(gpu.h, ptr(Q), len(Q), ptr(radii), capacity, ptr(offsets), ptr(ids), ptr(d), ptr(total))


def assert_counts_only(call, want, nq, what):
    """the count-only form and one cell short: offsets and total as ever, no cell written.  call(capacity, offsets, ids, d, total)"""
    total = int(want[0][-1])
    offsets, out_total = np.zeros(nq + 1, np.uint64), np.zeros(1, np.uint64)
    assert call(0, offsets, None, None, out_total) == 0, what
    assert np.array_equal(offsets, want[0]) and out_total[0] == total, what
    offsets, ids, d = np.zeros(nq + 1, np.uint64), np.full(total, -7, np.int64), np.full(total, -7, np.float32)
    out_total[0] = 0
    assert call(total - 1, offsets, ids, d, out_total) == 0, what
    assert np.array_equal(offsets, want[0]) and out_total[0] == total and (ids == -7).all() and (d == -7).all(), what


# ------------------------------------------------------------------------------------------------ (a) query blocks x row chunks
@functools.lru_cache(maxsize=1)
def blocks_index(metric):
    c = rec.blocks_case(metric)
    gpu, live = build(rec.A_DIM, metric, c.X, c.keys)
    assert np.array_equal(live, c.live)
    gpu.set_label_column(0, 0, c.tenant)
    return gpu, c


@pytest.mark.parametrize("batch", [BLOCK, BLOCK + 1, rec.A_NQ, "label boxes"])
@pytest.mark.parametrize("metric", ["l2sq", "cosine"])
def test_query_blocks_by_row_chunks(metric, batch):
    """3 row chunks (8192, 8192, 5 slots) x 1, 2 and 3 query blocks: one cand_count word per launch, k_range_offsets with one,
    two and three queries per thread (1024: every thread one; 1025: 513 threads, the last with one query, 511 idle).
    label boxes: BLOCK + 76 queries on tenant 0, whose list is longer than a row chunk — the plan cuts that group across the
    query dimension and its list across the positions; the other queries (two small tenants, an empty box, an absent tenant)
    lie between them."""
    gpu, c = blocks_index(metric)
    if batch == "label boxes":
        got = gpu.search_range_batch_by_label_box64(c.Q, c.box_radii, [0], c.lo, c.hi)
        stats, fstats = gpu.last_range(), gpu.last_range_filtered()
        print("(a) %s label boxes: last_range %s last_range_filtered %s" % (metric, stats, fstats))
        assert_range_answer(got, c.box_want, (metric, batch))
        assert stats[1] == got[3] and stats[2] == 0 and stats[0] >= stats[1]
        assert fstats[1] == sum(len(ids) for ids, _ in c.near)
        tenant0_pairs = rec.A_TENANT0_QUERIES * int(((c.tenant == 0) & c.live).sum())
        assert fstats[2] >= -(-tenant0_pairs // (BLOCK * CHUNK))  # (a launch holds no more pairs than the candidate buffer)
        assert_counts_only(lambda cap, o, i, d, t: raw_call(gpu, c.Q, c.box_radii, [0], 1, c.lo, c.hi, cap, o, i, d, t), c.box_want,
                           rec.A_NQ, (metric, batch))
        return
    nq = batch
    want = rec.prefix(c.want, nq)
    got = gpu.search_range_batch(c.Q[:nq], c.radii[:nq])
    stats = gpu.last_range()
    print("(a) %s %d queries x %d slots: last_range %s" % (metric, nq, rec.A_ROWS, stats))
    assert_range_answer(got, want, (metric, nq))
    assert stats[1] == got[3] == int(want[0][-1]) and stats[2] == 0 and stats[0] >= stats[1]
    if nq == rec.A_NQ:
        Q, radii = np.ascontiguousarray(c.Q[:nq]), np.ascontiguousarray(c.radii[:nq])
        assert_counts_only(lambda cap, o, i, d, t: plain_raw(gpu, Q, radii, cap, o, i, d, t), want, nq, (metric, nq))


# ------------------------------------------------------------------------------------------------ (b) full tiles
@pytest.mark.parametrize("metric", ["ip", "cosine"])
def test_full_tiles(metric):
    """every radius +inf: all 16384 pairs of each of the four dense tiles are staged in the 32 KiB compaction buffer, and in the
    label form all of one 128 x 128 and one 32 x 256 list tile; then the same with the four tile corners removed"""
    c = rec.full_tiles_case(metric)
    gpu = gc.gpu_index(rec.B_DIM, metric, 8, 16, 16)
    gpu.reserve(rec.B_ROWS)
    gpu.set_build_params(32768, 4)
    gpu.add(c.keys, c.X)
    gpu.set_label_column(0, c.first_rowid, c.labels)
    live = np.ones(rec.B_ROWS, bool)
    for corners_gone in (False, True):
        if corners_gone:
            assert gpu.remove(c.keys[rec.B_CORNERS]) == 4
            live[rec.B_CORNERS] = False
        n_live = int(live.sum())
        want, box_want = c.answers(live)
        got = gpu.search_range_batch(c.Q, c.radii)
        stats = gpu.last_range()
        print("(b) %s %d live rows: last_range %s" % (metric, n_live, stats))
        assert stats[0] == stats[1] == rec.B_NQ * n_live == got[3] and stats[2] == 0, stats
        assert_range_answer(got, want, (metric, n_live))
        got = gpu.search_range_batch_by_label_box64(c.Q[:c.box_nq], c.radii[:c.box_nq], [0], c.lo, c.hi)
        stats, fstats = gpu.last_range(), gpu.last_range_filtered()
        print("(b) %s %d live rows, label boxes: last_range %s last_range_filtered %s" % (metric, n_live, stats, fstats))
        assert stats[0] == stats[1] == c.box_nq * n_live == got[3] and fstats[1] == c.box_nq * n_live and fstats[2] >= 2, (stats, fstats)
        assert_range_answer(got, box_want, (metric, n_live, "label boxes"))


# ------------------------------------------------------------------------------------------------ (c) K-step counts
@pytest.mark.parametrize("dim", rec.K_STEP_DIMS + [rec.WIDE_DIM])
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_k_step_counts(metric, dim):
    """1, 1, 1, 2 (the second with one live chunk), 3, 5 and 48 steps of the double-buffered K loop, dense and gathered tile"""
    rows, nq = 130, plain_suite.NQ
    gpu, ref, Q = plain_suite.case(metric, dim, rows)
    radii = mixed_radii(ref, nq)
    got = gpu.search_range_batch(Q, radii)
    stats = gpu.last_range()
    assert_range_answer(got, expected(ref, radii), (metric, dim))
    assert stats[1] == got[3] and stats[2] == 0
    gpu, Q, lo, hi, near = label_suite.case(metric, dim, rows)
    radii, want = radii_and_answer(near)
    got = gpu.search_range_batch_by_label_box64(Q, radii, [0, 1], lo, hi)
    fstats = gpu.last_range_filtered()
    print("(c) %s dim %d (%d steps): last_range %s, label boxes %s %s" % (metric, dim, rec.k_steps(dim), stats, gpu.last_range(), fstats))
    assert_range_answer(got, want, (metric, dim, "label boxes"))
    assert fstats[1] == sum(len(ids) for ids, _ in near) and fstats[2] >= 2


# ------------------------------------------------------------------------------------------------ (d) mutations
@pytest.mark.parametrize("metric", ["l2sq", "cosine"])
def test_row_norms_across_mutations(metric):
    """Both range calls after every step of rec.MutationCase: with a stale |x|^2 (or stale norm extrema) the arrivals, which are
    the expected matches, would be dropped by the tile without a trace."""
    c = rec.MutationCase(metric)
    n, rows, gpu = rec.D_ROWS, {}, None

    def set_columns(index):
        index.set_label_column(0, 0, c.column0)
        index.set_label_column64(1, 0, c.column1)

    for name, removed, added in c.steps():
        if name == "build":
            gpu = gc.gpu_index(rec.D_DIM, metric, 8, 16, 16)
            gpu.reserve(n + 100)
            gpu.set_build_params(32768, 4)
            gpu.add(*added)
            set_columns(gpu)  # row ids 0 .. n + 400: before the arrivals exist
        elif name == "reserve and add past the end":
            at = gpu.nodes()
            gpu.reserve(n + 600)  # reallocates
            gpu.add(*added)
            assert gpu.nodes() == at + 300
        elif name == "save and load":
            fresh = gc.gpu_index(rec.D_DIM, metric, 8, 16, 16)
            fresh.load(gpu.save())
            gpu = fresh
            set_columns(gpu)  # (label columns are not persisted)
        elif name == "compact":
            gpu.compact()
        else:
            if len(removed):
                assert gpu.remove(removed) == len(removed)
            if added is not None:
                gpu.add(*added)
                assert n <= gpu.nodes() < n + 100  # the arrivals took over freed slots
        c.follow(rows, removed, added)
        (radii, want), (box_radii, box_want) = c.answers(rows)
        got = gpu.search_range_batch(c.Q, radii)
        stats = gpu.last_range()
        assert_range_answer(got, want, (metric, name))
        got = gpu.search_range_batch_by_label_box64(c.Q, box_radii, [0, 1], c.lo, c.hi)
        print("(d) %s after %s: last_range %s, label boxes %s %s" % (metric, name, stats, gpu.last_range(), gpu.last_range_filtered()))
        assert_range_answer(got, box_want, (metric, name, "label boxes"))


# ------------------------------------------------------------------------------------------------ (e) degenerate inputs
def assert_zeros(gpu, Q, columns, what):
    """both calls through the C ABI: return code 0, offsets and total zero, no cell written"""
    nq = len(Q)
    radii = np.full(nq, np.inf, np.float32)
    lo, hi = np.zeros((nq, len(columns)), np.uint64), np.full((nq, len(columns)), label_suite.NULL64)
    for form in ("plain", "label boxes"):
        offsets, total = np.full(nq + 1, 7, np.uint64), np.full(1, 7, np.uint64)
        ids, d = np.full(16, -7, np.int64), np.full(16, -7, np.float32)
        if form == "plain":
            rc = plain_raw(gpu, Q, radii, 16, offsets, ids, d, total)
        else:
            rc = raw_call(gpu, Q, radii, columns, len(columns), lo, hi, 16, offsets, ids, d, total)
        assert rc == 0 and (offsets == 0).all() and total[0] == 0 and (ids == -7).all() and (d == -7).all(), (what, form, offsets, total)


@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_nothing_to_answer(metric):
    """n_queries == 0, an index that never received a row, an index whose every row was removed (count > 0, nothing live), and
    five rows added back into it"""
    rng = np.random.default_rng(11)
    X, Q, keys, _ = rec.degenerate_data(metric, "zero row")
    labels = np.zeros(rec.E_ROWS + 5, np.uint32)
    empty = gc.gpu_index(rec.E_DIM, metric, 8, 16, 16)
    empty.set_label_column(0, 0, labels)
    assert_zeros(empty, Q, [0], "an index without rows")
    assert_zeros(empty, Q[:0], [0], "no query, no row")
    gpu, live = build(rec.E_DIM, metric, X, keys)
    gpu.set_label_column(0, 0, labels)
    assert_zeros(gpu, Q[:0], [0], "no query")
    assert gpu.remove(keys[live]) == live.sum()
    assert gpu.size() == 0 and gpu.nodes() == rec.E_ROWS
    assert_zeros(gpu, Q, [0], "every row removed")
    back = rng.standard_normal((5, rec.E_DIM)).astype(np.float32)
    back_keys = np.arange(rec.E_ROWS, rec.E_ROWS + 5, dtype=np.int64)
    gpu.add(back_keys, back)
    ref = gc.ExactReference(metric, back, back_keys, None, Q, 5)
    radii = mixed_radii(ref, rec.E_NQ)
    want = expected(ref, radii)
    assert_range_answer(gpu.search_range_batch(Q, radii), want, (metric, "five rows back"))
    lo, hi = np.zeros((rec.E_NQ, 1), np.uint64), np.zeros((rec.E_NQ, 1), np.uint64)
    assert_range_answer(gpu.search_range_batch_by_label_box64(Q, radii, [0], lo, hi), want, (metric, "five rows back, label boxes"))
    print("(e) %s five rows back: last_range %s last_range_filtered %s" % (metric, gpu.last_range(), gpu.last_range_filtered()))


@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_duplicates_at_the_radius(metric):
    """rows i, i + 128 and i + 256 hold the same vector; the radius is the bits of the distance to it: all three come back with
    those bits, and with the radius one f32 below none of them does"""
    X, Q, keys, live = rec.degenerate_data(metric, "duplicates")
    gpu, built_live = build(rec.E_DIM, metric, X, keys)
    assert np.array_equal(live, built_live)
    gpu.set_label_column(0, 0, np.zeros(rec.E_ROWS, np.uint32))
    lo, hi = np.zeros((rec.E_NQ, 1), np.uint64), np.zeros((rec.E_NQ, 1), np.uint64)
    ref = gc.ExactReference(metric, X[live], keys[live], None, Q, rec.E_ROWS)
    for triples, at, below in rec.duplicate_rounds(ref):
        for radii, present in ((at, True), (below, False)):
            want = expected(ref, radii)
            for got in (gpu.search_range_batch(Q, radii), gpu.search_range_batch_by_label_box64(Q, radii, [0], lo, hi)):
                assert_range_answer(got, want, (metric, present))
                offsets, ids, d, _ = got
                for q in range(rec.E_NQ):
                    mine = slice(int(offsets[q]), int(offsets[q + 1]))
                    hit = np.isin(ids[mine], triples[q])
                    assert hit.sum() == (3 if present else 0), (metric, q, present)
                    assert (d[mine][hit].view(np.uint32) == at[q:q + 1].view(np.uint32)).all(), (metric, q)


@pytest.mark.parametrize("metric", ["l2sq", "ip", "cosine"])
def test_zero_row(metric):
    """one all-zero live row: |x|^2 = 0 is the smallest norm there is.  (Under cosine the engine's distance to it is 1, as the
    reference's: finite, so the contract's rules for NaN and infinite distances have nothing to decide here.)"""
    X, Q, keys, _ = rec.degenerate_data(metric, "zero row")
    gpu, live = build(rec.E_DIM, metric, X, keys)
    assert live[rec.E_ZERO_ROW]
    ref = gc.ExactReference(metric, X[live], keys[live], None, Q, rec.E_ROWS)
    tenant = (keys % 3).astype(np.uint32)
    gpu.set_label_column(0, 0, tenant)
    lo = hi = np.full((rec.E_NQ, 1), rec.E_ZERO_ROW % 3, np.uint64)  # every query's box holds the zero row
    near = reference(ref, admitted_mask([tenant], [0], lo, hi))
    box_radii, box_want = radii_and_answer(near)
    for radii in (mixed_radii(ref, rec.E_NQ), np.full(rec.E_NQ, np.inf, np.float32)):
        assert_range_answer(gpu.search_range_batch(Q, radii), expected(ref, radii), (metric, "zero row"))
        print("(e) %s zero row: last_range %s" % (metric, gpu.last_range()))
    assert_range_answer(gpu.search_range_batch_by_label_box64(Q, box_radii, [0], lo, hi), box_want, (metric, "zero row, label boxes"))
    print("(e) %s zero row, label boxes: last_range %s last_range_filtered %s" % (metric, gpu.last_range(), gpu.last_range_filtered()))
