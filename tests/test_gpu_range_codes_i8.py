"""-m gpu: the exact range search with its rows proposed by the int8 tiles over the row codes (set_option("range.codes_i8", 1),
DESIGN §4.4).  The contract is the f32 tiles': cells, offsets and total equal gpu_common.ExactReference, the CPU brute force of
the wave-order metric; the option may only change how many pairs are proposed."""
import functools
import types

import numpy as np
import pytest

import gpu_common as gc
from test_gpu_range_label_box import CHUNK, admitted_mask, case as box_case, radii_and_answer, reference
from test_gpu_range_search import NQ, assert_range_answer, build, expected, mixed_radii, unit

pytestmark = pytest.mark.gpu


def rows_of(metric, dim, rows, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, dim)).astype(np.float32)
    Q = rng.standard_normal((NQ, dim)).astype(np.float32)
    return (X, Q) if metric == "l2sq" else (unit(X), unit(Q))


@functools.lru_cache(maxsize=1)
def case(metric, dim, rows):
    """test_gpu_range_search's case with the option on"""
    X, Q = rows_of(metric, dim, rows, 500 * dim + rows)
    keys = 1_000_000 - np.arange(rows, dtype=np.int64)
    gpu, live = build(dim, metric, X, keys)
    gpu.set_option("range.codes_i8", 1)
    return gpu, gc.ExactReference(metric, X[live], keys[live], None, Q, rows), Q


@pytest.mark.parametrize("nq", [1, NQ])
@pytest.mark.parametrize("rows", [130, CHUNK + 1])
@pytest.mark.parametrize("dim", [32, 96, 160])  # one MFMA block; a partial K step; a full step and a partial one: both LDS buffers
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_contract_at_the_indexing_edges(metric, dim, rows, nq):
    gpu, ref, Q = case(metric, dim, rows)
    radii = mixed_radii(ref, nq)
    got = gpu.search_range_batch(Q[:nq], radii)
    stats, (kind, launches, slack, _) = gpu.last_range(), gpu.last_range_scores()
    print("%s dim %d rows %d queries %d: slack %.3g, %d candidates, %d matches" % (metric, dim, rows, nq, slack, stats[0], stats[1]))
    assert_range_answer(got, expected(ref, radii), (metric, dim, rows, nq))
    assert kind == 2 and launches == -(-rows // CHUNK) and slack > 0
    assert stats[1] == got[3] and stats[0] >= stats[1] and stats[2] == 0 and gpu.memory_usage() >= stats[3]


@pytest.mark.parametrize("rows", [130, CHUNK + 3000])  # (the larger one: a second run of list positions)
@pytest.mark.parametrize("metric", ["l2sq", "cosine"])
def test_under_label_boxes(metric, rows):
    """boxes named by 1 .. 32 queries take the 32-query shape, the one named by 33 the other"""
    gpu, Q, lo, hi, near = box_case(metric, 96, rows)
    radii, want = radii_and_answer(near)
    gpu.set_option("range.codes_i8", 1)
    try:
        got = gpu.search_range_batch_by_label_box64(Q, radii, [0, 1], lo, hi)
        scores, fstats = gpu.last_range_scores(), gpu.last_range_filtered()
    finally:
        gpu.set_option("range.codes_i8", 0)  # (the index is that module's)
    assert_range_answer(got, want, (metric, rows))
    assert scores[0] == 2 and scores[1] == fstats[2] and fstats[2] >= (3 if rows > CHUNK + 1 else 2)
    assert fstats[1] == sum(len(ids) for ids, _ in near)


@pytest.mark.parametrize("dim", [32, 96])
def test_a_row_only_the_code_bound_keeps(dim):
    """ip.  x* = (1, 0.4 / 127, ...) codes to (127, 0, ...) and is the query too: the integer dot product drops (dim - 1)
    (0.4 / 127)^2 = 3.1e-4 / 9.4e-4 of the score, above the f32 tiles' E (4e-6 / 1.2e-5).  The radius is the pair's distance."""
    rng = np.random.default_rng(dim)
    star = np.full(dim, 0.4 / 127, np.float32)
    star[0] = 1
    X = unit(rng.standard_normal((3000, dim))) * (np.linalg.norm(star) * rng.uniform(0.5, 1.0, (3000, 1))).astype(np.float32)
    X[0] = star
    keys = np.arange(len(X), dtype=np.int64)
    gpu, live = build(dim, "ip", X, keys)
    ref = gc.ExactReference("ip", X[live], keys[live], None, star[None], len(X))
    assert ref.keys[0, 0] == 0
    radii = ref.dist[:1, 0].copy()
    gpu.search_range_batch(star[None], radii)
    E, dropped = gpu.last_range_scores()[2], (dim - 1) * (0.4 / 127) ** 2
    gpu.set_option("range.codes_i8", 1)
    got = gpu.search_range_batch(star[None], radii)
    kind, _, slack, _ = gpu.last_range_scores()
    print("dim %d: the codes drop %.3g, the f32 tiles' E is %.3g, the codes' slack %.3g" % (dim, dropped, E, slack))
    assert_range_answer(got, expected(ref, radii), dim)
    assert 0 in got[1] and kind == 2 and 0 < E < dropped < slack
    # the same row alone inside a one-column box
    tenant = (keys != 0).astype(np.uint32)
    gpu.set_label_column(0, 0, tenant)
    lo = hi = np.zeros((1, 1), np.uint64)
    near = reference(ref, admitted_mask([tenant], [0], lo, hi))
    want = expected(types.SimpleNamespace(keys=[near[0][0]], dist=[near[0][1]]), radii)
    got = gpu.search_range_batch_by_label_box64(star[None], radii, [0], lo, hi)
    assert_range_answer(got, want, "box, dim %d" % dim)
    assert list(got[1]) == [0] and gpu.last_range_scores()[0] == 2 and gpu.last_range_filtered()[1] == 1


@pytest.mark.parametrize("metric", ["l2sq", "cosine"])
def test_rows_with_no_bound(metric):
    """a zero row (no code); under l2sq a row of one huge component (the others code to 0) and one beyond the norm guard.  The
    radii admit them: the distance to the zero row, or to the farthest row"""
    dim, rows, nq = 96, 300, 8
    X, Q = rows_of(metric, dim, rows, 11)
    X[5] = 0
    if metric == "l2sq":
        X[6, 1:] *= 1e-3
        X[6, 0] = 1e4
        X[7] = unit(X[7]) * np.float32(2.0 ** 41)
    keys = np.arange(rows, dtype=np.int64)
    gpu, live = build(dim, metric, X, keys)
    assert live[5] and live[6] and live[7]
    gpu.set_option("range.codes_i8", 1)
    ref = gc.ExactReference(metric, X[live], keys[live], None, Q[:nq], rows)
    radii = np.array([ref.dist[q][ref.keys[q] == 5][0] if q % 2 == 0 else ref.dist[q, -1] for q in range(nq)], np.float32)
    got = gpu.search_range_batch(Q[:nq], radii)
    assert_range_answer(got, expected(ref, radii), metric)
    assert gpu.last_range_scores()[0] == 2 and all(5 in got[1][int(got[0][q]):int(got[0][q + 1])] for q in range(nq))


def test_codes_follow_the_rows():
    """rows added (some inside a query's radius), removed, compacted: each answer is the reference's over the rows live then"""
    dim, rows, nq = 96, 400, 16
    X, Q = rows_of("l2sq", dim, rows + 60, 23)
    Q = Q[:nq]
    keys = np.arange(len(X), dtype=np.int64)
    gpu, live0 = build(dim, "l2sq", X[:rows], keys[:rows])
    gpu.set_option("range.codes_i8", 1)
    live = np.zeros(len(X), bool)
    live[:rows] = live0

    def check(what):
        ref = gc.ExactReference("l2sq", X[live], keys[live], None, Q, len(X))
        assert_range_answer(gpu.search_range_batch(Q, radii), expected(ref, radii), what)
        assert gpu.last_range_scores()[0] == 2, what
        return ref

    radii = np.full(nq, np.inf, np.float32)
    radii = check("as built").dist[:, 4].copy()
    X[rows:rows + nq] = Q + np.float32(0.01) * X[rows:rows + nq]  # inside every query's radius
    gpu.reserve(len(X))  # (the rows move to larger buffers: so do their codes)
    gpu.add(keys[rows:], X[rows:])
    live[rows:] = True
    assert check("rows added").dist[0, 0] < radii[0] * 0.1
    gone = live & (keys % 7 == 2)
    gpu.remove(keys[gone])
    live &= ~gone
    check("rows removed")
    gpu.compact()
    check("compacted")


def test_fall_through_and_off_again():
    """dim 100 keeps the f32 tile; both options at dim 64 run kind 2; back at 0 the index answers as one that never saw the option"""
    gpu, ref, Q = case("l2sq", 100, 130)
    radii = mixed_radii(ref, NQ)
    assert_range_answer(gpu.search_range_batch(Q, radii), expected(ref, radii), "dim 100, option on")
    assert gpu.last_range_scores()[:2] == (0, 1)
    gpu, ref, Q = case("cosine", 64, 130)
    never, _ = build(64, "cosine", rows_of("cosine", 64, 130, 500 * 64 + 130)[0], 1_000_000 - np.arange(130, dtype=np.int64))
    radii = mixed_radii(ref, NQ)
    gpu.set_option("range.split_bf16", 1)
    assert_range_answer(gpu.search_range_batch(Q, radii), expected(ref, radii), "both options")
    assert gpu.last_range_scores()[0] == 2
    gpu.set_option("range.split_bf16", 0)
    gpu.set_option("range.codes_i8", 0)
    got, want = gpu.search_range_batch(Q, radii), never.search_range_batch(Q, radii)
    assert_range_answer(got, expected(ref, radii), "option off again")
    assert np.array_equal(got[0], want[0]) and got[3] == want[3]
    assert np.array_equal(gpu.last_range()[:3], never.last_range()[:3])
    assert gpu.last_range_scores()[0] == 0 and gpu.last_range_scores() == never.last_range_scores()
