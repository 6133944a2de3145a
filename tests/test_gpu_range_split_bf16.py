"""-m gpu: the exact range search with its rows proposed by the split-bf16 score (set_option("range.split_bf16", 1);
k_range_candidates_bf16x3 and k_range_candidates_lists_bf16x3).  The contract is the f32 tiles': per query the
set of (row id, distance bits), the offsets and the total equal gpu_common.ExactReference, the brute force of the wave-order
metric on the CPU.  The option may only change how many pairs are proposed."""
import functools
import types

import numpy as np
import pytest

import gpu_common as gc
from test_gpu_range_label_box import CHUNK, admitted_mask, case as box_case, radii_and_answer, reference
from test_gpu_range_search import NQ, assert_range_answer, build, expected, mixed_radii, unit

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def case(metric, dim, rows):
    """test_gpu_range_search's case with the option on: index (a tenth of the rows removed), reference over the live rows, queries"""
    rng = np.random.default_rng(300 * dim + rows)
    X = rng.standard_normal((rows, dim)).astype(np.float32)
    Q = rng.standard_normal((NQ, dim)).astype(np.float32)
    if metric != "l2sq":
        X, Q = unit(X), unit(Q)
    keys = 1_000_000 - np.arange(rows, dtype=np.int64)
    gpu, live = build(dim, metric, X, keys)
    gpu.set_option("range.split_bf16", 1)
    return gpu, gc.ExactReference(metric, X[live], keys[live], None, Q, rows), Q


@pytest.mark.parametrize("nq", [1, NQ])
@pytest.mark.parametrize("rows", [130, CHUNK + 1])
@pytest.mark.parametrize("dim", [64, 96])  # two 128-byte steps; three, an odd count for the two LDS buffers
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_contract_at_the_indexing_edges(metric, dim, rows, nq):
    gpu, ref, Q = case(metric, dim, rows)
    radii = mixed_radii(ref, nq)
    got = gpu.search_range_batch(Q[:nq], radii)
    stats, (kind, launches, E, _) = gpu.last_range(), gpu.last_range_scores()
    print("%s dim %d rows %d queries %d: E %.3g, %d candidates, %d matches" % (metric, dim, rows, nq, E, stats[0], stats[1]))
    assert_range_answer(got, expected(ref, radii), (metric, dim, rows, nq))
    assert kind == 1 and launches == -(-rows // CHUNK) and E > 0
    assert stats[1] == got[3] and stats[0] >= stats[1] and stats[2] == 0 and gpu.memory_usage() >= stats[3]


@pytest.mark.parametrize("rows", [130, CHUNK + 3000])  # (the larger one: a second run of list positions)
@pytest.mark.parametrize("metric", ["l2sq", "cosine"])
def test_under_label_boxes(metric, rows):
    """test_gpu_range_label_box's case: boxes named by 1 .. 32 queries take the 32-query shape, the one named by 33 the other"""
    gpu, Q, lo, hi, near = box_case(metric, 96, rows)
    radii, want = radii_and_answer(near)
    gpu.set_option("range.split_bf16", 1)
    try:
        got = gpu.search_range_batch_by_label_box64(Q, radii, [0, 1], lo, hi)
        scores, fstats = gpu.last_range_scores(), gpu.last_range_filtered()
    finally:
        gpu.set_option("range.split_bf16", 0)  # (the index is that module's)
    assert_range_answer(got, want, (metric, rows))
    assert scores[0] == 1 and scores[1] == fstats[2] and fstats[2] >= (3 if rows > CHUNK + 1 else 2)
    assert fstats[1] == sum(len(ids) for ids, _ in near)


@pytest.mark.parametrize("dim", [64, 96])
def test_a_row_only_the_split_bound_keeps(dim):
    """ip.  x* = (1 + 2^-8) 1 splits into hi = 1, lo = 2^-8, and the query is x* itself: the score drops lo.lo, dim 2^-16 in all
    (9.8e-4 / 1.46e-3), which is above the f32 tiles' E (5.0e-4 / 1.1e-3 at these norms) and below the split score's (4.7e-3 /
    8.4e-3).  The radius is exactly the pair's distance, so a threshold built from the f32 E loses the row."""
    rng = np.random.default_rng(dim)
    star = np.full(dim, 1 + 2.0 ** -8, np.float32)
    X = unit(rng.standard_normal((3000, dim))) * (np.linalg.norm(star) * rng.uniform(0.5, 1.0, (3000, 1))).astype(np.float32)
    X[0] = star
    keys = np.arange(len(X), dtype=np.int64)
    gpu, live = build(dim, "ip", X, keys)
    gpu.set_option("range.split_bf16", 1)
    ref = gc.ExactReference("ip", X[live], keys[live], None, star[None], len(X))
    assert ref.keys[0, 0] == 0
    radii = ref.dist[:1, 0].copy()
    got = gpu.search_range_batch(star[None], radii)
    assert_range_answer(got, expected(ref, radii), dim)
    kind, _, E, _ = gpu.last_range_scores()
    assert 0 in got[1] and kind == 1 and E > dim * 2.0 ** -16
    # the same row inside a box
    tenant = (keys % 3).astype(np.uint32)
    gpu.set_label_column(0, 0, tenant)
    lo = hi = np.zeros((1, 1), np.uint64)
    near = reference(ref, admitted_mask([tenant], [0], lo, hi))
    want = expected(types.SimpleNamespace(keys=[near[0][0]], dist=[near[0][1]]), radii)
    got = gpu.search_range_batch_by_label_box64(star[None], radii, [0], lo, hi)
    assert_range_answer(got, want, "box, dim %d" % dim)
    assert 0 in got[1] and gpu.last_range_scores()[0] == 1 and gpu.last_range_scores()[2] == E


def test_other_dimensions_keep_the_f32_tiles():
    gpu, ref, Q = case("l2sq", 100, 130)
    radii = mixed_radii(ref, NQ)
    assert_range_answer(gpu.search_range_batch(Q, radii), expected(ref, radii), "dim 100, option on")
    assert gpu.last_range_scores()[:2] == (0, 1)


def test_option_off_again():
    """the same index with the option back at 0: the f32 tile, and what an index that never saw the option answers"""
    gpu, ref, Q = case("cosine", 64, 130)
    rng = np.random.default_rng(300 * 64 + 130)  # (case's rows again, for the second index)
    X = unit(rng.standard_normal((130, 64)).astype(np.float32))
    never, _ = build(64, "cosine", X, 1_000_000 - np.arange(130, dtype=np.int64))
    radii = mixed_radii(ref, NQ)
    gpu.search_range_batch(Q, radii)
    assert gpu.last_range_scores()[0] == 1
    gpu.set_option("range.split_bf16", 0)
    try:
        got, want = gpu.search_range_batch(Q, radii), never.search_range_batch(Q, radii)
    finally:
        gpu.set_option("range.split_bf16", 1)  # (as case() hands it out)
    assert_range_answer(got, expected(ref, radii), "option off again")
    assert np.array_equal(got[0], want[0]) and got[3] == want[3]
    assert_range_answer(want, expected(ref, radii), "never on")
    assert np.array_equal(gpu.last_range()[:3], never.last_range()[:3])
    assert gpu.last_range_scores()[0] == 0 and gpu.last_range_scores() == never.last_range_scores()
