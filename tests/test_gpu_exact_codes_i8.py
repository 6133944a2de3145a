"""-m gpu: the exact search answered by bounds from the int8 row codes (set_option("exact.codes_i8", 1); k_exact_bounds_i8,
DESIGN §4.4).  The contract is the f32 path's — every cell equals gpu_common.ExactReference, the brute force of the wave-order
metric on the CPU.  The cases: the tile's indexing edges (with the bounds really selecting), chunks with the folded select and its
overflow repeat, rows and queries without a bound, data the codes cannot separate (the call falls back), a dimension the tile
does not serve, both options, the option switched off again, and the range search's diagnostics left alone."""
import numpy as np
import pytest

import gpu_common as gc
from test_gpu_exact_contract import build, keys_against_slot_order, unit
from test_gpu_exact_split_bf16 import edge_case

pytestmark = pytest.mark.gpu


def codes_index(dim, metric, X, keys, also_split=False):
    gpu = build(dim, metric, X, keys)
    gpu.set_option("exact.codes_i8", 1)
    if also_split:
        gpu.set_option("exact.split_bf16", 1)
    return gpu


@pytest.mark.parametrize("tombstones", [False, True])
@pytest.mark.parametrize("dim", [32, 128, 160, 384])  # a quarter K step; one; one and a quarter; three (odd for the two buffers)
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_contract_at_the_indexing_edges(metric, dim, tombstones):
    X, Q, keys, dead, ref = edge_case(metric, dim, tombstones)
    gpu = codes_index(dim, metric, X, keys)
    if tombstones:
        assert gpu.remove(keys[dead]) == len(dead)
    for k in (1, 10, 100):
        got = gpu.search_batch(Q, k, exact=True)
        kind, launches, slack, rescored = gpu.last_exact_scores()
        print("%s dim %d k %d: slack %.3g, %.1f pairs re-scored per query" % (metric, dim, k, slack, rescored / len(Q)))
        gc.assert_exact_answer(got, ref.top(k), "codes %s dim %d k %d" % (metric, dim, k))
        assert kind == 2 and launches > 0 and gpu.last_exact_fallbacks() == 0
        # the bounds select: a float64 estimate of the real-arithmetic bound leaves at most 400 of the 3000 rows for any query
        assert len(Q) * k <= rescored <= len(Q) * 600


@pytest.mark.parametrize("order", ["random", "descending"])
@pytest.mark.parametrize("metric", ["l2sq", "cosine"])
def test_chunks_and_the_folded_select(metric, order):
    """test_gpu_exact_split_bf16's data: 70 000 rows = two whole 32768-row chunks and a third, the first selected the plain way,
    the rest through the folded select; rows in descending-distance order overflow the survivor buffers and pass A is repeated"""
    dim, n = 64, 70_000
    rng = np.random.default_rng(7100)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = (rng.standard_normal(dim) + 0.05 * rng.standard_normal((8, dim))).astype(np.float32)
    if order == "descending":
        d = ((X - Q[0]) ** 2).sum(1) if metric == "l2sq" else -(unit(X) @ unit(Q[0]))
        X = np.ascontiguousarray(X[np.argsort(-d)])
    keys = keys_against_slot_order(n)
    ref = gc.ExactReference(metric, X, keys, np.arange(n), Q, 200)
    gpu = codes_index(dim, metric, X, keys)
    for k in (10, 200):
        gc.assert_exact_answer(gpu.search_batch(Q, k, exact=True), ref.top(k), "codes chunks %s %s k %d" % (metric, order, k))
        assert gpu.last_exact_scores()[0] == 2 and gpu.last_exact_fallbacks() == 0


def test_rows_and_queries_without_a_bound():
    """all-zero rows have no code and an all-zero query none either: the rows are re-scored for every query, the query looks at
    every row (its radius is +inf) — 1500 matches beside 15 x a few dozen, inside the 16 x 1024 cells"""
    dim, n = 32, 1500
    X, Q = gc.make_data(n, dim, "l2sq", 7300, nq=16)
    X[[5, 700, 1499]] = 0
    Q[3] = 0
    keys = keys_against_slot_order(n)
    ref = gc.ExactReference("l2sq", X, keys, np.arange(n), Q, 10)
    gpu = codes_index(dim, "l2sq", X, keys)
    gc.assert_exact_answer(gpu.search_batch(Q, 10, exact=True), ref.top(10), "zero rows, a zero query")
    assert gpu.last_exact_scores()[0] == 2 and gpu.last_exact_scores()[3] >= n


def test_data_the_codes_cannot_separate_falls_back():
    """3000 rows at 1e-4 around one unit base: every row's lower bound is below every tau, 24 000 pairs for 8 x 1024 cells"""
    dim = 32
    rng = np.random.default_rng(7400)
    base = unit(rng.standard_normal((1, dim)))[0]
    X = (base + 1e-4 * rng.standard_normal((3000, dim))).astype(np.float32)
    Q = (base + 1e-4 * rng.standard_normal((8, dim))).astype(np.float32)
    keys = keys_against_slot_order(len(X))
    ref = gc.ExactReference("l2sq", X, keys, np.arange(len(X)), Q, 10)
    gpu = codes_index(dim, "l2sq", X, keys)
    gc.assert_exact_answer(gpu.search_batch(Q, 10, exact=True), ref.top(10), "inseparable rows")
    assert gpu.last_exact_scores()[0] == 0 and gpu.last_exact_scores()[1] > 0 and gpu.last_exact_scores()[3] == 0


def test_other_dimensions_keep_the_f32_tile():
    dim, n = 100, 3000
    X, Q = gc.make_data(n, dim, "l2sq", 7200, nq=16)
    keys = keys_against_slot_order(n)
    ref = gc.ExactReference("l2sq", X, keys, np.arange(n), Q, 10)
    gpu = codes_index(dim, "l2sq", X, keys)
    gc.assert_exact_answer(gpu.search_batch(Q, 10, exact=True), ref.top(10), "dim 100, option on")
    assert gpu.last_exact_scores()[0] == 0 and gpu.last_exact_scores()[1] > 0


def test_both_options_and_the_option_off_again():
    """kind 2 goes before exact.split_bf16; with both back at 0: the f32 tile, and what an index that never saw them answers"""
    X, Q, keys, _, ref = edge_case("l2sq", 128, False)
    gpu, never = codes_index(128, "l2sq", X, keys, also_split=True), build(128, "l2sq", X, keys)
    gc.assert_exact_answer(gpu.search_batch(Q, 10, exact=True), ref.top(10), "both options")
    assert gpu.last_exact_scores()[0] == 2
    gpu.set_option("exact.codes_i8", 0)
    gpu.search_batch(Q, 10, exact=True)
    assert gpu.last_exact_scores()[0] == 1
    gpu.set_option("exact.split_bf16", 0)
    got, want = gpu.search_batch(Q, 10, exact=True), never.search_batch(Q, 10, exact=True)
    assert gpu.last_exact_scores()[0] == 0 and gpu.last_exact_scores()[:2] == never.last_exact_scores()[:2]
    gc.assert_exact_answer(got, ref.top(10), "options off again")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert gpu.last_exact_fallbacks() == never.last_exact_fallbacks()


def test_the_range_diagnostics_are_left_alone():
    X, Q, keys, _, ref = edge_case("cosine", 128, False)
    gpu = codes_index(128, "cosine", X, keys)
    gpu.search_range_batch(Q[:50], np.full(50, 0.8, dtype=np.float32))
    before = list(gpu.last_range()), gpu.last_range_scores()
    gc.assert_exact_answer(gpu.search_batch(Q, 100, exact=True), ref.top(100), "after a range call")
    assert gpu.last_exact_scores()[0] == 2
    assert (list(gpu.last_range()), gpu.last_range_scores()) == before
