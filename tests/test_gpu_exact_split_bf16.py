"""-m gpu: the exact search with its rows selected by the split-bf16 score (set_option("exact.split_bf16", 1);
k_exact_scores_bf16x3).  The contract is the f32 path's — every cell equals gpu_common.ExactReference, the brute
force of the wave-order metric on the CPU — and the option may only change how many queries are redone.  The cases: the tile's
indexing edges, a selection that is really used (no query redone where the reference's own gaps exceed 4 E), data on which the
score cannot decide (it must say so), chunks with the folded select and its overflow repeat, a dimension the tile does not
serve, and the option switched off again."""
import functools

import numpy as np
import pytest

import gpu_common as gc
from test_gpu_exact_contract import build, keys_against_slot_order, unit

pytestmark = pytest.mark.gpu


def split_index(dim, metric, X, keys):
    gpu = build(dim, metric, X, keys)
    gpu.set_option("exact.split_bf16", 1)
    return gpu


@functools.lru_cache(maxsize=None)
def edge_case(metric, dim, tombstones):
    """3000 rows = 23 whole tiles and one of 56; 200 queries = a whole query tile and one of 72; N(0, 1), unit under cosine / ip"""
    rng = np.random.default_rng(7000 + dim)
    X, Q = rng.standard_normal((3000, dim)).astype(np.float32), rng.standard_normal((200, dim)).astype(np.float32)
    if metric != "l2sq":
        X, Q = unit(X), unit(Q)
    keys = keys_against_slot_order(len(X))
    dead = np.arange(3, len(X), 10) if tombstones else np.array([], dtype=np.int64)
    live = np.setdiff1d(np.arange(len(X)), dead)
    return X, Q, keys, dead, gc.ExactReference(metric, X[live], keys[live], live, Q, 100)


@pytest.mark.parametrize("tombstones", [False, True])
@pytest.mark.parametrize("dim", [64, 96])  # two 128-byte steps; three, an odd count for the two LDS buffers
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_contract_at_the_indexing_edges(metric, dim, tombstones):
    X, Q, keys, dead, ref = edge_case(metric, dim, tombstones)
    gpu = split_index(dim, metric, X, keys)
    if tombstones:
        assert gpu.remove(keys[dead]) == len(dead)
    for k in (1, 10, 100):
        got = gpu.search_batch(Q, k, exact=True)
        kind, launches, E, _ = gpu.last_exact_scores()
        redone = gpu.last_exact_fallbacks()
        print("%s dim %d k %d: E %.3g, %d of %d queries redone" % (metric, dim, k, E, redone, len(Q)))
        gc.assert_exact_answer(got, ref.top(k), "split %s dim %d k %d" % (metric, dim, k))
        assert kind == 1 and launches > 0
        if k == 10 and not tombstones:
            # the selection is used, not bypassed: the 10th neighbour and the first row outside K' = 18 are further apart than
            # 4 E for every query (by the reference's own distances), so nothing may have been redone
            gap = (ref.dist[:, 18] - ref.dist[:, 9]).min()
            print("   smallest gap %.3g = %.1f E" % (gap, gap / E))
            assert 0 < E and gap > 4 * E
            assert redone == 0


@pytest.mark.parametrize("case,metric", [("groups", "l2sq"), ("groups", "cosine"), ("offset", "l2sq")])
def test_where_the_score_cannot_decide_it_says_so(case, metric):
    """test_gpu_exact_contract's constructions at dim 64: 4 groups of 60 rows at 1e-4 around unit bases (the order inside a group
    is below any score's error and the group is larger than K': queries must be redone), and rows = c + N(0, 1) with |c| = 8192"""
    dim = 64
    rng = np.random.default_rng(2000 + dim)
    if case == "groups":
        bases = unit(rng.standard_normal((4, dim)))
        groups = np.concatenate([b + 1e-4 * rng.standard_normal((60, dim)) for b in bases]).astype(np.float32)
        X = np.concatenate([unit(rng.standard_normal((2000, dim))), groups])
        X = np.ascontiguousarray(X[rng.permutation(len(X))])
        Q = np.concatenate([b + 1e-4 * rng.standard_normal((2, dim)) for b in bases]).astype(np.float32)
    else:
        c = unit(rng.standard_normal(dim)) * np.float32(8192.0)
        X = (c + rng.standard_normal((3000, dim))).astype(np.float32)
        Q = (c + rng.standard_normal((8, dim))).astype(np.float32)
    keys = keys_against_slot_order(len(X))
    ref = gc.ExactReference(metric, X, keys, np.arange(len(X)), Q, 40)
    gpu = split_index(dim, metric, X, keys)
    for k in (10, 40):
        got = gpu.search_batch(Q, k, exact=True)
        gc.assert_exact_answer(got, ref.top(k), "split %s %s k %d" % (case, metric, k))
        assert gpu.last_exact_scores()[0] == 1 and (case == "offset" or gpu.last_exact_fallbacks() > 0)


@pytest.mark.parametrize("order", ["random", "descending"])
@pytest.mark.parametrize("metric", ["l2sq", "cosine"])
def test_chunks_and_the_folded_select(metric, order):
    """70 000 rows = two whole 32768-row chunks and a third: the first is selected the plain way, the rest through the select
    folded into the tile's epilogue; rows in descending-distance order overflow the survivor buffers and the pass is repeated"""
    dim, n = 64, 70_000
    rng = np.random.default_rng(7100)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = (rng.standard_normal(dim) + 0.05 * rng.standard_normal((8, dim))).astype(np.float32)
    if order == "descending":
        d = ((X - Q[0]) ** 2).sum(1) if metric == "l2sq" else -(unit(X) @ unit(Q[0]))
        X = np.ascontiguousarray(X[np.argsort(-d)])
    keys = keys_against_slot_order(n)
    ref = gc.ExactReference(metric, X, keys, np.arange(n), Q, 200)
    gpu = split_index(dim, metric, X, keys)
    for k in (10, 200):
        gc.assert_exact_answer(gpu.search_batch(Q, k, exact=True), ref.top(k), "split chunks %s %s k %d" % (metric, order, k))
        assert gpu.last_exact_scores()[0] == 1


def test_other_dimensions_keep_the_f32_tile():
    dim, n = 100, 3000
    X, Q = gc.make_data(n, dim, "l2sq", 7200, nq=16)
    keys = keys_against_slot_order(n)
    ref = gc.ExactReference("l2sq", X, keys, np.arange(n), Q, 10)
    gpu = split_index(dim, "l2sq", X, keys)
    gc.assert_exact_answer(gpu.search_batch(Q, 10, exact=True), ref.top(10), "dim 100, option on")
    assert gpu.last_exact_scores()[0] == 0 and gpu.last_exact_scores()[1] > 0


def test_option_off_again():
    """the same index with the option back at 0: the f32 tile, and what an index that never saw the option answers"""
    X, Q, keys, _, ref = edge_case("l2sq", 64, False)
    gpu, never = split_index(64, "l2sq", X, keys), build(64, "l2sq", X, keys)
    gpu.search_batch(Q, 10, exact=True)
    assert gpu.last_exact_scores()[0] == 1
    gpu.set_option("exact.split_bf16", 0)
    got, want = gpu.search_batch(Q, 10, exact=True), never.search_batch(Q, 10, exact=True)
    assert gpu.last_exact_scores()[0] == 0 and gpu.last_exact_scores()[:2] == never.last_exact_scores()[:2]
    gc.assert_exact_answer(got, ref.top(10), "option off again")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert gpu.last_exact_fallbacks() == never.last_exact_fallbacks()
