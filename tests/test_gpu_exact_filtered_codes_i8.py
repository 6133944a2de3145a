"""-m gpu: the exact search under per-query predicates answered by bounds from the int8 row codes, gathered through the
predicates' lists (set_option("exact.filtered_codes_i8", 1); k_exact_filtered_bounds_i8).  The contract is the
metric kernel's — every cell equals gpu_common.ExactReference over the admitted live rows with their slots.  The cases: the
tile's edges in both shapes (with the bounds really selecting), chunks, the other entry points, the calls that fall back, the
option switched off again, and the other searches' diagnostics left alone."""
import functools

import numpy as np
import pytest

import gpu_common as gc
from test_gpu_exact_contract import build, unit

pytestmark = pytest.mark.gpu

N, NO_LABEL, OPTION = 3000, 0xFFFFFFFF, "exact.filtered_codes_i8"
# label 3: 2695 rows and 150 queries (a tall tile of 128 and a small one of 22); label 0: 300 rows = 2 x 128 + 44 = 256 + 44 and
# 33 queries (the smallest tall tile); label 1: 5 rows, fewer than k; label 2: no row; NO_LABEL: wants nothing
WANT = [3] * 150 + [0] * 33 + [1, 2, NO_LABEL]


def keys_of(n):
    """keys DESCEND with the slot (an order by key is caught) and stay below n: the label column has one cell per key"""
    return n - 1 - np.arange(n, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def labelled_case(metric, dim, tombstones):
    rng = np.random.default_rng(7500 + dim)
    X, Q = rng.standard_normal((N, dim)).astype(np.float32), rng.standard_normal((len(WANT), dim)).astype(np.float32)
    if metric != "l2sq":
        X, Q = unit(X), unit(Q)
    perm, label = rng.permutation(N), np.full(N, 3, dtype=np.uint32)  # by slot, scattered: the lists really gather
    label[perm[:300]], label[perm[300:305]] = 0, 1
    want = np.array(WANT, dtype=np.uint32)[rng.permutation(len(WANT))]  # the group order is not the query order
    dead = np.arange(3, N, 10) if tombstones else np.array([], dtype=np.int64)
    live, keys, refs = np.setdiff1d(np.arange(N), dead), keys_of(N), []
    for v in (0, 1, 3):
        rows, qs = live[label[live] == v], np.nonzero(want == v)[0]
        refs.append((qs, gc.ExactReference(metric, X[rows], keys[rows], rows, Q[qs], 100)))
    return X, Q, keys, dead, label, want, refs


def expected(case, k):
    keys, dist, cnt = np.full((len(case[1]), k), -1, np.int64), np.full((len(case[1]), k), np.inf, np.float32), np.zeros(len(case[1]), np.uint32)
    for qs, ref in case[6]:
        keys[qs], dist[qs], cnt[qs] = ref.top(k)
    return keys, dist, cnt


def labelled_index(metric, X, keys, label, dead=(), option=1):
    gpu = build(X.shape[1], metric, X, keys)
    gpu.set_labels(0, label[::-1])  # (key = n - 1 - slot)
    gpu.set_option(OPTION, option)
    if len(dead):
        assert gpu.remove(keys[dead]) == len(dead)
    return gpu


@pytest.mark.parametrize("tombstones", [False, True])
@pytest.mark.parametrize("dim", [32, 128, 160, 384])  # a quarter K step; one; one and a quarter; three (odd for the two buffers)
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_tile_edges(metric, dim, tombstones):
    case = labelled_case(metric, dim, tombstones)
    X, Q, keys, dead, label, want, refs = case
    gpu = labelled_index(metric, X, keys, label, dead)
    for k in (1, 10, 100):
        got = gpu.search_batch_by_label(Q, k, 64, want, mode="exact")
        kind, launches, slack, rescored = gpu.last_exact_filtered_scores()
        pairs = int(gpu.last_exact_filtered()[1])
        print("%s dim %d k %d: slack %.3g, %d of %d pairs re-scored" % (metric, dim, k, slack, rescored, pairs))
        gc.assert_exact_answer(got[:3], expected(case, k), "lists %s dim %d k %d" % (metric, dim, k))
        assert kind == 2 and launches > 0  # (0, 0 without the feature)
        # the bounds select: every admitted top-k row is re-scored, and far from every listed pair (test_gpu_exact_codes_i8's
        # float64 estimate of the bound on this very distribution: at most 600 of 3000 rows per query, here 150 x 2695 + ...)
        assert pairs == sum(len(qs) * ref.n for qs, ref in refs)
        assert sum(len(qs) * min(k, ref.n) for qs, ref in refs) <= rescored < pairs


@pytest.mark.parametrize("order", ["random", "descending"])
def test_chunks(order):
    """one label admits about 70 000 of 75 000 rows: two whole 32768-position chunks and a third; rows in descending-distance
    order fill the select's buffer in every chunk"""
    dim, n = 64, 75_000
    rng = np.random.default_rng(7600)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = (rng.standard_normal(dim) + 0.05 * rng.standard_normal((8, dim))).astype(np.float32)
    if order == "descending":
        X = np.ascontiguousarray(X[np.argsort(-((X - Q[0]) ** 2).sum(1))])
    label, keys = np.where(rng.random(n) < 14 / 15, 7, 1).astype(np.uint32), keys_of(n)
    rows = np.nonzero(label == 7)[0]
    ref = gc.ExactReference("l2sq", X[rows], keys[rows], rows, Q, 200)
    gpu = labelled_index("l2sq", X, keys, label)
    for k in (10, 200):
        got = gpu.search_batch_by_label(Q, k, 64, np.full(8, 7, dtype=np.uint32), mode="exact")
        gc.assert_exact_answer(got[:3], ref.top(k), "list chunks %s k %d" % (order, k))
        assert gpu.last_exact_filtered_scores()[0] == 2 and gpu.last_exact_filtered_scores()[1] == 3


def test_other_entry_points():
    case = labelled_case("cosine", 160, True)
    X, Q, keys, dead, label, want, _ = case
    gpu, exp = labelled_index("cosine", X, keys, label, dead), expected(case, 10)
    bitmaps = np.zeros((4, (N + 63) // 64), dtype=np.uint64)  # row v admits label v's keys; row 2 admits nothing
    for v in (0, 1, 3):
        ks = keys[label == v]
        np.bitwise_or.at(bitmaps[v], ks >> 6, np.uint64(1) << (ks & 63).astype(np.uint64))
    got = gpu.search_exact_batch_filtered_groups(Q, 10, bitmaps, N, np.where(want == NO_LABEL, 2, want))
    gc.assert_exact_answer(got, exp, "bitmaps")
    assert gpu.last_exact_filtered_scores()[0] == 2
    ends = np.where(want == NO_LABEL, 999, want).astype(np.uint64)[:, None]
    gc.assert_exact_answer(gpu.search_batch_by_label_box64(Q, 10, 64, [0], ends, ends, mode="exact")[:3], exp, "box64")
    assert gpu.last_exact_filtered_scores()[0] == 2
    # auto: len^2 * 64 <= C * live * 64 routes the lists of at most 300 rows exact and walks the tenant of 2695
    on = gpu.search_batch_by_label(Q, 10, 64, want, mode="auto", route_c=100)
    assert gpu.last_exact_filtered_scores()[0] == 2
    gpu.set_option(OPTION, 0)
    off = gpu.search_batch_by_label(Q, 10, 64, want, mode="auto", route_c=100)
    x = on[3] != 0
    assert np.array_equal(on[3], off[3]) and np.array_equal(x, want != 3) and np.all(on[3][np.isin(want, [0, 1, 2])] == 1)
    gc.assert_exact_answer([a[x] for a in on[:3]], [a[x] for a in exp], "auto, exact-routed")
    assert all(np.array_equal(a[~x].view(np.uint32), b[~x].view(np.uint32)) for a, b in zip(on[:3], off[:3])), "auto, graph-routed"


def one_label_data(what):
    if what == "inseparable":  # test_data_the_codes_cannot_separate_falls_back's: 24 000 pairs for 8 x 1024 cells
        rng = np.random.default_rng(7400)
        base = unit(rng.standard_normal((1, 32)))[0]
        return (base + 1e-4 * rng.standard_normal((3000, 32))).astype(np.float32), (base + 1e-4 * rng.standard_normal((8, 32))).astype(np.float32)
    if what == "dim 100":
        return gc.make_data(3000, 100, "l2sq", 7200, nq=16)
    X, Q = gc.make_data(1500, 32, "l2sq", 7300, nq=16)  # rows and a query without a bound
    X[[5, 700, 1499]], Q[3] = 0, 0
    return X, Q


@pytest.mark.parametrize("what,kind", [("inseparable", 0), ("dim 100", 0), ("zeros", 2)])
def test_falls_back_where_it_must(what, kind):
    X, Q = one_label_data(what)
    keys = keys_of(len(X))
    ref = gc.ExactReference("l2sq", X, keys, np.arange(len(X)), Q, 10)
    gpu = labelled_index("l2sq", X, keys, np.full(len(X), 5, dtype=np.uint32))
    got = gpu.search_batch_by_label(Q, 10, 64, np.full(len(Q), 5, dtype=np.uint32), mode="exact")
    gc.assert_exact_answer(got[:3], ref.top(10), what)
    scores = gpu.last_exact_filtered_scores()
    assert scores[0] == kind and (scores[1:] == [0, 0.0, 0] if kind == 0 else scores[3] >= len(X))


def test_option_off_again_and_other_diagnostics():
    case = labelled_case("cosine", 128, False)
    X, Q, keys, _, label, want, _ = case
    gpu, never = labelled_index("cosine", X, keys, label), labelled_index("cosine", X, keys, label, option=0)
    ends = want.astype(np.uint64)[:50, None]
    gpu.search_range_batch_by_label_box64(Q[:50], np.full(50, 0.8, dtype=np.float32), [0], ends, ends)
    gpu.search_batch(Q, 10, exact=True)
    before = list(gpu.last_range()), gpu.last_range_scores(), list(gpu.last_range_filtered()), gpu.last_exact_scores()
    gc.assert_exact_answer(gpu.search_batch_by_label(Q, 100, 64, want, mode="exact")[:3], expected(case, 100), "after a range call")
    assert gpu.last_exact_filtered_scores()[0] == 2
    assert (list(gpu.last_range()), gpu.last_range_scores(), list(gpu.last_range_filtered()), gpu.last_exact_scores()) == before
    by_bounds = list(gpu.last_exact_filtered()[:3])
    gpu.set_option(OPTION, 0)
    got, base = gpu.search_batch_by_label(Q, 100, 64, want, mode="exact"), never.search_batch_by_label(Q, 100, 64, want, mode="exact")
    assert gpu.last_exact_filtered_scores() == never.last_exact_filtered_scores() == [0, 0, 0.0, 0]
    assert by_bounds == list(gpu.last_exact_filtered()[:3]) == list(never.last_exact_filtered()[:3])
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got[:3], base[:3]))
