"""-m gpu: the greedy descent's rows bounded on their 8-bit codes (search.prescore_descent; descend and PoolScorer in
hnsw_kernels.h).  descend() takes a row only if its distance is strictly smaller than closest_dist, so a scoring
wave that writes +inf for a row proved >= the hop's closest_dist changes nothing: with the option on every answer — keys,
distance bits, counts, both work counters per query — must be what it is with the option off and what the oracle (kernel
mode: wave summation order, kernel candidate lists) computes, and vss_last_search_prescore_descent must show that the descent's
jobs really carried a bound and that rows were really rejected.  20 000 rows, batches of 1024 queries: every workgroup runs 4
walkers over the mailbox exchange."""
import numpy as np
import pytest

import gpu_common as gc
import golden_cases
import test_gpu_prescore as base  # its data generators (mixture, small integers); none of its tests is imported by name
from oracle_lib import parse_stream

pytestmark = pytest.mark.gpu

N, NQ, K = base.N, base.NQ, base.K
SHAPES = {"m16": (16, 32, 64), "m32": (32, 64, 64)}  # M, M0, ef_construction (M 16: 4 graph levels at 20 000 rows)


def _build(metric, dim, X, shape="m16"):
    M, M0, efc = SHAPES[shape]
    gpu = gc.gpu_index(dim, metric, M, M0, efc)
    gpu.set_option("search.prescore", 1)  # (the defaults; stated, so that the file also passes under the environment's 0s)
    gpu.set_option("search.prescore_descent", 1)
    gpu.reserve(N)
    gpu.add(np.arange(N), X[:N])
    return gpu


def _oracle_of(gpu, metric, dim, shape="m16"):
    M, M0, efc = SHAPES[shape]
    cpu = gc.oracle_index(dim, metric, M, M0, efc)
    cpu.load(gpu.save())
    return cpu


def _search(gpu, Q, k, ef, descent, filtered=None):
    gpu.set_option("search.prescore_descent", descent)
    try:
        if filtered is None:
            keys, d, cnt = gpu.search_batch(Q, k, ef)
        else:
            keys, d, cnt = gpu.search_batch_filtered(Q, k, ef, filtered[0], filtered[1])
    finally:
        gpu.set_option("search.prescore_descent", 1)
    return dict(keys=keys, bits=d.view(np.uint32).copy(), cnt=cnt, per_query=gpu.last_query_stats(len(Q)).copy(),
                totals=gpu.last_search_stats()[:2].copy(), pre=gpu.last_search_prescore().copy(),
                desc=gpu.last_search_prescore_descent().copy(), shape=gpu.last_search_shape().copy())


def _on_equals_off(gpu, Q, k, ef, what, filtered=None):
    on = _search(gpu, Q, k, ef, 1, filtered)
    off = _search(gpu, Q, k, ef, 0, filtered)
    base._same(on, off, what)
    assert off["desc"][0] == 0 and off["desc"][1] == 0, (what, off["desc"])
    assert on["pre"][0] == off["pre"][0], (what, on["pre"], off["pre"])  # the switch does not decide which launches carry codes
    return on, off


def _descent_filtered(on, what):
    rows, rejected = (int(v) for v in on["desc"])
    print("%s: descent rows with a bound %d (%.1f per query), rejected %d (%.3f)"
          % (what, rows, rows / NQ, rejected, rejected / max(rows, 1)))
    assert on["pre"][0] == 1 and rows > 0, (what, on["pre"], on["desc"])
    assert rejected / rows >= 0.3, (what, on["desc"])
    # the walkers' count is part of the scoring waves' (rows whose bound was computed / rows rejected there)
    assert rows <= int(on["pre"][1]) and rejected <= int(on["pre"][2]), (what, on["pre"], on["desc"])


_DATA, _INDEX = {}, {}


def _data(dim):
    if dim not in _DATA:
        X, Q = base._mixture(dim)
        for a in (X, Q):
            a.setflags(write=False)
        _DATA[dim] = (X, Q)
    return _DATA[dim]


def _index(metric, dim, shape="m16"):
    """mixture data, the engine's index over it and the oracle over the same graph: built once, never modified"""
    key = (metric, dim, shape)
    if key not in _INDEX:
        X, Q = _data(dim)
        gpu = _build(metric, dim, X, shape)
        _INDEX[key] = dict(X=X, Q=Q, gpu=gpu, cpu=_oracle_of(gpu, metric, dim, shape))
    return _INDEX[key]


@pytest.mark.parametrize("ef", [32, 64])
@pytest.mark.parametrize("dim", [768, 512])
@pytest.mark.parametrize("metric", ["l2sq", "ip", "cosine"])
def test_a_mixture(metric, dim, ef):
    ix = _index(metric, dim)
    assert ix["gpu"].max_level() >= 3, ix["gpu"].max_level()  # 4 graph levels: three levels of descent
    what = "%s dim %d ef %d" % (metric, dim, ef)
    on, _ = _on_equals_off(ix["gpu"], ix["Q"], K, ef, what)
    base._equals_oracle(on, ix["cpu"], ix["Q"], K, ef, what)
    _descent_filtered(on, what)
    assert on["shape"][0] == 1024 and on["shape"][1] >= 2 and on["shape"][6] == 0, on["shape"]  # several walkers per workgroup


def test_a_mixture_m32():
    ix = _index("cosine", 768, "m32")
    what = "cosine dim 768 ef 64, M 32 / M0 64"
    on, _ = _on_equals_off(ix["gpu"], ix["Q"], K, 64, what)
    base._equals_oracle(on, ix["cpu"], ix["Q"], K, 64, what)
    _descent_filtered(on, what)
    assert on["shape"][0] == 1024 and on["shape"][1] >= 2, on["shape"]


@pytest.mark.parametrize("metric", ["l2sq", "ip", "cosine"])
def test_b_ties_and_equality(metric):
    """Small-integer rows, every row present several times.  The first 256 queries are exact copies of rows that sit on upper
    levels of the graph: closest_dist reaches the distance of an exact copy — 0 for l2sq — while copies of the same row at
    exactly that distance are still among the neighbours, and distances exactly equal to closest_dist are met on every level."""
    dim = 512
    X, Q = base._small_integers(dim, 1015)
    gpu = _build(metric, dim, X)
    levels = parse_stream(gpu.save())["levels"]
    upper = np.nonzero(levels[:N] > 0)[0]
    assert len(upper) >= 256, len(upper)
    Q = Q.copy()
    Q[:256] = X[upper[:256]]
    cpu = _oracle_of(gpu, metric, dim)
    for ef in (32, 64):
        what = "%s small integers ef %d" % (metric, ef)
        on, _ = _on_equals_off(gpu, Q, K, ef, what)
        base._equals_oracle(on, cpu, Q, K, ef, what)
        assert on["pre"][0] == 1 and on["desc"][0] > 0, (what, on["pre"], on["desc"])
        print("%s: descent rows with a bound %d rejected %d" % (what, on["desc"][0], on["desc"][1]))


def test_c_zero_and_nan():
    """A zero query and a NaN query in the batch, a zero row in the index: no bound for any of them (a NaN closest_dist
    filters nothing, a row without a bound is never rejected).  No row with an infinite component: the build kernels fault on
    it."""
    dim = 768
    X0, Q0 = _data(dim)
    X = X0[:N].copy()
    X[17] = 0.0
    Q = Q0.copy()
    Q[3] = 0.0
    Q[700, 11] = np.nan
    gpu = _build("cosine", dim, X)
    cpu = _oracle_of(gpu, "cosine", dim)
    what = "zero / NaN queries, a zero row"
    on, _ = _on_equals_off(gpu, Q, K, 64, what)
    # (the NaN query's distances are NaN on both sides, with payload bits that are nobody's contract: it is compared on / off only)
    keep = np.arange(NQ) != 700
    base._equals_oracle({f: on[f][keep] for f in ("keys", "bits", "cnt", "per_query")}, cpu, Q[keep], K, 64, what)
    assert on["pre"][0] == 1 and on["desc"][0] > 0 and on["desc"][1] > 0, (on["pre"], on["desc"])


def test_d_launches_that_must_not_filter():
    ix = _index("cosine", 768)
    gpu, Q = ix["gpu"], ix["Q"]
    # a predicate search
    bm = golden_cases.filter_bitmap(N, 605, 0.5)
    on, _ = _on_equals_off(gpu, Q[:256], K, 64, "predicate", filtered=(bm, N))
    assert on["pre"][0] == 0 and on["desc"][0] == 0 and on["desc"][1] == 0, (on["pre"], on["desc"])
    # ef 768: the list lives in LDS or HBM, never pipelined
    on, _ = _on_equals_off(gpu, Q[:256], K, 768, "ef 768")
    assert on["pre"][0] == 0 and on["desc"][0] == 0 and on["desc"][1] == 0, (on["pre"], on["desc"])
    # a 1-query call
    one = gpu.search(Q[0], K, 64)
    pre, desc = gpu.last_search_prescore(), gpu.last_search_prescore_descent()
    gpu.set_option("search.prescore_descent", 0)
    try:
        assert np.array_equal(one, gpu.search(Q[0], K, 64))
    finally:
        gpu.set_option("search.prescore_descent", 1)
    assert pre[0] == 0 and desc[0] == 0 and desc[1] == 0, (pre, desc)
    # narrow rows: dim 128
    X, Qn = base._mixture(128)
    narrow = _build("cosine", 128, X)
    on, _ = _on_equals_off(narrow, Qn, K, 64, "dim 128")
    assert on["pre"][0] == 0 and on["desc"][0] == 0 and on["desc"][1] == 0, (on["pre"], on["desc"])
    # search.prescore = 0: no codes, so no bound in the descent either, whatever its own switch says
    gpu.set_option("search.prescore", 0)
    try:
        off = _search(gpu, Q, K, 64, 1)
    finally:
        gpu.set_option("search.prescore", 1)
    assert off["pre"][0] == 0 and off["desc"][0] == 0 and off["desc"][1] == 0, (off["pre"], off["desc"])
