"""-m gpu: pre-scoring on 8-bit row codes (search.prescore; row_codes.h, prescore_bound.h, pool_score in hnsw_kernels.h).
A scoring wave may skip a row's f32 components only if it has proved the row's distance >= the radius of a full list, so with
the option on every answer — ids, distance bits, counts, both work counters per query — must be what it is with the option
off and what the oracle (kernel mode: wave summation order, kernel candidate lists) computes; and vss_last_search_prescore
must show that the filter really ran and really rejected rows.  20 000 rows, batches of 1024 queries: every workgroup runs
several walkers over the mailbox exchange."""
import numpy as np
import pytest

import gpu_common as gc
import golden_cases

pytestmark = pytest.mark.gpu

N, NQ, K = 20000, 1024, 10
M, M0, EFC = 16, 32, 64


def _mixture(dim, normalize=True):
    """bench.py's mixture at the local density of its 10M-row set (about 3 200 rows per cluster): 6 clusters for 20 000 rows"""
    import torch
    import bench
    gen = bench.Mixture(36, dim, normalize, torch.device("cuda", 0))
    assert gen.k == 6
    X = gen.rows(bench.DATA_SEED, 0, N + 1500).cpu().numpy()
    Q = gen.rows(bench.QUERY_SEED, 0, NQ).cpu().numpy()
    return np.ascontiguousarray(X), np.ascontiguousarray(Q)


def _small_integers(dim, seed):
    """components in -3 .. 3, every row present several times, queries that ARE rows: exact ties at the radius in bulk"""
    rng = np.random.default_rng(seed)
    base = rng.integers(-3, 4, size=(N // 8, dim)).astype(np.float32)
    base[np.all(base == 0, axis=1), 0] = 1.0
    X = base[rng.integers(0, len(base), size=N)]
    Q = X[rng.integers(0, N, size=NQ)].copy()
    Q[NQ // 2:] += rng.integers(-1, 2, size=(NQ - NQ // 2, dim)).astype(np.float32)
    Q[np.all(Q == 0, axis=1), 0] = 1.0
    return np.ascontiguousarray(X), np.ascontiguousarray(Q)


def _build(metric, dim, X, n=N):
    gpu = gc.gpu_index(dim, metric, M, M0, EFC)
    gpu.set_option("search.prescore", 1)  # (the default; stated, so that the file also passes under VSS_SEARCH_PRESCORE=0)
    gpu.reserve(n)
    gpu.add(np.arange(n), X[:n])
    return gpu


def _oracle_of(gpu, metric, dim):
    """the oracle over the SAME graph (the engine's stream, which is the reference's format)"""
    cpu = gc.oracle_index(dim, metric, M, M0, EFC)
    cpu.load(gpu.save())
    return cpu


def _search(gpu, Q, k, ef, option, filtered=None):
    if option is not None:
        gpu.set_option("search.prescore", option)
    if filtered is None:
        keys, d, cnt = gpu.search_batch(Q, k, ef)
    else:
        keys, d, cnt = gpu.search_batch_filtered(Q, k, ef, filtered[0], filtered[1])
    return dict(keys=keys, bits=d.view(np.uint32).copy(), cnt=cnt, per_query=gpu.last_query_stats(len(Q)).copy(),
                totals=gpu.last_search_stats()[:2].copy(), pre=gpu.last_search_prescore().copy(), shape=gpu.last_search_shape().copy())


def _same(a, b, what):
    for f in ("keys", "bits", "cnt", "per_query", "totals"):
        assert np.array_equal(a[f], b[f]), (what, f)


def _on_equals_off(gpu, Q, k, ef, what, filtered=None):
    """The index is at option 1 and stays there between calls: the codes this search reads are the ones the index has kept
    valid through whatever happened since (switching the option off drops them, on again encodes every row afresh)."""
    on = _search(gpu, Q, k, ef, None, filtered)
    off = _search(gpu, Q, k, ef, 0, filtered)
    gpu.set_option("search.prescore", 1)
    _same(on, off, what)
    assert off["pre"][0] == 0 and off["pre"][1] == 0 and off["pre"][2] == 0 and off["pre"][3] == 0, (what, off["pre"])
    return on, off


def _equals_oracle(got, cpu, Q, k, ef, what):
    ck, cd, cc, cst = cpu.search_many(Q, k, ef=ef)
    assert np.array_equal(got["keys"], ck), what
    assert np.array_equal(got["bits"], cd.view(np.uint32)), what
    assert np.array_equal(got["cnt"], cc), what
    assert np.array_equal(got["per_query"], cst.astype(np.uint32)), what


def _filter_ran(pre, what, dim):
    active, scored, rejected, held = (int(v) for v in pre)
    print("%s: pre-scored %d rejected %d (%.3f) code bytes %d" % (what, scored, rejected, rejected / max(scored, 1), held))
    assert active == 1 and scored > 0, (what, pre)
    assert rejected / scored >= 0.3, (what, pre)
    assert held >= N * (dim + 16)


_MIX = {}


def _mix(dim):
    """mixture data, the engine's index over it and the oracle over the same graph: built once per dimension, never modified"""
    if dim not in _MIX:
        X, Q = _mixture(dim)
        for a in (X, Q):
            a.setflags(write=False)
        gpu = _build("cosine", dim, X)
        _MIX[dim] = dict(dim=dim, X=X, Q=Q, gpu=gpu, cpu=_oracle_of(gpu, "cosine", dim))
    return _MIX[dim]


@pytest.fixture(scope="module", params=[768, 1536], ids=["dim768", "dim1536"])
def mix(request):
    return _mix(request.param)


@pytest.mark.parametrize("ef", [32, 64])
def test_a_mixture_cosine(mix, ef):
    what = "cosine dim %d ef %d" % (mix["dim"], ef)
    on, _ = _on_equals_off(mix["gpu"], mix["Q"], K, ef, what)
    _equals_oracle(on, mix["cpu"], mix["Q"], K, ef, what)
    _filter_ran(on["pre"], what, mix["dim"])
    assert on["shape"][0] == 1024 and on["shape"][4] == 0 and on["shape"][6] == 0, on["shape"]


def test_a_mixture_cosine_12_wave_kernel():
    """ef 300: the 8-register list, pipelined in 12-wave workgroups.  Option 1 leaves these limits alone (257-512: measured
    slower with the filter); option 2 runs the filter there too, and that path is what is checked here."""
    mix = _mix(768)
    gpu, Q = mix["gpu"], mix["Q"]
    what = "cosine dim 768 ef 300"
    auto = _search(gpu, Q, K, 300, None)
    assert auto["pre"][0] == 0 and auto["pre"][1] == 0 and auto["shape"][0] == 768, (auto["pre"], auto["shape"])
    try:
        on = _search(gpu, Q, K, 300, 2)
        off = _search(gpu, Q, K, 300, 0)
    finally:
        gpu.set_option("search.prescore", 1)
    _same(on, off, what)
    _same(auto, off, what + " (option 1)")
    _equals_oracle(on, mix["cpu"], Q, K, 300, what)
    _filter_ran(on["pre"], what, 768)
    assert on["shape"][0] == 768, on["shape"]


@pytest.mark.parametrize("metric", ["l2sq", "ip", "cosine"])
def test_b_small_integers_and_ties(metric):
    dim = 512
    X, Q = _small_integers(dim, 515)
    gpu = _build(metric, dim, X)
    cpu = _oracle_of(gpu, metric, dim)
    for ef in (32, 64):
        what = "%s small integers ef %d" % (metric, ef)
        on, _ = _on_equals_off(gpu, Q, K, ef, what)
        _equals_oracle(on, cpu, Q, K, ef, what)
        assert on["pre"][0] == 1 and on["pre"][1] > 0, (what, on["pre"])
        print("%s: pre-scored %d rejected %d" % (what, on["pre"][1], on["pre"][2]))


def test_c_codes_stay_valid():
    """build, add, remove + add (slots are reused), compact, save + load: after each step the filter is active again and
    changes nothing"""
    dim = 768
    X, Q = _mixture(dim)
    gpu = gc.gpu_index(dim, "cosine", M, M0, EFC)
    gpu.set_option("search.prescore", 1)
    gpu.reserve(N + 1500)
    gpu.add(np.arange(N), X[:N])

    def step(what):
        on, _ = _on_equals_off(gpu, Q, K, 64, what)
        assert on["pre"][0] == 1 and on["pre"][1] > 0 and on["pre"][2] > 0, (what, on["pre"])
        return on

    step("after the build")
    gpu.add(N + np.arange(1000), X[N:N + 1000])
    step("after vss_add_batch")
    # Slots freed and ALL of them taken over again (five rounds of 40: what the free ring hands back at once), each by a copy of
    # a query: the new row is that query's nearest neighbour, while the code the slot held belongs to an unrelated row whose
    # bound lies beyond the radius of a full list — a stale code would reject the row and change the answer.
    for r in range(5):
        assert gpu.remove(np.arange(1000 + 40 * r, 1040 + 40 * r)) == 40
        gpu.add(40_000 + 40 * r + np.arange(40), Q[40 * r:40 * r + 40])
        assert gpu.size() == gpu.nodes() == N + 1000  # no tombstone left: the search is pipelined and filtered
    on = step("after slot reuse")
    found = int(np.sum(on["keys"][:200, 0] == 40_000 + np.arange(200)))
    print("slot reuse: %d of 200 queries have their own copy first" % found)
    assert found >= 190, found
    # 500 freed, 500 added: what the free ring holds is re-used, the rest is appended and leaves tombstones behind — searches
    # over tombstones are not pipelined and therefore not filtered (until vss_compact has dropped them)
    assert gpu.remove(np.arange(100, 600)) == 500
    gpu.add(50_000 + np.arange(500), X[N + 1000:N + 1500])
    assert gpu.size() == N + 1000 and N + 1000 <= gpu.nodes() < N + 1500
    on, _ = _on_equals_off(gpu, Q, K, 64, "after 500 removed and 500 added")
    assert int(on["pre"][0]) == (1 if gpu.nodes() == gpu.size() else 0), on["pre"]
    assert gpu.remove(np.arange(700, 900)) == 200
    gpu.compact()
    last = step("after vss_compact")
    blob = gpu.save()
    fresh = gc.gpu_index(dim, "cosine", M, M0, EFC)
    fresh.set_option("search.prescore", 1)
    fresh.load(blob)
    on, _ = _on_equals_off(fresh, Q, K, 64, "after save + load")
    assert on["pre"][0] == 1 and on["pre"][2] > 0
    for f in ("keys", "bits", "cnt"):
        assert np.array_equal(on[f], last[f]), ("a loaded index answers like the one that was saved", f)
    assert len(fresh.save()) == len(blob)  # codes are not serialized


def test_d_paths_that_must_not_filter():
    mix = _mix(768)
    gpu, Q = mix["gpu"], mix["Q"]
    # a predicate search
    bm = golden_cases.filter_bitmap(N, 605, 0.5)
    on, _ = _on_equals_off(gpu, Q[:256], K, 64, "predicate", filtered=(bm, N))
    assert on["pre"][0] == 0 and on["pre"][2] == 0, on["pre"]
    # ef 768: the list lives in LDS or HBM, never pipelined
    on, _ = _on_equals_off(gpu, Q[:256], K, 768, "ef 768")
    assert on["pre"][0] == 0 and on["pre"][2] == 0, on["pre"]
    # a 1-query call
    one = gpu.search(Q[0], K, 64)
    pre = gpu.last_search_prescore()
    gpu.set_option("search.prescore", 0)
    assert np.array_equal(one, gpu.search(Q[0], K, 64))
    gpu.set_option("search.prescore", 1)
    assert pre[0] == 0 and pre[2] == 0, pre
    # narrow rows: dim 128
    X, Qn = _mixture(128)
    narrow = _build("cosine", 128, X)
    on, _ = _on_equals_off(narrow, Qn, K, 64, "dim 128")
    assert on["pre"][0] == 0 and on["pre"][2] == 0 and on["pre"][3] == 0, on["pre"]


def test_e_zero_and_nan():
    """A zero query and a NaN query in the batch, a zero row in the index: no bound for any of them (cosine's zero-norm cases,
    NaN), the answers stay what they are.  A row with an infinite component is NOT part of this index: vss_add_batch of such a
    row faults on the device in the build kernels, before any pre-scoring code runs (NaN distances in the candidate lists:
    ADVICE.md, findings on wave_primitives.h) — tests/test_prescore_logic.py checks that the encoder gives such a row no
    code and the bound function refuses it."""
    mix = _mix(768)
    dim = 768
    X = mix["X"][:N].copy()
    X[17] = 0.0
    Q = mix["Q"].copy()
    Q[3] = 0.0
    Q[700, 11] = np.nan
    gpu = _build("cosine", dim, X)
    on, _ = _on_equals_off(gpu, Q, K, 64, "zero / NaN queries, a zero row")
    assert on["pre"][0] == 1 and on["pre"][2] > 0, on["pre"]
