"""-m gpu: the candidate list of search limits 513-4096 kept in LDS (LdsList, k_search<.., LDS_LIST_E>) against the oracle:
ids, distance bits, counts and work counters, for every limit at which the list takes another path, over data in which
every vector appears three times (exact ties in bulk: "a new entry goes before equal distances"), with the list overflowing
(about 4450 distances per query), and the same through the list in HBM (search.list_lds = 0)."""
import numpy as np
import pytest

import datagen
import golden_cases
import gpu_common as gc

pytestmark = pytest.mark.gpu

N, NQ = 4500, 40
LDS_PER_CU = 160 * 1024
SHAPES = [("l2sq", 16), ("cosine", 96)]
LDS_LIMITS = [(10, 513), (10, 576), (10, 577), (10, 1024), (10, 1536), (2047, 0), (10, 4096)]
HBM_LIMITS = [(10, 4097), (5000, 16)]  # capacity = min(limit, rows) = 4500: beyond the LDS list


def _data(metric, dim):
    norm = metric != "l2sq"
    X = datagen.mixture(N, dim, 8642, normalize=norm)
    X = np.ascontiguousarray(X[np.arange(N) % (N // 3)])
    Q = datagen.mixture(600, dim, 8643, n_clusters=67, normalize=norm)
    return X, Q


def _build(metric, dim):
    X, Q = _data(metric, dim)
    cpu, gpu = gc.oracle_index(dim, metric, 8, 16, 64), gc.gpu_index(dim, metric, 8, 16, 64)
    cpu.reserve(N), gpu.reserve(N)
    cpu.build_batch(np.arange(N), X, 64, 4)
    gpu.set_build_params(64, 4)
    gpu.add(np.arange(N), X)
    diff = gc.first_graph_difference(gpu.save(), cpu.save())
    assert diff is None, diff
    return cpu, gpu, Q


class Pair:
    def __init__(self, metric, dim):
        self.metric, self.dim = metric, dim
        self.cpu, self.gpu, self.Q = _build(metric, dim)
        self.want = {}

    def oracle(self, k, ef, nq=NQ):
        """the oracle's answer, computed once per (k, ef, queries) and never modified"""
        key = (k, ef, nq)
        if key not in self.want:
            r = self.cpu.search_many(self.Q[:nq], k, ef=ef if ef else None)
            for a in r:
                a.setflags(write=False)
            self.want[key] = r
        return self.want[key]

    def options(self, list_lds=2, walkers=0, waves=16, visited_lds_log2_max=0, solo=0):
        g = self.gpu
        g.set_search_params(waves, walkers)
        g.set_option("search.solo", solo)
        g.set_option("search.visited_lds_log2_max", visited_lds_log2_max)
        g.set_option("search.list_lds", list_lds)

    def check(self, k, ef, placement, nq=NQ):
        got = self.gpu.search_batch(self.Q[:nq], k, ef)
        stats = self.gpu.last_query_stats(nq)
        shape = self.gpu.last_search_shape()
        ck, cd, cc, cst = self.oracle(k, ef, nq)
        assert np.array_equal(got[0], ck), (k, ef)
        assert np.array_equal(got[1].view(np.uint32), cd.view(np.uint32)), (k, ef)
        assert np.array_equal(got[2], cc), (k, ef)
        assert np.array_equal(stats, cst.astype(np.uint32)), (k, ef)
        assert shape[4] == placement, (k, ef, shape)
        assert shape[3] <= LDS_PER_CU and shape[6] == 0 and shape[7] == 0, shape
        return got, stats, shape


def _align16(x):
    return (x + 15) & ~15


HEADER = 48 + 16 * 32 + 64 * 8  # ENGINE_HEADER_BYTES


def _slot_bytes(dim):
    """A walker's slot for this file's index (engine_slot_bytes, engine_layout.h): M0 16 and a visited set of 2^13 cells in
    LDS — what holds every row of the index."""
    return (4 << 13) + _align16(16 * ((dim + 3) // 4)) + 4 * _align16(4 * 16)


def _walkers_that_fit(dim, cells, cap=8):
    return min(cap, (LDS_PER_CU - HEADER) // (_slot_bytes(dim) + 2 * _align16(4 * cells) + 256))


def _expected_default_placement(dim, cells, n_queries, n_cus):
    """The automatic rule (host_logic.h candidate_list_placement): four walkers at most, sixteen waves."""
    today = max(1, min((n_queries + n_cus - 1) // n_cus, 4, (LDS_PER_CU - HEADER) // _slot_bytes(dim)))
    return (1 if _walkers_that_fit(dim, cells, 4) >= today else 2), today


@pytest.fixture(scope="module", params=SHAPES, ids=["%s-%d" % s for s in SHAPES])
def pair(request):
    return Pair(*request.param)


@pytest.mark.parametrize("k,ef", LDS_LIMITS)
def test_lds_list_equals_the_oracle_and_the_hbm_list(pair, k, ef):
    """One entry past the register list, a tile boundary and its successor, the benchmark's ef, the reference's largest k,
    the largest LDS list — forced into LDS, then the same launch with the list in HBM: bit-equal to the oracle and to each
    other."""
    pair.options(list_lds=2)
    lds, lds_stats, shape = pair.check(k, ef, 1)
    assert shape[1] >= 1 and shape[0] == 1024
    if ef == 1536:  # the list overflows: the full-list path (drop the last entry) runs, not just the filling path
        assert int(lds_stats[:, 0].min()) > 1536
    pair.options(list_lds=0)
    hbm, hbm_stats, _ = pair.check(k, ef, 2)
    for a, b in zip(lds, hbm):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    assert np.array_equal(lds_stats, hbm_stats)


@pytest.mark.parametrize("k,ef", HBM_LIMITS)
def test_capacities_beyond_the_lds_list_stay_in_hbm(pair, k, ef):
    for mode in (2, 1, 0):
        pair.options(list_lds=mode)
        pair.check(k, ef, 2)


@pytest.mark.parametrize("walkers,waves", [(1, 16), (2, 16), (4, 16), (1, 8), (4, 8), (0, 8)])
def test_lds_list_in_every_workgroup_shape(pair, walkers, waves):
    """Walkers and scoring waves compute the slot stride separately: every combination must find the mailbox buffers."""
    pair.options(list_lds=2, walkers=walkers, waves=waves)
    _, _, shape = pair.check(10, 1024, 1)
    assert shape[0] == 64 * waves
    if walkers:  # as many as asked for, or as fit next to the index's 32-KiB visited set and the list (three at 1024 entries)
        assert shape[1] == min(walkers, _walkers_that_fit(pair.dim, 1024))


def test_list_state_does_not_leak_between_queries(pair):
    """600 queries over one walker per workgroup: every walker answers several queries in a row."""
    pair.options(list_lds=2, walkers=1)
    _, _, shape = pair.check(10, 1024, 1, nq=600)
    assert shape[1] == 1 and shape[2] < 600


@pytest.mark.parametrize("k,ef", [(10, 1536), (10, 4096)])
def test_lds_list_next_to_a_visited_set_in_hbm(pair, k, ef):
    """The production combination: on a large index every limit above 512 has its visited set in HBM."""
    pair.options(list_lds=2, visited_lds_log2_max=1, walkers=4)  # (a one-walker launch would keep its roomy set in LDS)
    _, _, shape = pair.check(k, ef, 1)
    assert shape[5] == 2 and shape[1] == 4
    pair.options(list_lds=1, visited_lds_log2_max=1)  # four walkers fit next to the largest list: the automatic rule takes it
    _, _, shape = pair.check(k, ef, 1, nq=600)
    assert shape[5] == 2 and shape[1] >= 1




def test_default_options(pair):
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = pair.gpu
    pair.options(list_lds=1, solo=1)  # every option at its default
    for k, ef in ((10, 1024), (10, 4096)):
        want, today = _expected_default_placement(pair.dim, min(max(k, ef), N), 600, n_cus)
        _, _, shape = pair.check(k, ef, want, nq=600)
        assert shape[1] == today  # the automatic rule never takes a walker away
    assert _expected_default_placement(pair.dim, 1024, 600, n_cus)[0] == 1  # (so that the LDS branch above is not vacuous)
    ck, cd, cc, _ = pair.oracle(600, 0, 1)
    got = g.search(pair.Q[0], 600)
    shape = g.last_search_shape()
    assert np.array_equal(got, ck[0][:cc[0]])
    assert shape[6] == 1 and shape[4] == 2 and shape[1] == 1, shape
    got = g.search_batch(pair.Q[:NQ], 10, 100)  # a register list reports 0
    assert g.last_search_shape()[4] == 0
    with pytest.raises(gc.pkg().VssError, match="out of range"):
        g.set_option("search.list_lds", 3)
    with pytest.raises(gc.pkg().VssError, match="out of range"):
        g.set_option("search.list_lds", -1)


def test_multi_batch_launch_over_the_lds_list(pair):
    import torch
    g, B, k, ef = pair.gpu, 64, 10, 1024
    pair.options(list_lds=2)
    ref = [g.search_batch(pair.Q[b * B:(b + 1) * B], k, ef) for b in range(3)]
    assert g.last_search_shape()[4] == 1
    dq = [torch.from_numpy(pair.Q[b * B:(b + 1) * B].copy()).cuda() for b in range(3)]
    ok = [torch.full((B, k), -7, dtype=torch.int64, device="cuda") for _ in range(3)]
    od = [torch.empty((B, k), dtype=torch.float32, device="cuda") for _ in range(3)]
    oc = [torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    g.search_multi_begin(1, [t.data_ptr() for t in dq], B, k, ef, [t.data_ptr() for t in ok], [t.data_ptr() for t in od],
                         [t.data_ptr() for t in oc])
    g.search_end(1)
    torch.cuda.synchronize()
    assert g.last_search_shape()[4] == 1
    for b in range(3):
        assert np.array_equal(ok[b].cpu().numpy(), ref[b][0]), b
        assert np.array_equal(od[b].cpu().numpy().view(np.uint32), ref[b][1].view(np.uint32)), b
        assert np.array_equal(oc[b].cpu().numpy(), ref[b][2]), b


@pytest.mark.parametrize("metric,dim", SHAPES)
def test_tombstones_and_predicates_over_the_lds_list(metric, dim):
    """Every 7th row removed, then a 2 % predicate: level_search_impl's TOMB form (candidate queue in HBM, list in LDS)."""
    cpu, gpu, Q = _build(metric, dim)
    Q = Q[:NQ]
    dead = np.arange(0, N, 7)
    gpu.remove(dead)
    for key in dead:
        cpu.remove(int(key))
    gpu.set_option("search.solo", 0)

    def same(g, c):
        assert np.array_equal(g[0], c[0]) and np.array_equal(g[1].view(np.uint32), c[1].view(np.uint32))
        assert np.array_equal(g[2], c[2])

    want = {(k, ef): cpu.search_many(Q, k, ef=ef) for k, ef in ((10, 1024), (600, 1024))}
    bm = golden_cases.filter_bitmap(N, 605, 0.02)
    want_f = cpu.search_many_filtered(Q, 600, 1024, bm, N)
    for mode, placement in ((2, 1), (0, 2)):
        gpu.set_option("search.list_lds", mode)
        for (k, ef), c in want.items():
            same(gpu.search_batch(Q, k, ef), c)
            assert np.array_equal(gpu.last_query_stats(len(Q)), c[3].astype(np.uint32))
            assert gpu.last_search_shape()[4] == placement
        g = gpu.search_batch_filtered(Q, 600, 1024, bm, N)
        same(g, want_f)
        assert gpu.last_search_shape()[4] == placement
        live = g[0][g[0] >= 0]
        assert not set(live.tolist()) & set(dead.tolist())
