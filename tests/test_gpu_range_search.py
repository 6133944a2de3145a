"""-m gpu: the exact range search (vss_search_range_batch*).

Contract: query q matches every live row whose engine f32 distance d satisfies d <= radii[q]; offsets and total always, the
cells only when the total fits the capacity.  The reference is gpu_common.ExactReference's distances (orc_distance_wave over
every live pair on the CPU; it reads nothing from the index); per query the set of (row id, distance bits) is compared, sorted
by row id on both sides.  Radii come from the reference itself and mix inside a batch: below the nearest distance, the bits of
the 5th-nearest (boundary included), one f32 below them (boundary excluded), +inf, NaN.
"""
import functools

import numpy as np
import pytest

import gpu_common as gc

pytestmark = pytest.mark.gpu

NQ = 129


def unit(a):
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)


def build(dim, metric, X, keys):
    """A cheap graph (only the exact path is under test), a tenth of the rows removed; returns the index and the live mask."""
    gpu = gc.gpu_index(dim, metric, 8, 16, 16)
    gpu.reserve(len(X))
    gpu.set_build_params(32768, 4)
    gpu.add(keys, X)
    gone = np.arange(len(X)) % 10 == 3
    gpu.remove(keys[gone])
    return gpu, ~gone


def mixed_radii(ref, nq):
    d = ref.dist[:nq]
    with np.errstate(invalid="ignore"):
        kinds = [np.nextafter(d[:, 0], np.float32(-np.inf)), d[:, 4], np.nextafter(d[:, 4], np.float32(-np.inf)),
                 np.full(nq, np.inf, np.float32), np.full(nq, np.nan, np.float32)]
    which = (np.arange(nq) + 1) % 5  # (a batch of one query takes the boundary radius)
    return np.choose(which, kinds).astype(np.float32)


def expected(ref, radii):
    """offsets and, per query, (row ids, distances) sorted by row id"""
    cells = []
    for q, r in enumerate(radii):
        with np.errstate(invalid="ignore"):
            hit = ref.dist[q] <= r
        order = np.argsort(ref.keys[q][hit], kind="stable")
        cells.append((ref.keys[q][hit][order], ref.dist[q][hit][order]))
    offsets = np.concatenate([[0], np.cumsum([len(k) for k, _ in cells])]).astype(np.uint64)
    return offsets, cells


def assert_range_answer(got, want, what):
    (offsets, ids, d, total), (w_offsets, w_cells) = got, want
    assert np.array_equal(offsets, w_offsets) and total == int(w_offsets[-1]), (what, offsets[:8], w_offsets[:8], total)
    for q, (w_ids, w_d) in enumerate(w_cells):
        lo, hi = int(offsets[q]), int(offsets[q + 1])
        order = np.argsort(ids[lo:hi], kind="stable")
        assert np.array_equal(ids[lo:hi][order], w_ids), (what, q)
        assert np.array_equal(d[lo:hi][order].view(np.uint32), w_d.view(np.uint32)), (what, q)


@functools.lru_cache(maxsize=1)
def case(metric, dim, rows):
    """index, reference over the live rows (all of their distances, ascending per query) and queries: built once per shape"""
    rng = np.random.default_rng(100 * dim + rows)
    X = rng.standard_normal((rows, dim)).astype(np.float32)
    Q = rng.standard_normal((NQ, dim)).astype(np.float32)
    if metric != "l2sq":
        X, Q = unit(X), unit(Q)
    keys = 1_000_000 - np.arange(rows, dtype=np.int64)
    gpu, live = build(dim, metric, X, keys)
    ref = gc.ExactReference(metric, X[live], keys[live], None, Q, rows)
    return gpu, ref, Q


@pytest.mark.parametrize("nq", [1, NQ])
@pytest.mark.parametrize("rows", [130, gc.pkg().RANGE_ROW_CHUNK + 1])
@pytest.mark.parametrize("dim", [64, 100, 768])
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_range_search(metric, dim, rows, nq):
    gpu, ref, Q = case(metric, dim, rows)
    radii = mixed_radii(ref, nq)
    got = gpu.search_range_batch(Q[:nq], radii)
    stats = gpu.last_range()
    print("%s dim %d rows %d queries %d: %d candidates, %d matches" % (metric, dim, rows, nq, stats[0], stats[1]))
    assert_range_answer(got, expected(ref, radii), (metric, dim, rows, nq))
    assert stats[1] == got[3] and stats[0] >= stats[1] and stats[2] == 0 and stats[3] > 0
    assert gpu.memory_usage() >= stats[3]


@pytest.mark.parametrize("data", ["offset8192", "norm_2^41"])
def test_where_the_score_says_little(data):
    """l2sq.  offset8192: rows = c + N(0, 1), |c| = 8192 — E ~ 1.2e-5 (2 |c|)^2 ~ 3e3 against squared distances of ~2 dim, so
    every live row is a candidate and the metric alone decides.  norm_2^41: one row of that norm — no E, theta = +inf."""
    rng = np.random.default_rng(7)
    dim, rows, nq = 100, 300, 8
    c = unit(rng.standard_normal(dim)) * np.float32(8192 if data == "offset8192" else 0)
    X, Q = (c + rng.standard_normal((rows, dim))).astype(np.float32), (c + rng.standard_normal((nq, dim))).astype(np.float32)
    if data == "norm_2^41":
        X[17] = unit(X[17]) * np.float32(2.0 ** 41)
    keys = np.arange(rows, dtype=np.int64)
    gpu, live = build(dim, "l2sq", X, keys)
    ref = gc.ExactReference("l2sq", X[live], keys[live], None, Q, rows)
    radii = mixed_radii(ref, nq)
    assert_range_answer(gpu.search_range_batch(Q, radii), expected(ref, radii), data)
    stats = gpu.last_range()
    no_bound = nq if data == "norm_2^41" else 0
    proposing = nq if no_bound else int((~np.isnan(radii)).sum())  # (with a finite E a NaN radius gets theta = -inf)
    assert stats[0] == proposing * live.sum() and stats[2] == no_bound, stats


def test_capacity_and_device_form():
    import torch
    gpu, ref, Q = case("cosine", 100, 130)
    radii = mixed_radii(ref, NQ)
    want = expected(ref, radii)
    total = int(want[0][-1])
    # the count-only call: no cell pointers at all
    offsets, ids, d, got_total = gpu.search_range_batch(Q, radii, capacity=0)
    assert np.array_equal(offsets, want[0]) and got_total == total and len(ids) == 0
    # one cell short: VSS_OK, offsets and total as ever, no cell touched
    offsets, ids, d = np.zeros(NQ + 1, np.uint64), np.full(total, -7, np.int64), np.full(total, -7, np.float32)
    out_total = np.zeros(1, np.uint64)
    rc = gpu.lib.vss_search_range_batch(gpu.h, Q.ctypes.data, NQ, radii.ctypes.data, total - 1, offsets.ctypes.data, ids.ctypes.data,
                                        d.ctypes.data, out_total.ctypes.data)
    assert rc == 0 and np.array_equal(offsets, want[0]) and out_total[0] == total
    assert (ids == -7).all() and (d == -7).all()
    # the device form
    t_q, t_r = torch.from_numpy(Q).cuda(), torch.from_numpy(radii).cuda()
    t_off, t_total = torch.zeros(NQ + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    t_ids, t_d = torch.zeros(total, dtype=torch.int64, device="cuda"), torch.zeros(total, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu.search_range_batch_device(t_q.data_ptr(), NQ, t_r.data_ptr(), total, t_off.data_ptr(), t_ids.data_ptr(), t_d.data_ptr(),
                                  t_total.data_ptr())
    got = (t_off.cpu().numpy().astype(np.uint64), t_ids.cpu().numpy(), t_d.cpu().numpy(), int(t_total.item()))
    assert_range_answer(got, want, "device form")
