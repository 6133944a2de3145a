"""-m gpu: the exact range search under per-query label boxes (vss_search_range_batch_by_label_box64*): query q
matches the live rows that its box admits (the rule of vss_search_batch_by_label_box64, applied here in numpy on the label
arrays) and whose engine f32 distance d satisfies d <= radii[q].  The reference is gpu_common.ExactReference over the live rows
(it reads nothing from the index); per query the set of (row id, distance bits) is compared.  Row ids are 0 .. rows - 1."""
import functools
import types

import numpy as np
import pytest

import gpu_common as gc
from test_gpu_range_search import NQ, assert_range_answer, build, mixed_radii, unit

pytestmark = pytest.mark.gpu

CHUNK = gc.pkg().RANGE_ROW_CHUNK
NULL64, ABSENT = np.uint64(0xFFFFFFFFFFFFFFFF), 77  # the NULL cell; a tenant no row has


def admitted_mask(labels, columns, lo, hi):
    """n_queries x rows: the box rule — every named cell is not NULL and within [lo, hi], both ends inclusive, unsigned"""
    ok = np.ones((len(lo), len(labels[columns[0]])), dtype=bool)
    for j, c in enumerate(columns):
        cell = labels[c].astype(np.uint64)
        null = cell == (NULL64 if labels[c].dtype == np.uint64 else np.uint64(0xFFFFFFFF))
        ok &= ~null & (cell >= lo[:, j:j + 1]) & (cell <= hi[:, j:j + 1])
    return ok


def reference(ref, ok):
    """per query: (row ids, distances) of the admitted live rows, nearest first — ref is sorted so, and its keys are row ids"""
    return [(ref.keys[q][ok[q, ref.keys[q]]], ref.dist[q][ok[q, ref.keys[q]]]) for q in range(len(ok))]


def radii_and_answer(near):
    """mixed_radii on each query's ADMITTED distances (5th nearest; +inf where fewer than 5 are admitted), and the answer"""
    d5 = np.full((len(near), 5), np.inf, np.float32)
    for q, (_, d) in enumerate(near):
        d5[q, :min(5, len(d))] = d[:5]
    radii = mixed_radii(types.SimpleNamespace(dist=d5), len(near))
    radii[[len(d) < 5 for _, d in near]] = np.inf
    cells = []
    for (ids, d), r in zip(near, radii):
        with np.errstate(invalid="ignore"):
            hit = d <= r
        order = np.argsort(ids[hit], kind="stable")
        cells.append((ids[hit][order], d[hit][order]))
    offsets = np.concatenate([[0], np.cumsum([len(k) for k, _ in cells])]).astype(np.uint64)
    return radii, (offsets, cells)


@functools.lru_cache(maxsize=1)
def case(metric, dim, rows):
    """Column 0 (32 bits) is the tenant: among the LIVE rows tenant 1 owns 1, tenant 2 owns 31, tenant 3 owns 8 and tenant 0 the
    rest.  Column 1 (64 bits) is a ts above 2^32, every 7th cell NULL.  Query groups (spread over the batch, not contiguous):
    1 query on tenant 1, 32 on `tenant = 0 AND ts >= s` (the 32-query tile on a long list), 33 on tenant 0 (the 128-query tile),
    and the remaining 63 over tenant 2, tenant 3 with a ts interval, an empty box (lo > hi) and an absent tenant."""
    rng = np.random.default_rng(100 * dim + rows)
    X = rng.standard_normal((rows, dim)).astype(np.float32)
    Q = rng.standard_normal((NQ, dim)).astype(np.float32)
    if metric != "l2sq":
        X, Q = unit(X), unit(Q)
    keys = np.arange(rows, dtype=np.int64)
    gpu, live = build(dim, metric, X, keys)
    tenant = np.zeros(rows, np.uint32)
    tenant[rng.permutation(keys[live])[:40]] = np.repeat([1, 2, 3], [1, 31, 8])
    ts = (keys.astype(np.uint64) << np.uint64(33)) + np.uint64(5)
    ts[::7] = NULL64
    gpu.set_label_column(0, 0, tenant)
    gpu.set_label_column64(1, 0, ts)
    kind = rng.permutation(np.repeat(np.arange(7), [1, 32, 33, 20, 20, 10, 13]))
    s = ts[rows // 2]
    t_of = np.array([1, 0, 0, 2, 3, 0, ABSENT], np.uint64)[kind]
    lo = np.stack([t_of, np.where(kind == 1, s, np.uint64(0))], axis=1)
    hi = np.stack([t_of, np.where(kind == 4, s, NULL64).astype(np.uint64)], axis=1)
    lo[kind == 5, 1], hi[kind == 5, 1] = 9, 8
    ref = gc.ExactReference(metric, X[live], keys[live], None, Q, rows)
    near = reference(ref, admitted_mask([tenant, ts], [0, 1], lo, hi))
    return gpu, Q, lo, hi, near


SHAPES = [(m, d, r) for m in ("l2sq", "cosine", "ip") for d in (64, 100, 768) for r in (130, CHUNK + 1)]
# (with a tenth of CHUNK + 1 rows removed no list reaches a chunk: one more size, at which tenant 0's live rows with a ts are more)
SHAPES += [(m, 100, CHUNK + 3000) for m in ("l2sq", "cosine", "ip")]


@pytest.mark.parametrize("metric,dim,rows", SHAPES)
def test_range_search_by_label_box(metric, dim, rows):
    gpu, Q, lo, hi, near = case(metric, dim, rows)
    radii, want = radii_and_answer(near)
    got = gpu.search_range_batch_by_label_box64(Q, radii, [0, 1], lo, hi)
    stats, fstats = gpu.last_range(), gpu.last_range_filtered()
    print("%s dim %d rows %d: range %s filtered %s" % (metric, dim, rows, stats, fstats))
    assert_range_answer(got, want, (metric, dim, rows))
    assert stats[1] == got[3] and stats[0] >= stats[1] and stats[2] == 0
    assert fstats[1] == sum(len(ids) for ids, _ in near) and fstats[0] > 0 and fstats[3] > 0  # only admitted rows were scored
    assert fstats[2] >= (3 if rows > CHUNK + 1 else 2)  # both shapes, and a second run of list positions at the largest size
    assert gpu.memory_usage() >= stats[3]


def test_where_the_score_says_little():
    """l2sq, rows = c + N(0, 1) with |c| = 8192 (test_gpu_range_search's offset8192): E dwarfs the distances, so every listed
    pair of a query whose radius is not NaN is proposed and the metric alone decides."""
    rng = np.random.default_rng(7)
    dim, rows, nq = 100, 300, 8
    c = unit(rng.standard_normal(dim)) * np.float32(8192)
    X, Q = (c + rng.standard_normal((rows, dim))).astype(np.float32), (c + rng.standard_normal((nq, dim))).astype(np.float32)
    keys = np.arange(rows, dtype=np.int64)
    gpu, live = build(dim, "l2sq", X, keys)
    tenant = (keys % 3).astype(np.uint32)
    gpu.set_label_column(0, 0, tenant)
    lo = hi = (np.arange(nq, dtype=np.uint64) % 3)[:, None]
    near = reference(gc.ExactReference("l2sq", X[live], keys[live], None, Q, rows), admitted_mask([tenant], [0], lo, hi))
    radii, want = radii_and_answer(near)
    assert_range_answer(gpu.search_range_batch_by_label_box64(Q, radii, [0], lo, hi), want, "offset8192")
    proposing = sum(len(ids) for (ids, _), r in zip(near, radii) if not np.isnan(r))
    assert gpu.last_range()[0] == proposing and gpu.last_range()[2] == 0, gpu.last_range()
    assert gpu.last_range_filtered()[1] == sum(len(ids) for ids, _ in near)


def raw_call(gpu, Q, radii, columns, n_columns, lo, hi, capacity, offsets, ids, d, total):
    ptr = (lambda a: None if a is None else a.ctypes.data)  # (the host form through the C ABI itself; None is a NULL pointer)
    columns = np.asarray(columns, np.uint32)
    return gpu.lib.vss_search_range_batch_by_label_box64(gpu.h, ptr(Q), len(Q), ptr(radii), columns.ctypes.data, n_columns, ptr(lo),
                                                         ptr(hi), capacity, ptr(offsets), ptr(ids), ptr(d), ptr(total))


def test_capacity_and_device_form():
    import torch
    gpu, Q, lo, hi, near = case("cosine", 100, 130)
    radii, want = radii_and_answer(near)
    total = int(want[0][-1])
    offsets, out_total = np.zeros(NQ + 1, np.uint64), np.zeros(1, np.uint64)  # the count-only call: no cell pointers at all
    assert raw_call(gpu, Q, radii, [0, 1], 2, lo, hi, 0, offsets, None, None, out_total) == 0
    assert np.array_equal(offsets, want[0]) and out_total[0] == total
    # one cell short: VSS_OK, offsets and total as ever, no cell touched
    offsets, ids, d = np.zeros(NQ + 1, np.uint64), np.full(total, -7, np.int64), np.full(total, -7, np.float32)
    assert raw_call(gpu, Q, radii, [0, 1], 2, lo, hi, total - 1, offsets, ids, d, out_total) == 0
    assert np.array_equal(offsets, want[0]) and out_total[0] == total and (ids == -7).all() and (d == -7).all()
    # the device form
    t_q, t_r = torch.from_numpy(Q).cuda(), torch.from_numpy(radii).cuda()
    t_lo, t_hi = torch.from_numpy(lo.view(np.int64)).cuda(), torch.from_numpy(hi.view(np.int64)).cuda()
    t_off, t_total = torch.zeros(NQ + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    t_ids, t_d = torch.zeros(total, dtype=torch.int64, device="cuda"), torch.zeros(total, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu.search_range_batch_by_label_box64_device(t_q.data_ptr(), NQ, t_r.data_ptr(), [0, 1], t_lo.data_ptr(), t_hi.data_ptr(), total,
                                                 t_off.data_ptr(), t_ids.data_ptr(), t_d.data_ptr(), t_total.data_ptr())
    got = (t_off.cpu().numpy().astype(np.uint64), t_ids.cpu().numpy(), t_d.cpu().numpy(), int(t_total.item()))
    assert_range_answer(got, want, "device form")


@pytest.mark.parametrize("what,columns,n_columns,null_radii", [
    ("unset column", [0, 2], 2, False), ("repeated column", [0, 0], 2, False), ("no column", [0, 1], 0, False),
    ("five columns", [0, 1, 2, 3, 0], 5, False), ("null radii", [0, 1], 2, True)])
def test_errors_write_nothing(what, columns, n_columns, null_radii):
    gpu, Q, lo, hi, near = case("cosine", 100, 130)
    radii = None if null_radii else np.ones(NQ, np.float32)
    lo_w, hi_w = np.zeros((NQ, max(n_columns, 1)), np.uint64), np.full((NQ, max(n_columns, 1)), NULL64)
    offsets, ids, d, total = np.full(NQ + 1, 7, np.uint64), np.full(64, -7, np.int64), np.full(64, -7, np.float32), np.full(1, 7, np.uint64)
    assert raw_call(gpu, Q, radii, columns, n_columns, lo_w, hi_w, 64, offsets, ids, d, total) == 1, what  # VSS_ERROR
    assert (offsets == 7).all() and (ids == -7).all() and (d == -7).all() and total[0] == 7, what
