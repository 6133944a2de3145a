"""Conjunctions of ranges over several resident label columns (vss_search_batch_by_label_box) against the road users take today:
building one bitmap per distinct predicate on the host from the two columns, uploading the table and calling
vss_search_batch_filtered_groups_auto (or the exact scan).  One index in one process, the calls in turn.
The benchmark's mixture, the reference's default index options (M 16, ef_construction 128), k 10.  Column 0 holds a tenant of 64
values, column 1 a timestamp uniform in [0, 10^6).  A chunk of 204 queries, every one with its own (tenant, since) pair:
`items.tenant = q.tenant AND items.ts >= q.since`.  Modes auto and exact.  Five repetitions after a warm-up, median and spread
(max - min) of host-pointer wall time of
    (a) the by-box call
    (b) the bitmap call on a table built BEFOREHAND (the upload still inside)   — the yardstick: existing code, the same scan
    (c) the bitmap call INCLUDING building its table from the two columns in NumPy — what a caller pays today
  (a) is held to (b): slower by more than 3 x the larger spread of the two is reported as a loss.  (c) / (a) is what the caller
  gains.  Answers and routes of (a) and (b) are compared.
Then the one-column degenerate chunk: the timestamps written into column 0, 204 windows of their own, the box call naming
column 0 alone against vss_search_batch_by_label_range on the same column; the sign and size of the difference are printed.
    python tools/probe_label_boxes.py [rows [dim [metric [ef]]]]"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import bench  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
dim = int(sys.argv[2]) if len(sys.argv) > 2 else 128
metric = sys.argv[3] if len(sys.argv) > 3 else "l2sq"
EF = int(sys.argv[4]) if len(sys.argv) > 4 else 64
M, M0, EFC, K, REPEATS, NQ, TENANTS, STAMPS, TOP = 16, 32, 128, 10, 5, 204, 64, 1_000_000, 0xFFFFFFFF
pkg = load_package()
dev = torch.device("cuda", 0)
gen = bench.Mixture(rows, dim, metric != "l2sq", dev)
idx = pkg.GpuIndex(dim, metric, M, M0, EFC)
idx.reserve(rows)
for c in range(0, rows, bench.CHUNK):
    m = min(bench.CHUNK, rows - c)
    x = gen.rows(bench.DATA_SEED, c // bench.CHUNK, m)
    ids = torch.arange(c, c + m, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    idx.stage_device(ids.data_ptr(), x.data_ptr(), m)
    del x, ids
t0 = time.perf_counter()
idx.build_finalize()
torch.cuda.synchronize()
print("library %s\nbuilt %d x %d %s M %d efc %d in %.1f s; k %d ef %d" % (pkg.LIB_PATH, rows, dim, metric, M, EFC,
                                                                          time.perf_counter() - t0, K, EF), flush=True)
Q = np.ascontiguousarray(gen.rows(bench.QUERY_SEED, 0, NQ).cpu().numpy())
rng = np.random.default_rng(20261021)
tenant = rng.integers(0, TENANTS, size=rows).astype(np.uint32)
stamp = rng.integers(0, STAMPS, size=rows).astype(np.uint32)
t = time.perf_counter()
idx.set_label_column(0, 0, tenant)
idx.set_label_column(1, 0, stamp)
print("two label columns of %d rows took %.2f ms once" % (rows, (time.perf_counter() - t) * 1e3), flush=True)
pad = (-rows) % 64


def table_of(lo, hi, columns):
    """the bitmaps a caller of the bitmap calls builds from its columns: one per distinct predicate"""
    boxes = np.empty((len(lo), 2 * len(columns)), dtype=np.uint32)
    boxes[:, 0::2], boxes[:, 1::2] = lo, hi
    distinct, group_of = np.unique(boxes, axis=0, return_inverse=True)
    tables = np.zeros((len(distinct), (rows + 63) // 64), dtype=np.uint64)
    for g, row in enumerate(distinct):
        mask = np.ones(rows, dtype=bool)
        for j, column in enumerate(columns):
            mask &= (column >= row[2 * j]) & (column <= row[2 * j + 1])
        tables[g] = np.packbits(np.concatenate([mask, np.zeros(pad, dtype=bool)]).astype(np.uint8), bitorder="little").view(np.uint64)
    return tables, np.asarray(group_of).reshape(-1).astype(np.uint32)


def in_turn(calls):
    wall, out = [[] for _ in calls], [None] * len(calls)
    for r in range(REPEATS + 1):
        for i, call in enumerate(calls):
            t = time.perf_counter()
            out[i] = call()
            if r:
                wall[i].append((time.perf_counter() - t) * 1e3)
    return wall, out


def line(name, wall):
    print("%-50s wall ms %s  median %10.3f spread %8.3f" % (name, " ".join("%.2f" % v for v in wall), float(np.median(wall)),
                                                            max(wall) - min(wall)), flush=True)


def spread(w):
    return max(w) - min(w)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip((a[0], a[1].view(np.uint32), a[2], a[3]), (b[0], b[1].view(np.uint32), b[2], b[3])))


def bitmap_call(mode, tables, group_of):
    if mode == "auto":
        return idx.search_batch_filtered_groups_auto(Q, K, EF, tables, rows, group_of)
    return idx.search_exact_batch_filtered_groups(Q, K, tables, rows, group_of) + (np.ones(NQ, np.uint8),)


def verdict(diff, bar, name):
    return "%s LOSES" % name if diff > bar else "%s is the faster" % name if diff < -bar else "no difference shown"


# ---- tenant = q.tenant AND ts >= q.since, every query its own pair
lo = np.stack([rng.integers(0, TENANTS, NQ), rng.integers(0, STAMPS, NQ)], axis=1).astype(np.uint32)
hi = np.stack([lo[:, 0], np.full(NQ, TOP, dtype=np.uint32)], axis=1).astype(np.uint32)
tables, group_of = table_of(lo, hi, (tenant, stamp))
for mode in ("auto", "exact"):
    def with_table():
        tb, go = table_of(lo, hi, (tenant, stamp))
        return bitmap_call(mode, tb, go)

    (aw, bw, cw), (a_out, b_out, _) = in_turn((lambda: idx.search_batch_by_label_box(Q, K, EF, [0, 1], lo, hi, mode),
                                               lambda: bitmap_call(mode, tables, group_of), with_table))
    what = "two columns, mode %s" % mode
    line(what + ": (a) by box", aw), line(what + ": (b) bitmaps ready", bw), line(what + ": (c) bitmaps built + call", cw)
    bar = 3 * max(spread(aw), spread(bw))
    diff = float(np.median(aw) - np.median(bw))
    how = idx.last_filter_route() if mode == "auto" else [0, NQ]
    print("  %d distinct boxes; %d queries walked, %d scanned; answers and routes equal: %s\n"
          "  bytes to the device besides the queries: (a) %d, (b) %d\n"
          "  (a) - (b) = %.3f ms against a bar of %.3f ms (3 x the larger spread): %s; (a) / (b) = %.4f, (c) / (a) = %.2f"
          % (len(tables), how[0], how[1], same(a_out, b_out), lo.nbytes + hi.nbytes, tables.nbytes + group_of.nbytes, diff, bar,
             verdict(diff, bar, "the by-box call"), np.median(aw) / np.median(bw), np.median(cw) / np.median(aw)), flush=True)

# ---- one column: the timestamps in column 0, the box call naming it alone against the range call
idx.clear_labels()
idx.set_labels(0, stamp)
lo1 = rng.integers(0, STAMPS, (NQ, 1)).astype(np.uint32)
hi1 = np.minimum(lo1.astype(np.int64) + rng.integers(0, STAMPS // 4, (NQ, 1)), TOP).astype(np.uint32)
for mode in ("auto", "exact"):
    (aw, bw), (a_out, b_out) = in_turn((lambda: idx.search_batch_by_label_box(Q, K, EF, [0], lo1, hi1, mode),
                                        lambda: idx.search_batch_by_label_range(Q, K, EF, lo1[:, 0], hi1[:, 0], mode)))
    what = "one column, mode %s" % mode
    line(what + ": (a) by box", aw), line(what + ": (b) by range", bw)
    bar = 3 * max(spread(aw), spread(bw))
    diff = float(np.median(aw) - np.median(bw))
    print("  answers and routes equal: %s; (a) - (b) = %+.3f ms (%+.2f %%) against a bar of %.3f ms: %s"
          % (same(a_out, b_out), diff, 100.0 * diff / np.median(bw), bar, verdict(diff, bar, "the by-box call")), flush=True)
