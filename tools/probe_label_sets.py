"""IN-list predicates on the resident label column (vss_search_batch_by_label_set) against the road users take today: building
one bitmap per distinct list on the host, uploading the table and calling vss_search_batch_filtered_groups_auto.  One index in
one process, the calls in turn.
The benchmark's mixture, the reference's default index options (M 16, ef_construction 128), k 10; labels uniform over 1000
groups.  A chunk of 204 queries, each with a list of `width` distinct groups of its own, at widths 1, 4, 16 and 32, in mode auto.
Five repetitions after a warm-up, median and spread (max - min) of host-pointer wall time of
    (a) the by-set call
    (b) the bitmap call INCLUDING building its table from the column in NumPy (one table look-up and one packbits per distinct
        list) and its upload, which the host-pointer call does itself          — what a caller pays today
    (c) the bitmap call on a table built BEFOREHAND (the upload still inside)   — for the split of (b) into host and device work
  and the bytes each of (a) and (b) sends to the device besides the queries.  Answers and routes of (a) and (b) are compared.
  (a) is held to (b): slower by more than 3 x the larger spread of the two is reported as a loss.
    python tools/probe_label_sets.py [rows [dim [metric [ef]]]]"""
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
M, M0, EFC, K, REPEATS, NQ, GROUPS = 16, 32, 128, 10, 5, 204, 1000
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
rng = np.random.default_rng(20261020)
labels = rng.integers(0, GROUPS, size=rows).astype(np.uint32)
t = time.perf_counter()
idx.set_labels(0, labels)
print("set_labels of %d rows took %.2f ms once" % (rows, (time.perf_counter() - t) * 1e3), flush=True)


def table_of(sets):
    """the bitmaps a caller of the bitmap calls builds from its column: one per distinct list"""
    lists, group_of = np.unique(sets, axis=0, return_inverse=True)
    words = (len(labels) + 63) // 64
    tables = np.zeros((len(lists), words), dtype=np.uint64)
    pad = (-len(labels)) % 64
    member = np.zeros(GROUPS, dtype=bool)
    for g, row in enumerate(lists):
        member[:] = False
        member[row[row < GROUPS]] = True
        mask = member[labels]
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


for width in (1, 4, 16, 32):
    sets = np.array([rng.choice(GROUPS, width, replace=False) for _ in range(NQ)], dtype=np.uint32)
    tables, group_of = table_of(sets)

    def with_table():
        tb, go = table_of(sets)
        return idx.search_batch_filtered_groups_auto(Q, K, EF, tb, rows, go)

    (aw, bw, cw), (a_out, b_out, _) = in_turn((lambda: idx.search_batch_by_label_set(Q, K, EF, sets, "auto"), with_table,
                                               lambda: idx.search_batch_filtered_groups_auto(Q, K, EF, tables, rows, group_of)))
    what = "width %2d" % width
    line(what + ": (a) by set", aw), line(what + ": (b) bitmaps built + call", bw), line(what + ": (c) bitmaps ready", cw)
    how = idx.last_filter_route()
    bar = 3 * max(spread(aw), spread(bw))
    diff = float(np.median(aw) - np.median(bw))
    print("  %d distinct lists of %d groups (%.1f %% of the rows each); %d queries walked, %d scanned; answers and routes equal: %s\n"
          "  bytes to the device besides the queries: (a) %d, (b) %d\n"
          "  (a) - (b) = %.3f ms against a bar of %.3f ms (3 x the larger spread): %s; (a) / (b) = %.4f, (a) / (c) = %.4f"
          % (len(tables), width, 100.0 * width / GROUPS, how[0], how[1], same(a_out, b_out), sets.nbytes, tables.nbytes + group_of.nbytes,
             diff, bar, "the by-set call LOSES" if diff > bar else "the by-set call is the faster" if diff < -bar else "no difference shown",
             np.median(aw) / np.median(bw), np.median(aw) / np.median(cw)), flush=True)
