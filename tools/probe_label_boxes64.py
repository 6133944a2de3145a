"""Boxes with 64-bit ends over resident label columns of either width (vss_search_batch_by_label_box64) against the road users
take today for a 64-bit column: building one bitmap per distinct predicate on the host from the two columns, uploading the table
and calling vss_search_batch_filtered_groups_auto (or the exact scan).  One index in one process, the calls in turn.
The benchmark's mixture, the reference's default index options (M 16, ef_construction 128), k 10.  Column 0 holds a tenant of 64
values, 32 bits wide; column 1 a TIMESTAMP, 64 bits wide: microseconds uniform over 10^6 values around 10^15, mapped by x ^ 2^63
(INTEGRATION.md §5).  A chunk of 204 queries, every one with its own (tenant, since) pair:
`items.tenant = q.tenant AND items.ts >= q.since`.  Modes auto and exact.  Five repetitions after a warm-up, median and spread
(max - min) of host-pointer wall time of
    (a) the by-box64 call
    (b) the bitmap call on a table built BEFOREHAND (the upload still inside)   — existing code, the same scan
    (c) the bitmap call INCLUDING building its table from the two columns in NumPy — what a caller pays today
  (c) / (a) is what the caller gains; (a) against (b) is printed whichever way it falls.  Answers and routes of (a) and (b) are
  compared.
Then the WALKERS, which those pairs never reach (every box holds at most 1/64 of the rows and is scanned): 204 boxes of every
tenant and `ts >= since` with 25-60 % of the rows behind `since`, mode graph, (a) against (b) vss_search_batch_filtered_groups on
a ready table.
Then the cost of the 64-bit form where 32 bits would do: both columns 32 bits wide, the same pairs (modes auto and exact) and
the same wide boxes (mode graph), the box64 call against vss_search_batch_by_label_box; the sign and size of the difference are
printed.
    python tools/probe_label_boxes64.py [rows [dim [metric [ef]]]]"""
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
M, M0, EFC, K, REPEATS, NQ, TENANTS, STAMPS = 16, 32, 128, 10, 5, 204, 64, 1_000_000
TOP, TOP64, EPOCH = 0xFFFFFFFF, np.uint64(0xFFFFFFFFFFFFFFFF), 10 ** 15
SIGN = np.uint64(1 << 63)
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
stamp32 = rng.integers(0, STAMPS, size=rows).astype(np.uint32)
stamp = (stamp32.astype(np.int64) + EPOCH).view(np.uint64) ^ SIGN  # TIMESTAMP microseconds -> unsigned, in order
t = time.perf_counter()
idx.set_label_column(0, 0, tenant)
idx.set_label_column64(1, 0, stamp)
print("a 32-bit and a 64-bit label column of %d rows took %.2f ms once" % (rows, (time.perf_counter() - t) * 1e3), flush=True)
pad = (-rows) % 64


def table_of(lo, hi, columns):
    """the bitmaps a caller of the bitmap calls builds from its columns: one per distinct predicate"""
    boxes = np.empty((len(lo), 2 * len(columns)), dtype=lo.dtype)
    boxes[:, 0::2], boxes[:, 1::2] = lo, hi
    distinct, group_of = np.unique(boxes, axis=0, return_inverse=True)
    tables = np.zeros((len(distinct), (rows + 63) // 64), dtype=np.uint64)
    for g, row in enumerate(distinct):
        mask = np.ones(rows, dtype=bool)
        for j, column in enumerate(columns):
            mask &= (column >= row[2 * j].astype(column.dtype)) & (column <= min(row[2 * j + 1], np.iinfo(column.dtype).max))
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


# ---- tenant = q.tenant AND ts >= q.since, every query its own pair; the tenant 32 bits wide, the timestamp 64
pairs = np.stack([rng.integers(0, TENANTS, NQ), rng.integers(0, STAMPS, NQ)], axis=1)
since = (pairs[:, 1].astype(np.int64) + EPOCH).view(np.uint64) ^ SIGN
lo = np.stack([pairs[:, 0].astype(np.uint64), since], axis=1)
hi = np.stack([pairs[:, 0].astype(np.uint64), np.full(NQ, TOP64, dtype=np.uint64)], axis=1)
tables, group_of = table_of(lo, hi, (tenant, stamp))
for mode in ("auto", "exact"):
    def with_table():
        tb, go = table_of(lo, hi, (tenant, stamp))
        return bitmap_call(mode, tb, go)

    (aw, bw, cw), (a_out, b_out, _) = in_turn((lambda: idx.search_batch_by_label_box64(Q, K, EF, [0, 1], lo, hi, mode),
                                               lambda: bitmap_call(mode, tables, group_of), with_table))
    what = "tenant u32 x ts u64, mode %s" % mode
    line(what + ": (a) by box64", aw), line(what + ": (b) bitmaps ready", bw), line(what + ": (c) bitmaps built + call", cw)
    bar = 3 * max(spread(aw), spread(bw))
    diff = float(np.median(aw) - np.median(bw))
    how = idx.last_filter_route() if mode == "auto" else [0, NQ]
    print("  %d distinct boxes; %d queries walked, %d scanned; answers and routes equal: %s\n"
          "  bytes to the device besides the queries: (a) %d, (b) %d\n"
          "  (a) - (b) = %.3f ms against a bar of %.3f ms (3 x the larger spread): %s; (a) / (b) = %.4f, (c) / (a) = %.2f"
          % (len(tables), how[0], how[1], same(a_out, b_out), lo.nbytes + hi.nbytes, tables.nbytes + group_of.nbytes, diff, bar,
             verdict(diff, bar, "the by-box64 call"), np.median(aw) / np.median(bw), np.median(cw) / np.median(aw)), flush=True)

# ---- the walkers: every tenant, ts >= since with 25-60 % of the rows behind it, mode graph
wide_since = rng.integers(int(0.40 * STAMPS), int(0.75 * STAMPS), NQ)
wlo = np.stack([np.zeros(NQ, dtype=np.uint64), (wide_since.astype(np.int64) + EPOCH).view(np.uint64) ^ SIGN], axis=1)
whi = np.stack([np.full(NQ, TENANTS - 1, dtype=np.uint64), np.full(NQ, TOP64, dtype=np.uint64)], axis=1)
wtables, wgroup_of = table_of(wlo, whi, (tenant, stamp))
(aw, bw), (a_out, b_out) = in_turn((lambda: idx.search_batch_by_label_box64(Q, K, EF, [0, 1], wlo, whi, "graph"),
                                    lambda: idx.search_batch_filtered_groups(Q, K, EF, wtables, rows, wgroup_of) + (np.zeros(NQ, np.uint8),)))
line("wide boxes, mode graph: (a) by box64", aw), line("wide boxes, mode graph: (b) bitmaps ready", bw)
bar = 3 * max(spread(aw), spread(bw))
diff = float(np.median(aw) - np.median(bw))
print("  %d distinct boxes, all walked; answers equal: %s; (a) - (b) = %+.3f ms (%+.2f %%) against a bar of %.3f ms: %s"
      % (len(wtables), same(a_out, b_out), diff, 100.0 * diff / np.median(bw), bar, verdict(diff, bar, "the by-box64 call")), flush=True)

# ---- both columns 32 bits wide, the same pairs: what the 64-bit form costs where the 32-bit box call would do
idx.clear_label_column(1)
idx.set_label_column(1, 0, stamp32)
lo32 = pairs.astype(np.uint32)
hi32 = np.stack([lo32[:, 0], np.full(NQ, TOP, dtype=np.uint32)], axis=1)
lo64, hi64 = lo32.astype(np.uint64), hi32.astype(np.uint64)
wlo32 = np.stack([np.zeros(NQ, dtype=np.uint32), wide_since.astype(np.uint32)], axis=1)
whi32 = np.stack([np.full(NQ, TENANTS - 1, dtype=np.uint32), np.full(NQ, TOP, dtype=np.uint32)], axis=1)
for mode in ("auto", "exact", "graph"):
    a_lo, a_hi, b_lo, b_hi = (wlo32.astype(np.uint64), whi32.astype(np.uint64), wlo32, whi32) if mode == "graph" else (lo64, hi64, lo32, hi32)
    (aw, bw), (a_out, b_out) = in_turn((lambda: idx.search_batch_by_label_box64(Q, K, EF, [0, 1], a_lo, a_hi, mode),
                                        lambda: idx.search_batch_by_label_box(Q, K, EF, [0, 1], b_lo, b_hi, mode)))
    what = "two u32 columns, %s, mode %s" % ("wide boxes" if mode == "graph" else "the pairs", mode)
    line(what + ": (a) by box64", aw), line(what + ": (b) by box", bw)
    bar = 3 * max(spread(aw), spread(bw))
    diff = float(np.median(aw) - np.median(bw))
    print("  answers and routes equal: %s; (a) - (b) = %+.3f ms (%+.2f %%) against a bar of %.3f ms: %s"
          % (same(a_out, b_out), diff, 100.0 * diff / np.median(bw), bar, verdict(diff, bar, "the by-box64 call")), flush=True)
