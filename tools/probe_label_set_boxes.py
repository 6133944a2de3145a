"""An IN-list on one resident label column inside a box of ranges (vss_search_batch_by_label_set_box) against the road users take
today: building one bitmap per distinct predicate on the host from the columns, uploading the table and calling
vss_search_batch_filtered_groups_auto (or the exact scan).  One index in one process, the calls in turn.
The benchmark's mixture, the reference's default index options (M 16, ef_construction 128), k 10.  Column 0 holds a group of 64
values, 32 bits wide; column 1 a TIMESTAMP, 64 bits wide: microseconds uniform over 10^6 values around 10^15, mapped by x ^ 2^63
(INTEGRATION.md §5).  A chunk of 204 queries, every one with its own (groups, since) predicate, 8 groups each:
`items.grp IN (the groups this user may see) AND items.ts >= q.since`.  Modes auto and exact.  Five repetitions after a warm-up,
median and spread (max - min) of host-pointer wall time of
    (a) the by-set-box call
    (b) the bitmap call on a table built BEFOREHAND (the upload still inside)   — existing code, the same scan
    (c) the bitmap call INCLUDING building its table from the two columns in NumPy — what a caller pays today
  (c) / (a) is what the caller gains; (a) against (b) is printed whichever way it falls.  Answers and routes of (a) and (b) are
  compared.
Then the WALKERS: 204 lists of 32 of the 64 groups and `ts >= since` with 25-60 % of the rows behind `since`, mode graph, (a)
against (b) vss_search_batch_filtered_groups on a ready table.
Then the cost of the 64-bit words where 32 bits would do: no range column, the same lists on the narrow column 0 (modes auto,
exact and — the wide lists — graph), the set-box call against vss_search_batch_by_label_set; the sign and size of the difference
are printed.
    python tools/probe_label_set_boxes.py [rows [dim [metric [ef]]]]"""
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
M, M0, EFC, K, REPEATS, NQ, GROUPS, STAMPS, LIST = 16, 32, 128, 10, 5, 204, 64, 1_000_000, 8
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
print("built %d x %d %s M %d efc %d in %.1f s; k %d ef %d" % (rows, dim, metric, M, EFC, time.perf_counter() - t0, K, EF), flush=True)
Q = np.ascontiguousarray(gen.rows(bench.QUERY_SEED, 0, NQ).cpu().numpy())
rng = np.random.default_rng(20261021)
grp = rng.integers(0, GROUPS, size=rows).astype(np.uint32)
stamp32 = rng.integers(0, STAMPS, size=rows).astype(np.uint32)
stamp = (stamp32.astype(np.int64) + EPOCH).view(np.uint64) ^ SIGN  # TIMESTAMP microseconds -> unsigned, in order
idx.set_label_column(0, 0, grp)
idx.set_label_column64(1, 0, stamp)
pad = (-rows) % 64


def table_of(sets, lo):
    """the bitmaps a caller of the bitmap calls builds from its columns: one per distinct predicate (lo None: the list alone)"""
    pred = sets if lo is None else np.concatenate([sets, lo], axis=1)
    distinct, group_of = np.unique(pred, axis=0, return_inverse=True)
    tables = np.zeros((len(distinct), (rows + 63) // 64), dtype=np.uint64)
    for g, row in enumerate(distinct):
        mask = np.isin(grp, row[:sets.shape[1]].astype(np.uint32))
        if lo is not None:
            mask &= stamp >= row[-1]
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
    print("%-56s wall ms %s  median %10.3f spread %8.3f" % (name, " ".join("%.2f" % v for v in wall), float(np.median(wall)),
                                                            max(wall) - min(wall)), flush=True)


def spread(w):
    return max(w) - min(w)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip((a[0], a[1].view(np.uint32), a[2], a[3]), (b[0], b[1].view(np.uint32), b[2], b[3])))


def bitmap_call(mode, tables, group_of):
    if mode == "auto":
        return idx.search_batch_filtered_groups_auto(Q, K, EF, tables, rows, group_of)
    if mode == "graph":
        return idx.search_batch_filtered_groups(Q, K, EF, tables, rows, group_of) + (np.zeros(NQ, np.uint8),)
    return idx.search_exact_batch_filtered_groups(Q, K, tables, rows, group_of) + (np.ones(NQ, np.uint8),)


def verdict(diff, bar, name):
    return "%s LOSES" % name if diff > bar else "%s is the faster" % name if diff < -bar else "no difference shown"


def lists(width):
    return np.stack([rng.choice(GROUPS, width, replace=False) for _ in range(NQ)]).astype(np.uint64)


def stamps(values):
    return ((values.astype(np.int64) + EPOCH).view(np.uint64) ^ SIGN).reshape(NQ, 1)


# ---- grp IN (8 groups) AND ts >= q.since, every query its own predicate
sets = lists(LIST)
lo = stamps(rng.integers(0, STAMPS, NQ))
hi = np.full((NQ, 1), TOP64, dtype=np.uint64)
tables, group_of = table_of(sets, lo)
for mode in ("auto", "exact"):
    def with_table():
        tb, go = table_of(sets, lo)
        return bitmap_call(mode, tb, go)

    (aw, bw, cw), (a_out, b_out, _) = in_turn((lambda: idx.search_batch_by_label_set_box(Q, K, EF, 0, sets, [1], lo, hi, mode),
                                               lambda: bitmap_call(mode, tables, group_of), with_table))
    what = "grp u32 IN (8) x ts u64, mode %s" % mode
    line(what + ": (a) by set box", aw), line(what + ": (b) bitmaps ready", bw), line(what + ": (c) bitmaps built + call", cw)
    bar = 3 * max(spread(aw), spread(bw))
    diff = float(np.median(aw) - np.median(bw))
    how = idx.last_filter_route() if mode == "auto" else [0, NQ]
    print("  %d distinct predicates; %d queries walked, %d scanned; answers and routes equal: %s\n"
          "  bytes to the device besides the queries: (a) %d, (b) %d\n"
          "  (a) - (b) = %.3f ms against a bar of %.3f ms (3 x the larger spread): %s; (a) / (b) = %.4f, (c) / (a) = %.2f"
          % (len(tables), how[0], how[1], same(a_out, b_out), sets.nbytes + lo.nbytes + hi.nbytes, tables.nbytes + group_of.nbytes, diff,
             bar, verdict(diff, bar, "the by-set-box call"), np.median(aw) / np.median(bw), np.median(cw) / np.median(aw)), flush=True)

# ---- the walkers: 32 of the 64 groups, ts >= since with 25-60 % of the rows behind it, mode graph
wsets = lists(32)
wlo = stamps(rng.integers(int(0.40 * STAMPS), int(0.75 * STAMPS), NQ))
wtables, wgroup_of = table_of(wsets, wlo)
(aw, bw), (a_out, b_out) = in_turn((lambda: idx.search_batch_by_label_set_box(Q, K, EF, 0, wsets, [1], wlo, hi, "graph"),
                                    lambda: bitmap_call("graph", wtables, wgroup_of)))
line("lists of 32, mode graph: (a) by set box", aw), line("lists of 32, mode graph: (b) bitmaps ready", bw)
bar = 3 * max(spread(aw), spread(bw))
diff = float(np.median(aw) - np.median(bw))
print("  %d distinct predicates, all walked; answers equal: %s; (a) - (b) = %+.3f ms (%+.2f %%) against a bar of %.3f ms: %s"
      % (len(wtables), same(a_out, b_out), diff, 100.0 * diff / np.median(bw), bar, verdict(diff, bar, "the by-set-box call")), flush=True)

# ---- no range column, the narrow column 0: what the 64-bit words cost where vss_search_batch_by_label_set would do
for mode in ("auto", "exact", "graph"):
    s64 = wsets if mode == "graph" else sets
    s32 = s64.astype(np.uint32)
    (aw, bw), (a_out, b_out) = in_turn((lambda: idx.search_batch_by_label_set_box(Q, K, EF, 0, s64, mode=mode),
                                        lambda: idx.search_batch_by_label_set(Q, K, EF, s32, mode)))
    what = "no range column, lists of %d, mode %s" % (s64.shape[1], mode)
    line(what + ": (a) by set box", aw), line(what + ": (b) by set", bw)
    bar = 3 * max(spread(aw), spread(bw))
    diff = float(np.median(aw) - np.median(bw))
    print("  answers and routes equal: %s; (a) - (b) = %+.3f ms (%+.2f %%) against a bar of %.3f ms: %s"
          % (same(a_out, b_out), diff, 100.0 * diff / np.median(bw), bar, verdict(diff, bar, "the by-set-box call")), flush=True)
