"""Range predicates on the resident label column (vss_search_batch_by_label_range) against the bitmap calls on the table the
column and the call's ranges derive, on one index in one process, in turn.
The benchmark's mixture, the reference's default index options (M 16, ef_construction 128), k 10; labels uniform in [0, 10^6).
  A chunk of 204 queries, each with a range of its own (distinct lower ends), in modes graph and auto.  Mode auto takes widths
  of 0.01 %, 1 % and 5-60 % of the labels in equal parts; mode graph, which walks whatever it is given and whose cost grows as
  the inverse of the admitted share (seconds per call below a share of 1/64), takes 25-60 % only, the
  shares that call is for.  Five repetitions after a warm-up, median and spread (max - min) of host-pointer wall time of
    (a) the by-range call
    (b) the bitmap call of the same mode on a table built BEFOREHAND                — existing code of the same tree
    (c) the bitmap call INCLUDING building its table from the column in NumPy     — what a caller pays today
  and then the equality-degenerate chunk, lo = hi = one of 204 tenants, labels uniform in [0, 204), in modes auto and exact:
    (d) the by-range call        (e) vss_search_batch_by_label        — what two cells per query and a listing loop over the
                                                                         groups cost relative to the label form
  (a) is held to (b), (d) to (e): slower by more than 3 x the larger spread of the two is reported as a loss.
    python tools/probe_label_ranges.py [rows [dim [metric [ef]]]]"""
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
dim = int(sys.argv[2]) if len(sys.argv) > 2 else 768
metric = sys.argv[3] if len(sys.argv) > 3 else "l2sq"
EF = int(sys.argv[4]) if len(sys.argv) > 4 else 64
M, M0, EFC, K, REPEATS, NQ = 16, 32, 128, 10, 5, 204
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


def table_of(labels, lo, hi):
    """the bitmaps a caller of the bitmap calls builds from its column: one per distinct (lo, hi)"""
    packed = (lo.astype(np.uint64) << np.uint64(32)) | hi.astype(np.uint64)
    pairs, group_of = np.unique(packed, return_inverse=True)
    words = (len(labels) + 63) // 64
    tables = np.zeros((len(pairs), words), dtype=np.uint64)
    pad = (-len(labels)) % 64
    for g, p in enumerate(pairs):
        mask = (labels >= np.uint32(p >> np.uint64(32))) & (labels <= np.uint32(p & np.uint64(0xFFFFFFFF))) & (labels != 0xFFFFFFFF)
        tables[g] = np.packbits(np.concatenate([mask, np.zeros(pad, dtype=bool)]).astype(np.uint8), bitorder="little").view(np.uint64)
    return tables, group_of.astype(np.uint32)


def bitmap_call(mode, tables, group_of):
    if mode == "graph":
        return idx.search_batch_filtered_groups(Q, K, EF, tables, rows, group_of) + (np.zeros(NQ, np.uint8),)
    return idx.search_batch_filtered_groups_auto(Q, K, EF, tables, rows, group_of)


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
    print("%-58s wall ms %s  median %10.3f spread %8.3f" % (name, " ".join("%.2f" % v for v in wall), float(np.median(wall)),
                                                            max(wall) - min(wall)), flush=True)


def spread(w):
    return max(w) - min(w)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip((a[0], a[1].view(np.uint32), a[2], a[3]), (b[0], b[1].view(np.uint32), b[2], b[3])))


def verdict(name, x, y):
    bar = 3 * max(spread(x), spread(y))
    diff = float(np.median(x) - np.median(y))
    return "%s = %.3f ms against a bar of %.3f ms (3 x the larger spread): %s" % (name, diff, bar, "the range call LOSES" if diff > bar
                                                                                  else "no loss shown")


# ---- 204 distinct ranges over labels uniform in [0, 10^6)
labels = rng.integers(0, 1_000_000, size=rows).astype(np.uint32)
WIDTHS = {"auto": np.concatenate([np.full(68, 100), np.full(68, 10_000), rng.integers(50_000, 600_000, 68)])[rng.permutation(NQ)],
          "graph": rng.integers(250_000, 600_000, NQ)}
t = time.perf_counter()
idx.set_labels(0, labels)
print("set_labels of %d rows took %.2f ms once" % (rows, (time.perf_counter() - t) * 1e3), flush=True)
for mode in ("graph", "auto"):
    lo = rng.choice(400_000, NQ, replace=False).astype(np.uint32)
    hi = (lo + WIDTHS[mode]).astype(np.uint32)
    t = time.perf_counter()
    tables, group_of = table_of(labels, lo, hi)
    print("mode %s: table of %d bitmaps: %.1f MB, built in NumPy in %.1f ms" % (mode, len(tables), tables.nbytes / 1e6,
                                                                              (time.perf_counter() - t) * 1e3), flush=True)

    def with_table():
        tb, go = table_of(labels, lo, hi)
        return bitmap_call(mode, tb, go)

    (aw, bw, cw), (a_out, b_out, _) = in_turn((lambda: idx.search_batch_by_label_range(Q, K, EF, lo, hi, mode),
                                               lambda: bitmap_call(mode, tables, group_of), with_table))
    what = "204 distinct ranges, mode %s" % mode
    line(what + ": (a) by range", aw), line(what + ": (b) bitmaps, table ready", bw), line(what + ": (c) bitmaps + table", cw)
    how = idx.last_filter_route() if mode == "auto" else [NQ, 0]
    print("  %d queries walked, %d scanned; answers and routes equal: %s\n  %s; (a) / (c) = %.4f"
          % (how[0], how[1], same(a_out, b_out), verdict("(a) - (b)", aw, bw), np.median(aw) / np.median(cw)), flush=True)

# ---- the equality-degenerate chunk: one tenant per query of 204 equal tenants
labels = rng.integers(0, NQ, size=rows).astype(np.uint32)
want = rng.permutation(NQ).astype(np.uint32)
idx.set_labels(0, labels)
for mode in ("auto", "exact"):  # (a walk under a share of 1/204 takes seconds per call in either form: not timed)
    (dw, ew), (d_out, e_out) = in_turn((lambda: idx.search_batch_by_label_range(Q, K, EF, want, want, mode),
                                        lambda: idx.search_batch_by_label(Q, K, EF, want, mode)))
    what = "lo = hi = one of 204 tenants, mode %s" % mode
    line(what + ": (d) by range", dw), line(what + ": (e) by label", ew)
    print("  answers and routes equal: %s\n  %s" % (same(d_out, e_out), verdict("(d) - (e)", dw, ew)), flush=True)
