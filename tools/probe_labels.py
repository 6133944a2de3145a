"""Equality predicates on the resident label column (vss_search_batch_by_label, mode auto) against the routed bitmap call
(vss_search_batch_filtered_groups_auto) on the table the column derives, on one index in one process, in turn.
The benchmark's mixture, the reference's default index options (M 16, ef_construction 128), k 10.
  For 16 tenants of 1/16, 256 tenants of 1/256 and one tenant per query (as many tenants as queries, equal shares), 1024 and 204
  queries, each of a tenant drawn uniformly (one tenant per query: a permutation), five repetitions after a warm-up, median and
  spread (max - min) of host-pointer wall time of
    (a) the by-label call, mode auto
    (b) the bitmap call on a table built BEFOREHAND                      — the yardstick: existing code of the same tree
    (c) the bitmap call INCLUDING building its table from the column in NumPy  — what a caller pays today
  (a) is held to (b): slower by more than 3 x the larger spread of the two is a loss.  The count step alone — the listing's
  first pass, label form against bitmap form — is timed through the exact mode with k = 1 and ONE query per tenant, where the
  scoring is as small as the call allows; the device span of the whole exact call (vss_timing [0]) is printed beside it, NOT a
  span of the listing alone.
    python tools/probe_labels.py [rows [dim [metric [ef]]]]"""
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
M, M0, EFC, K, REPEATS = 16, 32, 128, 10, 5
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
Q = gen.rows(bench.QUERY_SEED, 0, 1024).cpu().numpy()
rng = np.random.default_rng(20261020)


def table_of(labels, want):
    """the bitmaps a caller of the bitmap call builds from its tenant column: one per distinct wanted value"""
    values, group_of = np.unique(want, return_inverse=True)
    words = (len(labels) + 63) // 64
    tables = np.zeros((len(values), words), dtype=np.uint64)
    pad = (-len(labels)) % 64
    for g, v in enumerate(values):
        mask = labels == v
        tables[g] = np.packbits(np.concatenate([mask, np.zeros(pad, dtype=bool)]).astype(np.uint8), bitorder="little").view(np.uint64)
    return tables, group_of.astype(np.uint32)


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


for tenants in (16, 256, 0):
    for nq in (1024, 204):
        n_tenants = tenants or nq
        labels = rng.integers(0, n_tenants, size=rows).astype(np.uint32)
        want = (rng.integers(0, n_tenants, size=nq) if tenants else rng.permutation(nq)).astype(np.uint32)
        t = time.perf_counter()
        idx.set_labels(0, labels)
        set_ms = (time.perf_counter() - t) * 1e3
        q = np.ascontiguousarray(Q[:nq])
        tables, group_of = table_of(labels, want)

        def with_table():
            tb, go = table_of(labels, want)
            return idx.search_batch_filtered_groups_auto(q, K, EF, tb, rows, go)

        (aw, bw, cw), (a_out, b_out, _) = in_turn((lambda: idx.search_batch_by_label(q, K, EF, want, "auto"),
                                                   lambda: idx.search_batch_filtered_groups_auto(q, K, EF, tables, rows, group_of),
                                                   with_table))
        how = idx.last_filter_route()
        what = ("%d tenants, %d queries" % (tenants, nq)) if tenants else ("one tenant per query, %d queries" % nq)
        line(what + ": (a) by label", aw), line(what + ": (b) bitmaps, table ready", bw), line(what + ": (c) bitmaps + table", cw)
        bar = 3 * max(spread(aw), spread(bw))
        print("  table of %d bitmaps: %.1f MB; set_labels of %d rows took %.2f ms once; %d queries walked, %d scanned; answers and routes "
              "equal: %s\n  (a) - (b) = %.3f ms against a bar of %.3f ms (3 x the larger spread): %s; (a) / (c) = %.3f"
              % (len(tables), tables.nbytes / 1e6, rows, set_ms, how[0], how[1], same(a_out, b_out), np.median(aw) - np.median(bw), bar,
                 "by label LOSES" if np.median(aw) - np.median(bw) > bar else "no loss shown", np.median(aw) / np.median(cw)), flush=True)
        # the count step: exact mode, k 1, one query per tenant in use
        values = np.unique(want)
        one_each = values.astype(np.uint32)
        q1 = np.ascontiguousarray(Q[:len(one_each)])
        g1 = np.arange(len(one_each), dtype=np.uint32)
        span = [[], []]

        def label_exact():
            out = idx.search_batch_by_label(q1, 1, EF, one_each, "exact")
            span[0].append(idx.timing()["search_kernel_ms"])
            return out

        def bitmap_exact():
            out = idx.search_exact_batch_filtered_groups(q1, 1, tables, rows, g1)
            span[1].append(idx.timing()["search_kernel_ms"])
            return out

        (lw, xw), (l_out, x_out) = in_turn((label_exact, bitmap_exact))
        line(what + ": exact k 1, %d values: by label" % len(values), lw), line(what + ": exact k 1, %d values: bitmaps" % len(values), xw)
        print("  device span of the whole exact call (count, lists, scores, select, rerank), median ms: by label %.3f, bitmaps %.3f; "
              "answers equal: %s" % (float(np.median(span[0][1:])), float(np.median(span[1][1:])),
                                     all(np.array_equal(x, y) for x, y in zip((l_out[0], l_out[2]), (x_out[0], x_out[2])))), flush=True)
