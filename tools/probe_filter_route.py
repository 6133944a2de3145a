"""Routed per-query predicates (vss_search_batch_filtered_groups_auto) against the two calls it chooses between
(vss_search_batch_filtered_groups, vss_search_exact_batch_filtered_groups), all on one index in one process, in turn.
The benchmark's mixture, the reference's default index options (M 16, ef_construction 128), k 10.
  mix       one table of 24 tenants that partition the rows — shares 1/2, 1/4, 2 x 1/16, 4 x 1/64, 16 x 1/256 —, 1024 and 204
            queries, each of a tenant drawn uniformly: graph, exact, auto, five repetitions after a warm-up; median and spread
            (max - min) of host-pointer wall time.  Auto is held to the smaller median of the other two: slower by more than
            3 x the larger spread of the two is a loss.
  single    uniform tenants of one share (1/2 ... 1/256) through the auto call and through the call it routes to: the plumbing alone
  floor     n = 1 ... 256 queries of ONE tenant of share 1/1, 1/2, 1/3 through the graph and the exact call: how many queries a walk
            needs before its launch beats scanning the tenant for them — the smallest graph sub-batch worth launching
  sweep     uniform tenants of shares 1/2, 1/3, 1/4, 1/6, 1/8, 1/16 through the graph and the exact call: between which shares the
            faster one changes, and whether the rule's crossover len* = sqrt(C * limit / 64 * L) lies there
    python tools/probe_filter_route.py [rows [dim [metric [ef [legs: mix,single,floor,sweep]]]]]"""
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
legs = (sys.argv[5] if len(sys.argv) > 5 else "mix,single,sweep").split(",")
M, M0, EFC, K, REPEATS, C = 16, 32, 128, 10, 5, 62_500
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
limit = max(K, EF)
crossover = (C * limit * rows / 64) ** 0.5
print("library %s\nbuilt %d x %d %s M %d efc %d in %.1f s; k %d ef %d; the rule's crossover len* = %.0f rows (share 1/%.2f)"
      % (pkg.LIB_PATH, rows, dim, metric, M, EFC, time.perf_counter() - t0, K, EF, crossover, rows / crossover), flush=True)
Q = gen.rows(bench.QUERY_SEED, 0, 1024).cpu().numpy()
rng = np.random.default_rng(20261020)


def bitmap_of(mask):
    pad = (-len(mask)) % 64
    return np.packbits(np.concatenate([mask, np.zeros(pad, dtype=bool)]).astype(np.uint8), bitorder="little").view(np.uint64)


def in_turn(calls):
    """REPEATS of every call after one warm-up each, a / b / c / a / b / c ...: ([wall ms], last result) per call"""
    wall, out = [[] for _ in calls], [None] * len(calls)
    for r in range(REPEATS + 1):
        for i, call in enumerate(calls):
            t = time.perf_counter()
            out[i] = call()
            if r:
                wall[i].append((time.perf_counter() - t) * 1e3)
    return wall, out


def line(name, wall):
    print("%-44s wall ms %s  median %10.3f spread %8.3f" % (name, " ".join("%.2f" % v for v in wall), float(np.median(wall)),
                                                            max(wall) - min(wall)), flush=True)


def spread(w):
    return max(w) - min(w)


def same(a, b, rows_):
    return all(np.array_equal(x[rows_], y[rows_]) for x, y in zip((a[0], a[1].view(np.uint32), a[2]), (b[0], b[1].view(np.uint32), b[2])))


def uniform_tables(n, nq):
    tenant = rng.integers(0, n, size=rows)
    groups = min(n, nq)
    return np.stack([bitmap_of(tenant == g) for g in range(groups)]), (np.arange(nq) % groups).astype(np.uint32), groups


if "mix" in legs:
    shares = [2, 4, 16, 16, 64, 64, 64, 64] + [256] * 16
    edges = np.cumsum([0.0] + [1.0 / s for s in shares])
    assert abs(edges[-1] - 1.0) < 1e-12
    tenant = np.searchsorted(edges, rng.random(rows), side="right") - 1
    tables = np.stack([bitmap_of(tenant == g) for g in range(len(shares))])
    for nq in (1024, 204):
        group_of = rng.integers(0, len(shares), size=nq).astype(np.uint32)
        q = np.ascontiguousarray(Q[:nq])
        (gw, xw, aw), (g_out, x_out, a_out) = in_turn((lambda: idx.search_batch_filtered_groups(q, K, EF, tables, rows, group_of),
                                                       lambda: idx.search_exact_batch_filtered_groups(q, K, tables, rows, group_of),
                                                       lambda: idx.search_batch_filtered_groups_auto(q, K, EF, tables, rows, group_of)))
        how, listed = idx.last_filter_route(), idx.last_exact_filtered()
        route = a_out[3]
        what = "mix of 24 tenants, %d queries" % nq
        line(what + ": graph", gw), line(what + ": exact", xw), line(what + ": auto", aw)
        best, name = min((float(np.median(gw)), "graph"), (float(np.median(xw)), "exact"))
        bar = 3 * max(spread(gw if name == "graph" else xw), spread(aw))
        print("  auto: %d queries walked, %d scanned (%d / %d groups), %d rows listed; answers equal to the call routed to: %s\n"
              "  auto / min(graph, exact) = %.3f (the smaller is %s); auto - min = %.3f ms against a bar of %.3f ms (3 x the larger "
              "spread of the two): %s\n  graph filled k %d of %d, auto %d of %d"
              % (how[0], how[1], how[2], how[3], listed[0], same(a_out, x_out, route == 1) and same(a_out, g_out, route == 0),
                 np.median(aw) / best, name, np.median(aw) - best, bar, "auto LOSES" if np.median(aw) - best > bar else "auto holds",
                 int((g_out[2] == K).sum()), nq, int((a_out[2] == K).sum()), nq), flush=True)

if "single" in legs:
    for n in (2, 4, 16, 64, 256):
        for nq in (1024, 204):
            tables, group_of, groups = uniform_tables(n, nq)
            q = np.ascontiguousarray(Q[:nq])
            route = idx.search_batch_filtered_groups_auto(q, K, EF, tables, rows, group_of)[3]
            if len(set(route)) != 1:  # tenants of about len* rows: some above the boundary, some below
                print("share 1/%d, %d queries: %d walked, %d scanned — the tenants straddle the boundary; no single call to hold auto to"
                      % (n, nq, (route == 0).sum(), (route == 1).sum()), flush=True)
                continue
            if route[0]:
                target, other = "exact", lambda: idx.search_exact_batch_filtered_groups(q, K, tables, rows, group_of)
            else:
                target, other = "graph", lambda: idx.search_batch_filtered_groups(q, K, EF, tables, rows, group_of)
            (ow, aw), (o_out, a_out) = in_turn((other, lambda: idx.search_batch_filtered_groups_auto(q, K, EF, tables, rows, group_of)))
            what = "share 1/%d, %d queries" % (n, nq)
            line(what + ": " + target, ow), line(what + ": auto", aw)
            bar = 3 * max(spread(ow), spread(aw))
            print("  auto / %s = %.3f; auto - %s = %.3f ms against a bar of %.3f ms: %s; identical answers %s"
                  % (target, np.median(aw) / np.median(ow), target, np.median(aw) - np.median(ow), bar,
                     "auto is SLOWER" if np.median(aw) - np.median(ow) > bar else "no loss shown",
                     same(a_out, o_out, np.ones(nq, dtype=bool))), flush=True)

if "floor" in legs:
    for n in (1, 2, 3):
        tenant = rng.integers(0, n, size=rows)
        tables = np.stack([bitmap_of(tenant == 0)])
        length = int((tenant == 0).sum())
        for nq in (1, 8, 16, 32, 64, 128, 256):
            q = np.ascontiguousarray(Q[:nq])
            group_of = np.zeros(nq, dtype=np.uint32)
            (gw, xw), _ = in_turn((lambda: idx.search_batch_filtered_groups(q, K, EF, tables, rows, group_of),
                                   lambda: idx.search_exact_batch_filtered_groups(q, K, tables, rows, group_of)))
            print("floor ef %d, one tenant of %d rows, %3d queries (%.2e distances to scan): graph median %7.3f spread %6.3f | exact "
                  "median %7.3f spread %6.3f | %s" % (EF, length, nq, float(nq) * length, np.median(gw), spread(gw), np.median(xw),
                                                      spread(xw), "graph" if np.median(gw) < np.median(xw) else "exact"), flush=True)

if "sweep" in legs:
    for nq in (1024, 204):
        faster = []
        for n in (2, 3, 4, 6, 8, 16):
            tables, group_of, groups = uniform_tables(n, nq)
            q = np.ascontiguousarray(Q[:nq])
            (gw, xw), _ = in_turn((lambda: idx.search_batch_filtered_groups(q, K, EF, tables, rows, group_of),
                                   lambda: idx.search_exact_batch_filtered_groups(q, K, tables, rows, group_of)))
            rule = "exact" if (rows // n) ** 2 * 64 <= C * limit * rows else "graph"
            faster.append((n, "graph" if np.median(gw) < np.median(xw) else "exact", rule))
            print("sweep ef %d, share 1/%d, %d queries: graph median %9.3f spread %7.3f | exact median %9.3f spread %7.3f | graph / exact "
                  "%.2f | the rule says %s" % (EF, n, nq, np.median(gw), spread(gw), np.median(xw), spread(xw),
                                               np.median(gw) / np.median(xw), rule), flush=True)
        print("  ef %d, %d queries: faster call by share %s; the rule's crossover is share 1/%.2f"
              % (EF, nq, ", ".join("1/%d %s (rule %s)" % f for f in faster), rows / crossover), flush=True)
