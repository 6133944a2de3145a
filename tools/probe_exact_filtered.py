"""Exact top-k under per-query predicates (vss_search_exact_batch_filtered_groups) against the grouped graph call
(vss_search_batch_filtered_groups), both on one index in one process, alternating.
The benchmark's mixture, the reference's default index options (M 16, ef_construction 128), k 10, ef 64; query q belongs to tenant
q mod n, tenant t admits the rows r with tenant[r] == t (a random assignment), so a tenant's share of the rows is 1 / n.
  tenants   shares 1/2, 1/4, 1/16, 1/64, 1/256; 1024 queries and a 204-query chunk: one graph call, one exact call, five repetitions
            after a warm-up; median and spread (max - min) of host-pointer wall time and of kernel time (vss_timing: for the exact
            call the span of its stream work, listing and the copy-back of the list lengths included), vss_last_exact_filtered,
            and the graph call's recall@10 and filled-k share against the exact answers
  ones      an all-ones bitmap against vss_search_exact_batch (the MFMA path): what a dense predicate leaves on the table
    python tools/probe_exact_filtered.py [rows [dim [metric [shares, comma separated [legs: tenants,ones]]]]]"""
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
shares = [int(s) for s in (sys.argv[4] if len(sys.argv) > 4 else "2,4,16,64,256").split(",")]
legs = (sys.argv[5] if len(sys.argv) > 5 else "tenants,ones").split(",")
M, M0, EFC, K, EF, REPEATS = 16, 32, 128, 10, 64, 5
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
print("library %s\nbuilt %d x %d %s M %d efc %d in %.1f s" % (pkg.LIB_PATH, rows, dim, metric, M, EFC, time.perf_counter() - t0),
      flush=True)
Q = gen.rows(bench.QUERY_SEED, 0, 1024).cpu().numpy()
rng = np.random.default_rng(20261019)


def bitmap_of(mask):
    pad = (-len(mask)) % 64
    return np.packbits(np.concatenate([mask, np.zeros(pad, dtype=bool)]).astype(np.uint8), bitorder="little").view(np.uint64)


def timed(call):
    """(wall ms, kernel ms, result) of one blocking host-pointer call"""
    t = time.perf_counter()
    out = call()
    return (time.perf_counter() - t) * 1e3, idx.timing()["search_kernel_ms"], out


def line(name, wall, kern):
    print("%-46s wall ms %s  median %8.3f spread %7.3f" % (name, " ".join("%.2f" % v for v in wall), float(np.median(wall)),
                                                             max(wall) - min(wall))
          + (" | kernel ms median %8.3f spread %7.3f" % (float(np.median(kern)), max(kern) - min(kern)) if kern else ""), flush=True)


def alternate(a, b):
    """REPEATS of a and b after one warm-up each, a / b / a / b ...: ([wall], [kernel], last result) per side"""
    wall, kern, out = ([], []), ([], []), [None, None]
    for r in range(REPEATS + 1):
        for i, call in enumerate((a, b)):
            w, k_ms, out[i] = timed(call)
            if r:
                wall[i].append(w), kern[i].append(k_ms)
    return (wall[0], kern[0], out[0]), (wall[1], kern[1], out[1])


if "tenants" in legs:
    for n in shares:
        tenant = rng.integers(0, n, size=rows)
        for nq in (1024, 204):
            groups = min(n, nq)  # (more tenants than queries: the table holds the tenants the chunk names)
            tables = np.stack([bitmap_of(tenant == g) for g in range(groups)])
            group_of = (np.arange(nq) % groups).astype(np.uint32)
            q = np.ascontiguousarray(Q[:nq])
            reruns = []

            def graph():
                out = idx.search_batch_filtered_groups(q, K, EF, tables, rows, group_of)
                reruns.append(int(idx.last_search_stats()[3]))
                return out
            (gw, gk, g_out), (xw, xk, x_out) = alternate(graph, lambda: idx.search_exact_batch_filtered_groups(q, K, tables, rows, group_of))
            stats = idx.last_exact_filtered()
            recall = float(np.mean([len(set(g_out[0][i][:g_out[2][i]].tolist()) & set(x_out[0][i].tolist())) / K for i in range(nq)]))
            what = "share 1/%d, %d queries, %d groups" % (n, nq, groups)
            line(what + ": graph", gw, gk)
            line(what + ": exact", xw, xk)
            bar = 3 * max(max(gw) - min(gw), max(xw) - min(xw))
            print("  wall graph / exact = %.2f; graph - exact = %.3f ms against a bar of %.3f ms (3 x the larger spread): %s\n"
                  "  exact: listed %d rows, %d distances, %d pass(es), %d bytes of list scratch; filled k %d of %d\n"
                  "  graph: recall@10 %.4f against the exact answers, filled k %d of %d, re-run queries %d"
                  % (np.median(gw) / np.median(xw), np.median(gw) - np.median(xw), bar,
                     "exact is faster" if np.median(gw) - np.median(xw) > bar else
                     ("graph is faster" if np.median(xw) - np.median(gw) > bar else "no difference shown"),
                     int(stats[0]), int(stats[1]), int(stats[2]), int(stats[3]), int((x_out[2] == K).sum()), nq,
                     recall, int((g_out[2] == K).sum()), nq, reruns[-1]), flush=True)

if "ones" in legs:
    ones = np.full((1, (rows + 63) // 64), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    (mw, mk, m_out), (xw, xk, x_out) = alternate(lambda: idx.search_batch(Q, K, exact=True),
                                                 lambda: idx.search_exact_batch_filtered_groups(Q, K, ones, rows, None))
    same = all(np.array_equal(a, b) for a, b in zip((m_out[0], m_out[1].view(np.uint32), m_out[2]),
                                                    (x_out[0], x_out[1].view(np.uint32), x_out[2])))
    line("all ones, 1024 queries: vss_search_exact_batch", mw, None)  # (the MFMA path keeps no kernel time)
    line("all ones, 1024 queries: exact filtered", xw, xk)
    print("  wall exact filtered / MFMA path = %.2f; identical answers %s" % (np.median(xw) / np.median(mw), same), flush=True)
