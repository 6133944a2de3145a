"""Pre-scoring on 8-bit row codes (search.prescore) against the same launches without it.
The benchmark's rows (1M x 768 cosine by default) under the given index options (the benchmark's M 32 / ef_construction 384 by
default; pass 16 128 for the reference's defaults); one launch of 20 x 1024 queries per measurement at each ef, with
search.prescore 0 and 1 (and 2 at limits above 256, which 1 leaves unfiltered; each filtering setting with search.prescore_descent 0
and 1: the greedy descent's rows unbounded / bounded), five repeats each: kernel milliseconds (vss_timing), the work counters, the algorithmic bytes over
time as bench.py computes them (n_dist * (4 * dim + 4) + n_expand * (4 + 4 * M0) — no longer bounded by the HBM rate once rows
are rejected on their codes), the share of pre-scored rows that were rejected (vss_last_search_prescore), and the descent's rows
handed over with a bound and rejected (vss_last_search_prescore_descent).  Answers and work counters of all settings must be
identical.
    python tools/probe_prescore.py [rows [dim [metric [ef,ef,... [M [ef_construction]]]]]]"""
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
metric = sys.argv[3] if len(sys.argv) > 3 else "cosine"
efs = [int(e) for e in (sys.argv[4] if len(sys.argv) > 4 else "60,512").split(",")]
M = int(sys.argv[5]) if len(sys.argv) > 5 else bench.HEADLINE_OPTIONS["M"]
EFC = int(sys.argv[6]) if len(sys.argv) > 6 else bench.HEADLINE_OPTIONS["ef_construction"]
M0, K, B, G, REPEATS = 2 * M, 10, 1024, 20, 5
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
Q = [gen.rows(bench.QUERY_SEED, i, B) for i in range(G)]
outs = [(torch.empty((B, K), dtype=torch.int64, device=dev), torch.empty((B, K), dtype=torch.float32, device=dev),
         torch.empty(B, dtype=torch.int32, device=dev)) for _ in range(G)]
torch.cuda.synchronize()

bad = 0
for ef in efs:
    ref = None
    # (1 leaves limits of 257-512 alone, 2 filters there too)
    for mode, descent in ((0, 1), (1, 0), (1, 1)) if max(ef, K) <= 256 else ((0, 1), (1, 1), (2, 0), (2, 1)):
        idx.set_option("search.prescore", mode)
        idx.set_option("search.prescore_descent", descent)
        ms_all = []
        for r in range(REPEATS + 1):  # (the first one warms up: scratch allocations)
            torch.cuda.synchronize()
            idx.search_multi_begin(0, [q.data_ptr() for q in Q], B, K, ef, [o[0].data_ptr() for o in outs],
                                   [o[1].data_ptr() for o in outs], [o[2].data_ptr() for o in outs])
            idx.search_end(0)
            ms_all.append(idx.timing()["search_kernel_ms"])
        ms_all = ms_all[1:]
        st = idx.last_search_stats()
        pre = idx.last_search_prescore()
        desc = idx.last_search_prescore_descent()
        gb = (float(st[0]) * (4 * dim + 4) + float(st[1]) * (4 + 4 * M0)) / 1e9
        ms = float(np.median(ms_all))
        ans = [o[j].cpu().numpy().view(np.uint32 if j == 1 else o[j].cpu().numpy().dtype).copy() for o in outs for j in range(3)]
        ans.append(np.array([int(st[0]), int(st[1])]))
        if ref is None:
            ref = ans
        same = all(np.array_equal(a, b) for a, b in zip(ref, ans))
        bad += not same
        print("ef %4d  prescore %d descent %d active %d  kernel ms %s  median %8.2f spread %5.2f -> %7.0f queries/s, algorithmic %5.0f GB/s = "
              "%.3f of 8 TB/s; distances %d expansions %d; pre-scored %d rejected %d = %.3f of pre-scored, %.3f of all rows; "
              "descent: %d rows with a bound (%.1f per query), %d rejected = %.3f; code bytes %d; identical %s"
              % (ef, mode, descent, int(pre[0]), " ".join("%.2f" % v for v in ms_all), ms, max(ms_all) - min(ms_all), G * B / ms * 1e3,
                 gb / (ms / 1e3), gb / (ms / 1e3) / 8000, int(st[0]), int(st[1]), int(pre[1]), int(pre[2]),
                 int(pre[2]) / max(1, int(pre[1])), int(pre[2]) / max(1, int(st[0])), int(desc[0]), int(desc[0]) / (G * B), int(desc[1]),
                 int(desc[1]) / max(1, int(desc[0])), int(pre[3]), same), flush=True)
# The regimes that run mostly in crew mode (one walker per workgroup) and must not get slower: ONE batch per launch, the
# 204-query host chunk and the single vss_search — wall-clock medians through the blocking calls, option 0 against 1.
ef0 = efs[0]
qh = [q.cpu().numpy() for q in Q[:4]]
for mode in (0, 1):
    idx.set_option("search.prescore", mode)
    t_batch, t_chunk, t_one = [], [], []
    for r in range(3 + 20):
        q = Q[r % G]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx.search_batch_device(q.data_ptr(), B, K, ef0, outs[0][0].data_ptr(), outs[0][1].data_ptr(), outs[0][2].data_ptr())
        t_batch.append(time.perf_counter() - t0)
        pre_batch = idx.last_search_prescore()
        t0 = time.perf_counter()
        idx.search_batch(qh[r % 4][:204], K, ef0)
        t_chunk.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        idx.search(qh[r % 4][r % B], K, ef0)
        t_one.append(time.perf_counter() - t0)
    med = [float(np.median(t[3:])) * 1e6 for t in (t_batch, t_chunk, t_one)]
    print("ef %4d  prescore %d  one batch of %d per launch %8.1f us (%7.0f queries/s; rejected %d of %d pre-scored)  204-query chunk "
          "%7.1f us  one vss_search %7.1f us" % (ef0, mode, B, med[0], B / med[0] * 1e6, int(pre_batch[2]), int(pre_batch[1]), med[1],
                                                  med[2]), flush=True)
print("DIFFERENCES: %d" % bad)
sys.exit(1 if bad else 0)
