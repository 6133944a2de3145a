"""Round 7: the candidate list of search limits 513-4096 in LDS (search.list_lds) against the list in HBM.
The benchmark's rows (1M x 768 cosine by default) under the reference's default index options (M 16, ef_construction 128); one
launch of 20 x 1024 queries per measurement at ef 768, 1536 and 4096, with search.list_lds 0 and 1, five repeats each: kernel
milliseconds (vss_timing), the work counters, and the algorithmic bytes over time as bench.py computes them
(n_dist * (4 * dim + 4) + n_expand * (4 + 4 * M0)).  Answers and work counters of the two placements must be identical.
A library without the option (an older build, VSS_LIBRARY=...) is measured as it is: that run is the baseline.
    python tools/probe_lds_list.py [rows [dim [metric [ef,ef,...]]]]"""
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
efs = [int(e) for e in (sys.argv[4] if len(sys.argv) > 4 else "768,1536,4096").split(",")]
M, M0, EFC, K, B, G, REPEATS = 16, 32, 128, 10, 1024, 20, 5
pkg = load_package()
import ctypes  # noqa: E402
HAVE_SHAPE = hasattr(ctypes.CDLL(pkg.LIB_PATH), "vss_last_search_shape")
if not HAVE_SHAPE:  # an older library (the baseline run): bind what it has
    pkg.SIGNATURES.pop("vss_last_search_shape")
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

modes = []
for mode in (0, 1):
    try:
        idx.set_option("search.list_lds", mode)
        modes.append(mode)
    except pkg.VssError:
        pass
if not modes:
    print("this library has no search.list_lds: measured as it is (the list in HBM)")
    modes = [None]
PLACES = {0: "registers", 1: "LDS", 2: "HBM"}
bad = 0
for ef in efs:
    ref = None
    for mode in modes:
        if mode is not None:
            idx.set_option("search.list_lds", mode)
        ms_all = []
        for r in range(REPEATS + 1):  # (the first one warms up: scratch allocations)
            torch.cuda.synchronize()
            idx.search_multi_begin(0, [q.data_ptr() for q in Q], B, K, ef, [o[0].data_ptr() for o in outs],
                                   [o[1].data_ptr() for o in outs], [o[2].data_ptr() for o in outs])
            idx.search_end(0)
            ms_all.append(idx.timing()["search_kernel_ms"])
        ms_all = ms_all[1:]
        st = idx.last_search_stats()
        shape = idx.last_search_shape() if HAVE_SHAPE else None
        gb = (float(st[0]) * (4 * dim + 4) + float(st[1]) * (4 + 4 * M0)) / 1e9
        ms = float(np.median(ms_all))
        ans = [o[j].cpu().numpy().view(np.uint32 if j == 1 else o[j].cpu().numpy().dtype).copy() for o in (outs[0], outs[G - 1])
               for j in range(3)] + [np.array([int(st[0]), int(st[1])])]
        if ref is None:
            ref = ans
        same = all(np.array_equal(a, b) for a, b in zip(ref, ans))
        bad += not same
        print("ef %4d  list_lds %-4s list in %-9s walkers %s  kernel ms %s  median %8.2f spread %5.2f -> %7.0f queries/s, %5.0f GB/s = "
              "%.3f of 8 TB/s; distances %d expansions %d re-run %d; identical %s"
              % (ef, mode, PLACES[int(shape[4])] if shape is not None else "HBM", int(shape[1]) if shape is not None else -1,
                 " ".join("%.2f" % v for v in ms_all), ms, max(ms_all) - min(ms_all), G * B / ms * 1e3, gb / (ms / 1e3),
                 gb / (ms / 1e3) / 8000, int(st[0]), int(st[1]), int(st[3]), same), flush=True)
print("DIFFERENCES: %d" % bad)
sys.exit(1 if bad else 0)
