"""The exact search's certificate (csrc/exact_certificate.h) on the benchmark's kind of data: how many queries it cannot vouch
for (they are answered again by brute force in the metric: vss_last_exact_fallbacks) and what the exact call costs.
bench.Mixture rows under a cheap graph (M 8, ef_construction 16: only the exact path is measured), 1024 queries, k = 10 and 100;
per k the fallbacks and the call's milliseconds between two hipEvents on the index's stream, five repeats after one warm-up.
On this data the fallbacks must be 0.  Run it once more with VSS_LIBRARY pointing at another build of the engine (the parent
commit's, which has no certificate and no getter: its fallbacks print as n/a) for the time the certificate costs.
    python tools/probe_exact_certificate.py [rows [dim [metric]]]"""
import os
import sys

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
B, REPEATS = 1024, 5
pkg = load_package()
import ctypes  # noqa: E402
HAVE_GETTER = hasattr(ctypes.CDLL(pkg.LIB_PATH), "vss_last_exact_fallbacks")
if not HAVE_GETTER:  # an older library (the baseline run): bind what it has
    pkg.SIGNATURES.pop("vss_last_exact_fallbacks")
dev = torch.device("cuda", 0)
gen = bench.Mixture(rows, dim, metric != "l2sq", dev)
idx = pkg.GpuIndex(dim, metric, 8, 16, 16)
stream = torch.cuda.Stream()  # (the index works on this stream, so that the events below bracket its kernels)
idx.set_stream(stream.cuda_stream)
idx.reserve(rows)
idx.set_build_params(65536, 4)
for c in range(0, rows, bench.CHUNK):
    m = min(bench.CHUNK, rows - c)
    x = gen.rows(bench.DATA_SEED, c // bench.CHUNK, m)
    ids = torch.arange(c, c + m, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    idx.stage_device(ids.data_ptr(), x.data_ptr(), m)
    del x, ids
idx.build_finalize()
torch.cuda.synchronize()
print("library %s (%s)  VSS_EXACT_CERTIFY=%s\n%d x %d %s, %d queries"
      % (os.path.relpath(pkg.LIB_PATH, os.path.dirname(HERE)), "certifies" if HAVE_GETTER else "no certificate: an older build",
         os.environ.get("VSS_EXACT_CERTIFY", "(unset)"), rows, dim, metric, B), flush=True)
Q = gen.rows(bench.QUERY_SEED, 0, B)
bad = 0
for k in (10, 100):
    keys = torch.empty((B, k), dtype=torch.int64, device=dev)
    dist = torch.empty((B, k), dtype=torch.float32, device=dev)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)
    ms = []
    for r in range(REPEATS + 1):  # (the first one warms up: scratch allocations, the row norms)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        idx.search_batch_device(Q.data_ptr(), B, k, 0, keys.data_ptr(), dist.data_ptr(), cnt.data_ptr(), exact=True)
        e1.record(stream)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[1:]
    redone = idx.last_exact_fallbacks() if HAVE_GETTER else None
    bad += redone or 0
    d = dist.cpu().numpy()
    print("k %3d  fallbacks %s of %d  exact call ms %s  median %.2f spread %.2f  (sorted %s, counts %s)"
          % (k, "n/a" if redone is None else redone, B, " ".join("%.2f" % v for v in ms), float(np.median(ms)), max(ms) - min(ms),
             bool(np.all(d[:, 1:] >= d[:, :-1])), bool((cnt == k).all().item())), flush=True)
print("FALLBACKS: %d" % bad)
sys.exit(1 if bad else 0)
