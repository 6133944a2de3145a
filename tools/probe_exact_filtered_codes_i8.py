"""A/B of the exact search under per-query predicates with exact.filtered_codes_i8 at 0 (the metric kernel, k_exact_filtered_scores)
and at 1 (bounds from the int8 row codes gathered through the lists, k_exact_filtered_bounds_i8 + the gathered range search of
kind 2), on one index in one process, alternating.  The data and the tenants are tools/probe_exact_filtered.py's: the benchmark's
mixture, query q belongs to tenant q mod n, tenant t admits the rows r with tenant[r] == t (a random assignment); the graph is a
cheap one, only the exact path runs.  Per (share, queries, k): whole host-pointer calls of vss_search_exact_batch_filtered_groups,
wall milliseconds (the call blocks) and vss_timing's kernel milliseconds, median and max - min of --repeats after a warm-up each;
vss_last_exact_filtered, vss_last_exact_filtered_scores; the answers of the two settings compared cell for cell.
    python tools/probe_exact_filtered_codes_i8.py [--rows 1000000] [--dim 128] [--out profiles/exact_filtered_codes_i8.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def bitmap_of(mask):
    pad = (-len(mask)) % 64
    return np.packbits(np.concatenate([mask, np.zeros(pad, dtype=bool)]).astype(np.uint8), bitorder="little").view(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--metric", default="l2sq")
    ap.add_argument("--shares", default="2,16,256")
    ap.add_argument("--queries", default="1024,204")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_filtered_codes_i8.json"))
    args = ap.parse_args()
    pkg = load_package()
    dev = torch.device("cuda", 0)
    gen = bench.Mixture(args.rows, args.dim, args.metric != "l2sq", dev)
    idx = pkg.GpuIndex(args.dim, args.metric, 8, 16, 16)
    idx.reserve(args.rows)
    idx.set_build_params(65536, 4)
    for c in range(0, args.rows, bench.CHUNK):
        m = min(bench.CHUNK, args.rows - c)
        x = gen.rows(bench.DATA_SEED, c // bench.CHUNK, m)
        ids = torch.arange(c, c + m, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        idx.stage_device(ids.data_ptr(), x.data_ptr(), m)
        del x, ids
    idx.build_finalize()
    torch.cuda.synchronize()
    print("library %s\n%s: %d x %d indexed" % (pkg.LIB_PATH, args.metric, args.rows, args.dim), flush=True)
    Q = gen.rows(bench.QUERY_SEED, 0, 1024).cpu().numpy()
    rng = np.random.default_rng(20261019)
    results = []
    for n in (int(s) for s in args.shares.split(",")):
        tenant = rng.integers(0, n, size=args.rows)
        for nq in (int(s) for s in args.queries.split(",")):
            groups = min(n, nq)
            tables = np.stack([bitmap_of(tenant == g) for g in range(groups)])
            group_of = (np.arange(nq) % groups).astype(np.uint32)
            q = np.ascontiguousarray(Q[:nq])
            for k in (int(s) for s in args.ks.split(",")):
                wall, kern, out, stats = ([], []), ([], []), [None, None], [None, None]
                for r in range(args.repeats + 1):  # (the first round warms up: scratch allocations, the row codes, the norms)
                    for option in (0, 1):
                        idx.set_option("exact.filtered_codes_i8", option)
                        t = time.perf_counter()
                        out[option] = idx.search_exact_batch_filtered_groups(q, k, tables, args.rows, group_of)
                        w = (time.perf_counter() - t) * 1e3
                        if r:
                            wall[option].append(w), kern[option].append(idx.timing()["search_kernel_ms"])
                        stats[option] = ([int(v) for v in idx.last_exact_filtered()], idx.last_exact_filtered_scores())
                same = all(np.array_equal(a, b) for a, b in zip((out[0][0], out[0][1].view(np.uint32), out[0][2]),
                                                                (out[1][0], out[1][1].view(np.uint32), out[1][2])))
                for option in (0, 1):
                    w, km = sorted(wall[option]), sorted(kern[option])
                    r = dict(metric=args.metric, rows=args.rows, dim=args.dim, share=n, queries=nq, groups=groups, k=k, option=option,
                             kind=stats[option][1][0], bound_launches=stats[option][1][1], slack=stats[option][1][2],
                             rescored=stats[option][1][3], listed=stats[option][0][0], distances=stats[option][0][1],
                             passes=stats[option][0][2], wall_ms_median=float(np.median(w)), wall_ms_spread=w[-1] - w[0], wall_ms=w,
                             kernel_ms_median=float(np.median(km)), kernel_ms_spread=km[-1] - km[0], answers_identical=bool(same))
                    print(json.dumps(r), flush=True)
                    results.append(r)
    idx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
