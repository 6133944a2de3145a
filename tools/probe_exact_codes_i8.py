"""A/B of the exact search's three score kinds on one index and one query block: the f32 tile (0), exact.split_bf16 (1) and
exact.codes_i8 (2: bounds from the int8 row codes, k_exact_bounds_i8 + the range search of kind 2).  The data and the cheap graph
are tools/probe_exact_split_bf16.py's.  Per (metric, k) the three kinds run in turn and then again in the same process; per run:
the device form's milliseconds between two events on the index's stream (median of --repeats after a warm-up, and max - min),
vss_last_exact_scores, the queries redone and, for kind 2, the pairs re-scored per answer cell.  The answers of the kinds are
compared cell for cell on the way.
    python tools/probe_exact_codes_i8.py [--rows 1000000] [--dim 768] [--out profiles/exact_codes_i8.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

OPTIONS = {0: (0, 0), 1: (1, 0), 2: (0, 1)}  # kind -> (exact.split_bf16, exact.codes_i8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--metrics", default="cosine,l2sq")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_codes_i8.json"))
    args = ap.parse_args()
    pkg = load_package()
    dev = torch.device("cuda", 0)
    results = []
    for metric in args.metrics.split(","):
        gen = bench.Mixture(args.rows, args.dim, metric != "l2sq", dev)
        idx = pkg.GpuIndex(args.dim, metric, 8, 16, 16)
        stream = torch.cuda.Stream()  # (the index works on this stream, so that the events below bracket its kernels)
        idx.set_stream(stream.cuda_stream)
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
        print("%s: %d x %d indexed" % (metric, args.rows, args.dim), flush=True)
        nq = args.queries
        Q = gen.rows(bench.QUERY_SEED, 0, nq)
        for k in (int(v) for v in args.ks.split(",")):
            answers = {}
            for turn in (0, 1):
                for kind in (0, 1, 2):
                    idx.set_option("exact.split_bf16", OPTIONS[kind][0])
                    idx.set_option("exact.codes_i8", OPTIONS[kind][1])
                    keys = torch.empty((nq, k), dtype=torch.int64, device=dev)
                    dist = torch.empty((nq, k), dtype=torch.float32, device=dev)
                    cnt = torch.empty(nq, dtype=torch.int32, device=dev)
                    call = []
                    for r in range(args.repeats + 1):  # (the first one warms up: scratch allocations, the row norms)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        e0.record(stream)
                        idx.search_batch_device(Q.data_ptr(), nq, k, 0, keys.data_ptr(), dist.data_ptr(), cnt.data_ptr(), exact=True)
                        e1.record(stream)
                        torch.cuda.synchronize()
                        call.append(e0.elapsed_time(e1))
                    ran, launches, E, rescored = idx.last_exact_scores()
                    call = sorted(call[1:])
                    r = dict(metric=metric, rows=args.rows, dim=args.dim, queries=nq, k=k, turn=turn, option=kind, score_kind=ran,
                             score_launches=launches, call_ms_median=float(np.median(call)), call_ms_spread=call[-1] - call[0],
                             call_ms=call, redone=idx.last_exact_fallbacks(), E_or_slack=E, rescored_per_cell=rescored / (nq * k))
                    print(json.dumps(r), flush=True)
                    results.append(r)
                    answers[kind] = (keys.cpu().numpy(), dist.cpu().numpy().view(np.uint32), cnt.cpu().numpy())
            same = all(np.array_equal(a, b) for kind in (1, 2) for a, b in zip(answers[0], answers[kind]))
            results.append(dict(metric=metric, queries=nq, k=k, answers_identical=bool(same)))
            print("answers identical: %s" % same, flush=True)
        idx.close()
        del gen
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
