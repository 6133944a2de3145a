"""A/B of the exact search's two score kinds on one index and one query block: option exact.split_bf16 at 0 (the f32 tile)
and at 1 (k_exact_scores_bf16x3).  The data and the cheap graph are tools/probe_exact_certificate.py's (bench.Mixture, M 8,
ef_construction 16).  Per (metric, queries, k, kind): the exact call's milliseconds between two events on the index's stream,
the device time of its first pass (score tiles + selects: GpuIndex.timing()["search_kernel_ms"]), the queries redone, the
certificate's E; the answers of the two kinds are compared cell for cell on the way.
    python tools/probe_exact_split_bf16.py [--rows 1000000] [--dim 768] [--out profiles/exact_split_bf16.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--metrics", default="cosine,l2sq")
    ap.add_argument("--queries", default="1024,128")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_split_bf16.json"))
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
        for nq in (int(q) for q in args.queries.split(",")):
            Q = gen.rows(bench.QUERY_SEED, 0, nq)
            for k in (int(v) for v in args.ks.split(",")):
                answers = {}
                for kind in (0, 1):
                    idx.set_option("exact.split_bf16", kind)
                    keys = torch.empty((nq, k), dtype=torch.int64, device=dev)
                    dist = torch.empty((nq, k), dtype=torch.float32, device=dev)
                    cnt = torch.empty(nq, dtype=torch.int32, device=dev)
                    call, first = [], []
                    for r in range(args.repeats + 1):  # (the first one warms up: scratch allocations, the row norms)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        e0.record(stream)
                        idx.search_batch_device(Q.data_ptr(), nq, k, 0, keys.data_ptr(), dist.data_ptr(), cnt.data_ptr(), exact=True)
                        e1.record(stream)
                        torch.cuda.synchronize()
                        call.append(e0.elapsed_time(e1))
                        first.append(float(idx.timing()["search_kernel_ms"]))
                    ran, launches, E, _ = idx.last_exact_scores()
                    r = dict(metric=metric, rows=args.rows, dim=args.dim, queries=nq, k=k, option=kind, score_kind=ran,
                             score_launches=launches, call_ms=sorted(call[1:]), first_pass_ms=sorted(first[1:]),
                             redone=idx.last_exact_fallbacks(), E=E)
                    print(json.dumps(r), flush=True)
                    results.append(r)
                    answers[kind] = (keys.cpu().numpy(), dist.cpu().numpy().view(np.uint32), cnt.cpu().numpy())
                same = all(np.array_equal(a, b) for a, b in zip(answers[0], answers[1]))
                results.append(dict(metric=metric, queries=nq, k=k, answers_identical=bool(same)))
                print("answers identical: %s" % same, flush=True)
        idx.close()
        del gen
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
