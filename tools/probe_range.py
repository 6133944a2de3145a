"""The exact range search (vss_search_range_batch_device) beside the exact top-k on ONE index: bench.Mixture rows under a cheap
graph (M 8, ef_construction 16: only the exact paths are measured), 1024 queries, every radius = the distance of the query's
100th neighbour as vss_search_exact_batch(k = 100) reports it — about 100 matches per query.  Prints the milliseconds of the
range call (count-only and with the cells filled) and of the exact top-100 call, each between two hipEvents on the index's
stream, five repeats after one warm-up, and candidates / matches from vss_last_range: how many rows the score threshold hands
to the re-score per row that matches (set by the certificate's E: 1.8e-4 for cosine at 768 dimensions).
--split measures the range calls under option range.split_bf16 = 0 and = 1 in turn (the f32 and the split-bf16 candidate tiles),
ten repeats each, with vss_last_range_scores' kind and E beside the candidates.
--codes-i8 measures them under kinds 0, 1 and 2 in turn, twice (range.codes_i8 = 1 for the int8 tiles over the row codes; the
figure beside kind 2 is the largest per-query slack of its pair test, not an E).
    python tools/probe_range.py [--split | --codes-i8] [rows [dim [metric [neighbour]]]]"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import bench  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

SPLIT, CODES = "--split" in sys.argv, "--codes-i8" in sys.argv
sys.argv = [a for a in sys.argv if a not in ("--split", "--codes-i8")]
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
dim = int(sys.argv[2]) if len(sys.argv) > 2 else 768
metric = sys.argv[3] if len(sys.argv) > 3 else "cosine"
K = int(sys.argv[4]) if len(sys.argv) > 4 else 100
B, REPEATS = 1024, 10 if SPLIT or CODES else 5
pkg = load_package()
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
print("%d x %d %s, %d queries, radius = distance of neighbour %d" % (rows, dim, metric, B, K), flush=True)
Q = gen.rows(bench.QUERY_SEED, 0, B)


def timed(call):
    ms = []
    for _ in range(REPEATS + 1):  # (the first one warms up: scratch allocations, the row norms)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        call()
        e1.record(stream)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[1:]
    return "%s  median %.2f spread %.2f" % (" ".join("%.2f" % v for v in ms), float(np.median(ms)), max(ms) - min(ms))


keys = torch.empty((B, K), dtype=torch.int64, device=dev)
dist = torch.empty((B, K), dtype=torch.float32, device=dev)
cnt = torch.empty(B, dtype=torch.int32, device=dev)
print("exact top-%d call ms  %s" % (K, timed(lambda: idx.search_batch_device(Q.data_ptr(), B, K, 0, keys.data_ptr(), dist.data_ptr(),
                                                                            cnt.data_ptr(), exact=True))), flush=True)
radii = dist[:, K - 1].contiguous()
offsets = torch.zeros(B + 1, dtype=torch.int64, device=dev)
total = torch.zeros(1, dtype=torch.int64, device=dev)
torch.cuda.synchronize()


def range_calls():
    print("range call ms, count only  %s" % timed(lambda: idx.search_range_batch_device(Q.data_ptr(), B, radii.data_ptr(), 0, offsets.data_ptr(),
                                                                                        None, None, total.data_ptr())), flush=True)
    n = int(total.item())
    r_ids = torch.empty(n, dtype=torch.int64, device=dev)
    r_d = torch.empty(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    print("range call ms, %d cells    %s" % (n, timed(lambda: idx.search_range_batch_device(Q.data_ptr(), B, radii.data_ptr(), n, offsets.data_ptr(),
                                                                                             r_ids.data_ptr(), r_d.data_ptr(), total.data_ptr()))),
          flush=True)
    stats = idx.last_range()
    per_query = (offsets[1:] - offsets[:-1]).cpu().numpy()
    print("candidates %d  matches %d  candidates / matches %.2f  queries without a bound %d  scratch %.1f MB"
          % (stats[0], stats[1], stats[0] / max(1, stats[1]), stats[2], stats[3] / 1e6))
    print("matches per query: min %d median %d max %d; the top-%d's rows are among them: %s"
          % (per_query.min(), np.median(per_query), per_query.max(), K, bool((per_query >= K).all())), flush=True)


if not SPLIT and not CODES:
    range_calls()
# (each kind twice, in turn: how far two equal runs lie apart is part of the answer)
for kind in ((0, 1, 2, 0, 1, 2) if CODES else (0, 1, 0, 1) if SPLIT else ()):
    idx.set_option("range.split_bf16", int(kind == 1))
    idx.set_option("range.codes_i8", int(kind == 2))
    print("range.split_bf16 = %d, range.codes_i8 = %d" % (kind == 1, kind == 2))
    range_calls()
    print("score kind %d, %d tile launches, E %.3g" % idx.last_range_scores()[:3], flush=True)
