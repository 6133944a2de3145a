"""The range search under per-query label boxes (vss_search_range_batch_by_label_box64) beside the only route there was before it:
vss_search_range_batch plus a filter on the host over the returned cells.  ONE index of bench.Mixture rows under a cheap graph
(only the exact paths are measured), 1024 queries, label column 0 = row id % T for T = 1, 16, 256 (tenant selectivity 1 / T),
query q wants tenant q % T, every radius = the distance of the query's 10th ADMITTED neighbour (the exact search by label box64
reports it) — about 10 matches per query.  Per T, interleaved, 10 repeats after one warm-up, median and spread (max - min):
  device form   the new call between two hipEvents on the index's stream (capacity = the total: the cells are filled)
  host form     the new call through GpuIndex.search_range_batch_by_label_box64 (count, then fill), wall clock
  old route     GpuIndex.search_range_batch (count, then fill) + numpy keeps the cells whose row has the query's tenant, wall clock
  dense device  vss_search_range_batch_device between two hipEvents, same radii
and the pairs scored with the whole-call rate 2 x dim x pairs / device time of the new and of the dense call (a call's rate, not
the tile kernel's: that takes a kernel trace in a run of its own).  The answers of the two routes are compared.
--split adds two legs to the same interleaved rounds: the device form and the dense device call under option range.split_bf16 = 1
(the split-bf16 candidate tiles), and prints the pairs the split score proposed beside the f32 score's.
    python tools/probe_range_filtered.py [--split] [rows [dim [metric]]]"""
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

SPLIT = "--split" in sys.argv
sys.argv = [a for a in sys.argv if a != "--split"]
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
dim = int(sys.argv[2]) if len(sys.argv) > 2 else 768
metric = sys.argv[3] if len(sys.argv) > 3 else "cosine"
B, K, REPEATS = 1024, 10, 10
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
print("%d x %d %s, %d queries, radius = distance of admitted neighbour %d" % (rows, dim, metric, B, K), flush=True)
d_Q = gen.rows(bench.QUERY_SEED, 0, B)
Q = d_Q.cpu().numpy()


def events(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    call()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def summary(ms):
    return "median %8.2f  spread %6.2f" % (float(np.median(ms)), max(ms) - min(ms))


for T in (1, 16, 256):
    tenant = (np.arange(rows) % T).astype(np.uint32)
    idx.set_label_column(0, 0, tenant)
    want = (np.arange(B, dtype=np.uint64) % T)[:, None]
    _, d, cnt, _ = idx.search_batch_by_label_box64(Q, K, 0, [0], want, want, mode="exact")
    assert (cnt == K).all()
    radii = np.ascontiguousarray(d[:, K - 1])
    d_radii, d_want = torch.from_numpy(radii).to(dev), torch.from_numpy(want.view(np.int64)).to(dev)
    d_off, d_total = torch.zeros(B + 1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    n_new = idx.search_range_batch_by_label_box64(Q, radii, [0], want, want, capacity=0)[3]
    n_old = idx.search_range_batch(Q, radii, capacity=0)[3]
    d_ids, d_d = torch.empty(max(n_old, 1), dtype=torch.int64, device=dev), torch.empty(max(n_old, 1), dtype=torch.float32, device=dev)
    got = {}

    def new_device():
        idx.search_range_batch_by_label_box64_device(d_Q.data_ptr(), B, d_radii.data_ptr(), [0], d_want.data_ptr(), d_want.data_ptr(),
                                                     n_new, d_off.data_ptr(), d_ids.data_ptr(), d_d.data_ptr(), d_total.data_ptr())

    def new_host():
        got["new"] = idx.search_range_batch_by_label_box64(Q, radii, [0], want, want)

    def old_route():
        offsets, ids, dist, _ = idx.search_range_batch(Q, radii)
        query = np.repeat(np.arange(B), np.diff(offsets.astype(np.int64)))
        keep = tenant[ids] == want[query, 0]
        got["old"] = (np.concatenate([[0], np.cumsum(np.bincount(query[keep], minlength=B))]), ids[keep], dist[keep])

    def dense_device():
        idx.search_range_batch_device(d_Q.data_ptr(), B, d_radii.data_ptr(), n_old, d_off.data_ptr(), d_ids.data_ptr(), d_d.data_ptr(),
                                      d_total.data_ptr())

    def split(clock):  # the same clock around a call under range.split_bf16 = 1 (set and reset outside the timed part)
        def timed(call):
            idx.set_option("range.split_bf16", 1)
            t = clock(call)
            proposed_split[0] = int(idx.last_range()[0])
            idx.set_option("range.split_bf16", 0)
            return t
        return timed

    proposed_split = [0]
    legs = [("device form", events, new_device), ("host form", wall, new_host), ("old route", wall, old_route),
            ("dense device", events, dense_device)]
    if SPLIT:
        legs += [("dense split", split(events), dense_device), ("device split", split(events), new_device)]
    ms = {name: [] for name, _, _ in legs}
    for rep in range(REPEATS + 1):  # (the first round warms up: scratch allocations, the row norms)
        for name, clock, call in legs:
            t = clock(call)
            if rep:
                ms[name].append(t)
            if name == "device form":
                pairs, launches = int(idx.last_range_filtered()[1]), int(idx.last_range_filtered()[2])
                listed, proposed = int(idx.last_range_filtered()[0]), int(idx.last_range()[0])
    # the two routes agree: per query the same (row id, distance bits)
    (o_new, i_new, x_new, _), (o_old, i_old, x_old) = got["new"], got["old"]
    same = np.array_equal(o_new.astype(np.int64), o_old.astype(np.int64))
    for q in range(B if same else 0):
        a, b = slice(int(o_new[q]), int(o_new[q + 1])), slice(int(o_old[q]), int(o_old[q + 1]))
        oa, ob = np.argsort(i_new[a]), np.argsort(i_old[b])
        same &= np.array_equal(i_new[a][oa], i_old[b][ob]) and np.array_equal(x_new[a][oa].view(np.uint32), x_old[b][ob].view(np.uint32))
    print("selectivity 1/%d: %d matches (%d unfiltered), %d rows listed, %d pairs scored, %d proposed, %d tile launches, routes agree: %s"
          % (T, n_new, n_old, listed, pairs, proposed, launches, bool(same)), flush=True)
    for name, _, _ in legs:
        print("  %-13s ms  %s" % (name, summary(ms[name])), flush=True)
    if SPLIT:
        print("  device split proposed %d pairs (f32: %d) for %d matches" % (proposed_split[0], proposed, n_new), flush=True)
    new_ms, dense_ms = float(np.median(ms["device form"])), float(np.median(ms["dense device"]))
    print("  whole-call rate: new %.1f TFLOP/s over %d pairs, dense %.1f TFLOP/s over %d pairs"
          % (2.0 * dim * pairs / new_ms / 1e9, pairs, 2.0 * dim * B * rows / dense_ms / 1e9, B * rows), flush=True)
