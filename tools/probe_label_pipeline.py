"""Label predicates in the pipelined and multi-batch launches (vss_search_by_label_device_begin,
vss_search_multi_by_label_device_begin) against the blocking _device calls in mode graph, which were the only way to walk under a
label predicate.  One index in one process, the roads in turn.
The shape of the other label probes: the benchmark's mixture, 1M x 128, the reference's default index options (M 16,
ef_construction 128), k 10, ef 64, chunks of 204 queries, every query its own predicate.  Column 0 holds a group of 8 values, 32
bits wide (a walk under an equality on one of 64 groups rejects 63 rows of 64: that predicate takes the scan, not this road); column 1 a TIMESTAMP, 64 bits wide.  Two forms:
    eq        `items.grp = q.grp`                                                  (vss_search_batch_by_label_device)
    set box   `items.grp IN (4 of the 8 groups) AND items.ts >= q.since`, 25-60 % of the rows behind `since`
                                                                                   (vss_search_batch_by_label_set_box_device)
N chunks (default 32), all words on the device beforehand, three repetitions after a warm-up, median and spread (max - min) of the
wall time of
    (a) N blocking _device calls in mode graph, one after the other, on context 0
    (b) the same N chunks as one-batch launches through three contexts in flight (1, 2, 3: the oldest is ended, the next begun)
        — with the pipelining gate on (the default) and off
    (c) the same N chunks as launches of up to 32 batches, one after the other, on context 1
  and the ratios (a) / (b) and (a) / (c).  The answers of (b) and (c) are compared with (a)'s, cell for cell.
Then what ShardedHNSWIndex::SearchBatchByLabel* does per probe in mode graph, on G (default 2) row-range shards CO-RESIDENT on this
one device, each its own index over rows / G rows and the whole columns: BEFORE — the blocking _device call shard after shard;
AFTER — every shard begun through the _begin call, then every shard ended.  (The upload, the exchange and the merge around them
did not change and are not part of either figure.)
    python tools/probe_label_pipeline.py [rows [dim [chunks [shards]]]]"""
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
N = int(sys.argv[3]) if len(sys.argv) > 3 else 32
G = int(sys.argv[4]) if len(sys.argv) > 4 else 2
metric, M, M0, EFC, K, EF, REPEATS, NQ, GROUPS, STAMPS, LIST = "l2sq", 16, 32, 128, 10, 64, 3, 204, 8, 1_000_000, 4
TOP64, EPOCH, SIGN = np.uint64(0xFFFFFFFFFFFFFFFF), 10 ** 15, np.uint64(1 << 63)
pkg = load_package()
dev = torch.device("cuda", 0)
gen = bench.Mixture(rows, dim, False, dev)
rng = np.random.default_rng(20261022)
grp = rng.integers(0, GROUPS, size=rows).astype(np.uint32)
stamp = (rng.integers(0, STAMPS, size=rows).astype(np.int64) + EPOCH).view(np.uint64) ^ SIGN  # TIMESTAMP microseconds -> unsigned, in order


def build(first, count):
    """an index over rows [first, first + count) of the mixture, row id = position, holding the whole columns"""
    idx = pkg.GpuIndex(dim, metric, M, M0, EFC)
    idx.reserve(count)
    for c in range(first, first + count, bench.CHUNK):
        m = min(bench.CHUNK, first + count - c)
        x = gen.rows(bench.DATA_SEED, c // bench.CHUNK, m)  # (first is a multiple of bench.CHUNK)
        ids = torch.arange(c, c + m, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        idx.stage_device(ids.data_ptr(), x.data_ptr(), m)
        del x, ids
    idx.build_finalize()
    torch.cuda.synchronize()
    idx.set_label_column(0, 0, grp)
    idx.set_label_column64(1, 0, stamp)
    return idx


def dev_of(a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).to(dev)


class Out:
    def __init__(self, n):
        self.keys = torch.empty((n, NQ, K), dtype=torch.int64, device=dev)
        self.dist = torch.empty((n, NQ, K), dtype=torch.float32, device=dev)
        self.cnt = torch.empty((n, NQ), dtype=torch.int32, device=dev)

    def ptrs(self, c):
        return self.keys[c].data_ptr(), self.dist[c].data_ptr(), self.cnt[c].data_ptr()

    def same(self, o):
        torch.cuda.synchronize()
        return bool(torch.equal(self.keys, o.keys) and torch.equal(self.dist.view(torch.int32), o.dist.view(torch.int32))
                    and torch.equal(self.cnt, o.cnt))


t0 = time.perf_counter()
idx = build(0, rows)
print("built %d x %d %s M %d efc %d in %.1f s; k %d ef %d; %d chunks of %d queries" % (rows, dim, metric, M, EFC, time.perf_counter() - t0, K, EF,
                                                                                     N, NQ), flush=True)
d_Q = torch.stack([gen.rows(bench.QUERY_SEED, c, NQ) for c in range(N)]).contiguous()
want = dev_of(rng.integers(0, GROUPS, (N, NQ)).astype(np.uint32))
sets = dev_of(np.stack([rng.choice(GROUPS, LIST, replace=False) for _ in range(N * NQ)]).astype(np.uint64).reshape(N, NQ, LIST))
since = dev_of(((rng.integers(int(0.40 * STAMPS), int(0.75 * STAMPS), (N, NQ, 1)).astype(np.int64) + EPOCH).view(np.uint64) ^ SIGN))
until = dev_of(np.full((N, NQ, 1), TOP64, dtype=np.uint64))
torch.cuda.synchronize()
P = pkg.LabelPredicate
FORMS = {
    "eq": (lambda ix, c, out: ix.search_batch_by_label_device(d_Q[c].data_ptr(), NQ, K, EF, want[c].data_ptr(), *out, None, "graph"),
           lambda c: P.eq(want[c])),
    "set box": (lambda ix, c, out: ix.search_batch_by_label_set_box_device(d_Q[c].data_ptr(), NQ, K, EF, 0, sets[c].data_ptr(), LIST, [1],
                                                                          since[c].data_ptr(), until[c].data_ptr(), *out, None, "graph"),
                lambda c: P.set_box(0, sets[c], LIST, [1], since[c], until[c])),
}


def timed(road):
    wall = []
    for r in range(REPEATS + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        road()
        if r:
            wall.append((time.perf_counter() - t) * 1e3)
    return wall


def line(name, wall):
    print("%-44s wall ms %s  median %9.3f spread %7.3f" % (name, " ".join("%.2f" % v for v in wall), float(np.median(wall)),
                                                           max(wall) - min(wall)), flush=True)


for form, (blocking, predicate) in FORMS.items():
    preds = [predicate(c) for c in range(N)]
    a_out, b_out, c_out = Out(N), Out(N), Out(N)

    def road_a():
        for c in range(N):
            blocking(idx, c, a_out.ptrs(c))

    def road_b():
        flying = []
        for c in range(N):
            if len(flying) == 3:
                idx.search_end(flying.pop(0))
            context = 1 + c % 3
            idx.search_by_label_begin(context, d_Q[c].data_ptr(), NQ, K, EF, preds[c], *b_out.ptrs(c))
            flying.append(context)
        for context in flying:
            idx.search_end(context)

    def road_c():
        for first in range(0, N, 32):
            cs = range(first, min(first + 32, N))
            idx.search_multi_by_label_begin(1, [d_Q[c].data_ptr() for c in cs], NQ, K, EF, [preds[c] for c in cs],
                                            [c_out.ptrs(c)[0] for c in cs], [c_out.ptrs(c)[1] for c in cs], [c_out.ptrs(c)[2] for c in cs])
            idx.search_end(1)

    aw = timed(road_a)
    line(form + ": (a) %d blocking calls" % N, aw)
    bw = timed(road_b)
    line(form + ": (b) three contexts in flight", bw)
    idx.set_search_gating(False)  # (b) again with every launch issued at once instead of when its predecessor starts to drain
    try:
        uw = timed(road_b)
    finally:
        idx.set_search_gating(True)
    line(form + ": (b) the same, search.gating off", uw)
    cw = timed(road_c)
    line(form + ": (c) launches of up to 32 batches", cw)
    qps = [N * NQ / (float(np.median(w)) * 1e-3) for w in (aw, bw, cw)]
    print("  answers of (b) equal (a)'s: %s, of (c): %s; queries/s (a) %.0f (b) %.0f (c) %.0f; (a) / (b) = %.3f, (a) / (c) = %.3f"
          % (b_out.same(a_out), c_out.same(a_out), qps[0], qps[1], qps[2], np.median(aw) / np.median(bw), np.median(aw) / np.median(cw)),
          flush=True)

# ---- G co-resident row-range shards: the per-probe calls of ShardedHNSWIndex in mode graph, before and after
if G > 1 and rows % (G * bench.CHUNK) == 0:
    del idx
    shards = [build(g * (rows // G), rows // G) for g in range(G)]
    for form, (blocking, predicate) in FORMS.items():
        before, after = [Out(1) for _ in range(G)], [Out(1) for _ in range(G)]
        pred = predicate(0)

        def road_before():
            for g, s in enumerate(shards):
                blocking(s, 0, before[g].ptrs(0))

        def road_after():
            for g, s in enumerate(shards):
                s.search_by_label_begin(0, d_Q[0].data_ptr(), NQ, K, EF, pred, *after[g].ptrs(0))
            for s in shards:
                s.search_end(0)

        bw, aw = timed(road_before), timed(road_after)
        line("%d shards, %s: before, shard after shard" % (G, form), bw)
        line("%d shards, %s: after, all begun then ended" % (G, form), aw)
        print("  answers equal: %s; before / after = %.3f" % (all(a.same(b) for a, b in zip(after, before)), np.median(bw) / np.median(aw)),
              flush=True)
else:
    print("shards skipped: %d rows do not split into %d shards of whole chunks" % (rows, G))
