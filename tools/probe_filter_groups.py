"""Per-query predicates in one launch (vss_search_batch_filtered_groups) against one vss_search_batch_filtered call per
predicate, and the cost of the feature to the calls that were there before it.
The benchmark's mixture (1M x 128 l2sq by default), the reference's default index options (M 16, ef_construction 128), k 10, ef 64:
  1. ONE vss_search_batch_filtered of 1024 queries under a 0.5 bitmap, five launches after a warm-up: kernel ms (vss_timing) and
     host-pointer wall time.  Run the same script from a checkout of the parent commit with its own library to compare; a
     library without the grouped call stops here.
  2. tenants: 1024 queries in 16 equal groups whose bitmaps admit 1/16 of the rows each, and 204 queries in 4 such groups — one
     grouped call against one filtered call per group over that group's queries (what a caller had to do before), both as
     host-pointer wall time and as summed kernel ms, median of five; the answers of both must be identical.
  3. eight join chunks of 204 queries, each with its own table of 4 tenants: ONE vss_search_multi_filtered_device_begin + _end
     against eight blocking vss_search_batch_filtered_groups_device calls.
  4. three 1024-query batches under one bitmap each: three contexts in flight (vss_search_batch_filtered_device_begin) against
     three blocking vss_search_batch_filtered_device calls.
     Legs 3 and 4 alternate their two sides in this process, five repetitions after a warm-up, host clock between
     synchronisations; identical answers required.  A library without these calls stops after leg 2.
    python tools/probe_filter_groups.py [rows [dim [metric [ef]]]]"""
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
EF = int(sys.argv[4]) if len(sys.argv) > 4 else 64
M, M0, EFC, K, REPEATS = 16, 32, 128, 10, 5
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
words = (rows + 63) // 64
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
    print("%-58s wall ms %s  median %7.3f spread %6.3f | kernel ms %s  median %7.3f spread %6.3f"
          % (name, " ".join("%.3f" % v for v in wall), float(np.median(wall)), max(wall) - min(wall),
             " ".join("%.3f" % v for v in kern), float(np.median(kern)), max(kern) - min(kern)), flush=True)


# ---- 1. what was there before: one bitmap for the whole batch
half = bitmap_of(rng.random(rows) < 0.5)
wall, kern = [], []
for r in range(REPEATS + 1):  # (the first one warms up: scratch allocations)
    w, k_ms, out = timed(lambda: idx.search_batch_filtered(Q, K, EF, half, rows))
    wall.append(w), kern.append(k_ms)
st = idx.last_search_stats()
line("filtered, 1024 queries, 0.5 bitmap", wall[1:], kern[1:])
print("  distances %d expansions %d re-run queries %d; checksum of the row ids %d" % (int(st[0]), int(st[1]), int(st[3]),
                                                                                   int(out[0].sum())), flush=True)
if not hasattr(idx, "search_batch_filtered_groups"):
    print("this library has no grouped call: done")
    sys.exit(0)

# ---- 2. what the feature buys: tenants
tenant = rng.integers(0, 16, size=rows)
bad = 0
for nq, n_groups in ((1024, 16), (204, 4)):
    tables = np.stack([bitmap_of(tenant == g) for g in range(n_groups)])  # 1/16 of the rows each
    group_of = (np.arange(nq) % n_groups).astype(np.uint32)
    q = np.ascontiguousarray(Q[:nq])
    per_group_q = [np.ascontiguousarray(q[group_of == g]) for g in range(n_groups)]

    def one_call():
        return idx.search_batch_filtered_groups(q, K, EF, tables, rows, group_of)

    def call_per_group():
        total = 0.0
        outs = []
        for g in range(n_groups):
            outs.append(idx.search_batch_filtered(per_group_q[g], K, EF, tables[g], rows))
            total += idx.timing()["search_kernel_ms"]
        return total, outs

    gw, gk, pw, pk = [], [], [], []
    for r in range(REPEATS + 1):
        w, k_ms, grouped = timed(one_call)
        gw.append(w), gk.append(k_ms)
        reruns = int(idx.last_search_stats()[3])
        t = time.perf_counter()
        k_ms, outs = call_per_group()
        pw.append((time.perf_counter() - t) * 1e3), pk.append(k_ms)
    same = True
    for g in range(n_groups):
        at = np.nonzero(group_of == g)[0]
        same = same and np.array_equal(grouped[0][at], outs[g][0]) and np.array_equal(grouped[2][at], outs[g][2])
        same = same and np.array_equal(grouped[1][at].view(np.uint32), outs[g][1].view(np.uint32))
    bad += not same
    line("%d queries, %d tenants of 1/16: ONE grouped call" % (nq, n_groups), gw[1:], gk[1:])
    line("%d queries, %d tenants of 1/16: %d filtered calls" % (nq, n_groups, n_groups), pw[1:], pk[1:])
    print("  wall: grouped / per-group = %.3f; kernel: %.3f; re-run queries of the grouped call %d; full answers %d of %d; identical %s"
          % (np.median(gw[1:]) / np.median(pw[1:]), np.median(gk[1:]) / np.median(pk[1:]), reruns,
             int((grouped[2] == K).sum()), nq, same), flush=True)
if not hasattr(idx, "search_multi_filtered_begin"):
    print("this library has no pipelined filtered calls: done\nDIFFERENCES: %d" % bad)
    sys.exit(1 if bad else 0)

# ---- 3. / 4. the pipelined and multi-batch forms against the sequence of blocking device calls they replace.  Device pointers on
# both sides, the two sides alternating in this process; every timed call returns with the device idle (vss_search_batch_end and
# the blocking calls synchronise), so the host clock around it, taken after a torch.cuda.synchronize(), measures it whole.


def to_dev(a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).to(dev)


def cells(nq):
    return (torch.empty((nq, K), dtype=torch.int64, device=dev), torch.empty((nq, K), dtype=torch.float32, device=dev),
            torch.empty(nq, dtype=torch.int32, device=dev))


def alternate(new_side, old_side):
    """[(wall ms, kernel ms)] of both sides, REPEATS each after one warm-up, new / old / new / old ..."""
    new, old = [], []
    for r in range(REPEATS + 1):
        for side, into in ((new_side, new), (old_side, old)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            k_ms = side()
            into.append(((time.perf_counter() - t) * 1e3, k_ms))
    return new[1:], old[1:]


def report(what, new_name, old_name, new, old, same):
    line("%s: %s" % (what, new_name), [w for w, _ in new], [k for _, k in new])
    line("%s: %s" % (what, old_name), [w for w, _ in old], [k for _, k in old])
    print("  wall: new / blocking = %.3f; kernel: %.3f; identical %s" % (
        np.median([w for w, _ in new]) / np.median([w for w, _ in old]),
        np.median([k for _, k in new]) / np.median([k for _, k in old]), same), flush=True)


def equal(a, b):
    return all(bool(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y))
               for x, y in zip(a, b))


# 3. eight join chunks of 204 queries, each chunk with its own table of 4 tenants (of 16): one launch against eight
CHUNKS, PER = 8, 204
Q3 = gen.rows(bench.QUERY_SEED, 1, CHUNKS * PER).contiguous()
d_q3 = [Q3[c * PER:(c + 1) * PER].contiguous() for c in range(CHUNKS)]
d_tables = [to_dev(np.stack([bitmap_of(tenant == (2 * c + j) % 16) for j in range(4)])) for c in range(CHUNKS)]
d_groups = [to_dev(((np.arange(PER) + c) % 4).astype(np.uint32)) for c in range(CHUNKS)]
out_new, out_old = [cells(PER) for _ in range(CHUNKS)], [cells(PER) for _ in range(CHUNKS)]
torch.cuda.synchronize()


def multi_launch():
    idx.search_multi_filtered_begin(1, [t.data_ptr() for t in d_q3], PER, K, EF, [t.data_ptr() for t in d_tables], [4] * CHUNKS, rows,
                                    [t.data_ptr() for t in d_groups], [o[0].data_ptr() for o in out_new],
                                    [o[1].data_ptr() for o in out_new], [o[2].data_ptr() for o in out_new])
    idx.search_end(1)
    return idx.timing()["search_kernel_ms"]


def eight_blocking():
    total = 0.0
    for c in range(CHUNKS):
        idx.search_batch_filtered_groups_device(d_q3[c].data_ptr(), PER, K, EF, d_tables[c].data_ptr(), 4, rows, d_groups[c].data_ptr(),
                                                *[t.data_ptr() for t in out_old[c]])
        total += idx.timing()["search_kernel_ms"]
    return total


new, old = alternate(multi_launch, eight_blocking)
same = all(equal(a, b) for a, b in zip(out_new, out_old))
bad += not same
report("8 chunks x 204 queries, 4 tenants each", "ONE multi-batch launch", "8 blocking grouped calls", new, old, same)

# 4. three 1024-query batches, one bitmap each: three contexts in flight against three blocking calls
d_q4 = [to_dev(Q) for _ in range(3)]
d_bitmaps = [to_dev(half), to_dev(~half), to_dev(bitmap_of(rng.random(rows) < 0.1))]
out_new, out_old = [cells(1024) for _ in range(3)], [cells(1024) for _ in range(3)]
torch.cuda.synchronize()


def three_in_flight():
    for c in range(3):
        idx.search_filtered_begin(c, d_q4[c].data_ptr(), 1024, K, EF, d_bitmaps[c].data_ptr(), rows, *[t.data_ptr() for t in out_new[c]])
    total = 0.0
    for c in range(3):
        idx.search_end(c)
        total += idx.timing()["search_kernel_ms"]
    return total


def three_blocking():
    total = 0.0
    for c in range(3):
        idx._check(idx.lib.vss_search_batch_filtered_device(idx.h, d_q4[c].data_ptr(), 1024, K, EF, d_bitmaps[c].data_ptr(), rows,
                                                            *[t.data_ptr() for t in out_old[c]]))
        total += idx.timing()["search_kernel_ms"]
    return total


new, old = alternate(three_in_flight, three_blocking)
same = all(equal(a, b) for a, b in zip(out_new, out_old))
bad += not same
report("3 batches x 1024 queries, one bitmap each", "three contexts in flight", "3 blocking filtered calls", new, old, same)
print("  (kernel ms of launches in flight together overlap: their sum is not the elapsed time; compare the wall times)")
print("DIFFERENCES: %d" % bad)
sys.exit(1 if bad else 0)
