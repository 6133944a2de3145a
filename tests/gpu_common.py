"""Helpers shared by the -m gpu parity tests and tools/gpu_diag.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import datagen  # noqa: E402
from oracle_lib import CpuIndex, load_oracle, parse_stream  # noqa: E402


def pkg():
    from __graft_entry__ import load_package
    return load_package()


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def make_data(n, dim, metric, seed, nq=64):
    norm = metric != "l2sq"
    X = datagen.mixture(n, dim, seed, normalize=norm)
    Q = datagen.mixture(nq, dim, seed + 1, n_clusters=max(2, int(np.sqrt(n))), normalize=norm)
    return X, Q


def oracle_index(dim, metric, M=16, M0=None, efc=128, efs=64):
    """The CPU mirror of the kernels: wave summation order + kernel candidate lists."""
    return CpuIndex(load_oracle(), dim, metric, M, M0, efc, efs, order=1, wave=1)


def gpu_index(dim, metric, M=16, M0=None, efc=128, efs=64):
    return pkg().GpuIndex(dim, metric, M, M0, efc, efs)


def first_graph_difference(blob_a, blob_b, ignore_counts=False):
    """Human-readable location of the first difference between two serialized graphs (or None).
    ignore_counts: skip the header's count_present / count_deleted, which usearch mis-reports once 64 slots were freed
    (ring_gt::size() == 0 when full)."""
    if blob_a == blob_b:
        return None
    a, b = parse_stream(blob_a), parse_stream(blob_b)
    if ignore_counts:
        ha, hb = bytearray(a["head"]), bytearray(b["head"])
        ha[17:33] = hb[17:33] = bytes(16)
        if ha != hb:
            return "stream header differs"
    elif a["head"] != b["head"]:
        return "stream header differs"
    if a["rows"] != b["rows"]:
        return "row count %d vs %d" % (a["rows"], b["rows"])
    if not np.array_equal(a["levels"], b["levels"]):
        i = int(np.nonzero(a["levels"] != b["levels"])[0][0])
        return "level of slot %d: %d vs %d" % (i, a["levels"][i], b["levels"][i])
    if (a["max_level"], a["entry"]) != (b["max_level"], b["entry"]):
        return "entry/max_level %s vs %s" % ((a["max_level"], a["entry"]), (b["max_level"], b["entry"]))
    if not np.array_equal(a["keys"], b["keys"]):
        i = int(np.nonzero(a["keys"] != b["keys"])[0][0])
        return "key of slot %d: %d vs %d" % (i, a["keys"][i], b["keys"][i])
    if a["vectors"] is not None and not np.array_equal(a["vectors"], b["vectors"]):
        return "vector payload differs"
    n_bad = 0
    first = None
    for s in range(a["rows"]):
        for l in range(len(a["adj"][s])):
            if not np.array_equal(a["adj"][s][l], b["adj"][s][l]):
                n_bad += 1
                if first is None:
                    first = "slot %d level %d: %s vs %s" % (s, l, a["adj"][s][l].tolist(), b["adj"][s][l].tolist())
    if not n_bad:
        return None if ignore_counts else "streams differ outside the parsed fields"
    return "%d lists differ; first: %s" % (n_bad, first)


class ExactReference:
    """The contract of the exact search as a brute force on the CPU: the wave-order f32 distance (orc_distance_wave) of every
    (query, live row) pair, sorted by (distance as f32, slot); top(k) = the first k keys, distances and the count, padded with
    -1 / +inf like the engine's output.  Reads nothing from the index under test.
    rows: the live rows (n x dim), keys / slots: theirs.  slots=None = the caller does not know them (slots re-used, rows
    reordered by compact): the order is then defined only where distances differ, and top(k) refuses a query whose first k + 1
    distances hold a tie."""

    def __init__(self, metric, rows, keys, slots, Q, kmax):
        lib = load_oracle()
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        n, dim = rows.shape
        self.tie_free_only = slots is None
        slots = np.arange(n) if slots is None else np.asarray(slots)
        keys = np.asarray(keys, dtype=np.int64)
        m = min(n, kmax + 1)
        self.n, self.kmax = n, kmax
        self.keys = np.full((len(Q), m), -1, dtype=np.int64)
        self.dist = np.full((len(Q), m), np.inf, dtype=np.float32)
        d = np.empty(n, dtype=np.float32)
        mi = {"l2sq": 0, "cosine": 1, "ip": 2}[metric]
        for i in range(len(Q)):
            if n:
                lib.orc_distance_wave_rows(mi, Q[i].ctypes.data, rows.ctypes.data, n, dim, d.ctypes.data)
            assert np.isfinite(d).all()
            order = np.lexsort((slots, d))[:m]  # by distance, then slot (floats compare by value: -0.0 ties with 0.0)
            self.keys[i], self.dist[i] = keys[order], d[order]

    def top(self, k, queries=None):
        assert k <= self.kmax
        sel = np.arange(len(self.keys)) if queries is None else np.asarray(queries)
        c = min(k, self.n)
        keys = np.full((len(sel), k), -1, dtype=np.int64)
        dist = np.full((len(sel), k), np.inf, dtype=np.float32)
        keys[:, :c], dist[:, :c] = self.keys[sel, :c], self.dist[sel, :c]
        if self.tie_free_only:
            head = self.dist[sel, :c + 1]
            assert np.all(head[:, 1:] > head[:, :-1]), "tied distances: this case needs the rows' slots"
        return keys, dist, np.full(len(sel), c, dtype=np.uint32)


def assert_exact_answer(got, ref, what=""):
    """keys, distance bits and counts of an exact search equal the reference's, every query and every cell."""
    (gk, gd, gc_), (rk, rd, rc) = got, ref
    bad_q = [i for i in range(len(rk)) if not (np.array_equal(gk[i], rk[i]) and gc_[i] == rc[i] and
                                                np.array_equal(gd[i].view(np.uint32), rd[i].view(np.uint32)))]
    if bad_q:
        i = bad_q[0]
        cells = np.nonzero((gk[i] != rk[i]) | (gd[i].view(np.uint32) != rd[i].view(np.uint32)))[0]
        j = int(cells[0]) if len(cells) else -1
        missed = np.mean([len(set(rk[q].tolist()) - set(gk[q].tolist())) / max(1, int(rc[q])) for q in range(len(rk))])
        raise AssertionError("%s: %d of %d queries differ from the brute force (share of the true top-k missing: %.3f); first: query %d "
                             "cell %d got (%d, %r) want (%d, %r), counts %d / %d"
                             % (what, len(bad_q), len(rk), missed, i, j, gk[i][j], float(gd[i][j]), rk[i][j], float(rd[i][j]),
                                int(gc_[i]), int(rc[i])))


def recall_at_k(got, truth):
    k = truth.shape[1]
    return float(np.mean([len(set(got[i].tolist()) & set(truth[i].tolist())) / k for i in range(len(truth))]))
