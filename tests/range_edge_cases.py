"""Inputs of the range search's edge tests: tests/test_gpu_range_edges.py sends them to the GPU, tests/test_range_edges_inputs.py
checks on the CPU, with the oracle alone, that they reach what they are meant to reach.  Nothing here touches a GPU: numpy,
gpu_common.ExactReference (orc_distance_wave over every live pair) and the helpers of the two existing range suites.

  (a) blocks_case     more than one query block x more than two row chunks, and a label group of more than a block of queries
  (b) full_tiles_case 128 x 128 and 32 x 256 tiles whose every pair survives
  (c) K_STEP_DIMS     dimensions of 1, 1, 1, 2, 3 and 5 K steps (and WIDE_DIM, 48)
  (d) MutationCase    one index through remove / add into freed slots / reserve + add / save + load / remove / compact
  (e) degenerate_case duplicates across tile boundaries, an all-zero row
"""
import functools
import os
import re

import numpy as np

import gpu_common as gc
from test_gpu_range_label_box import ABSENT, admitted_mask, radii_and_answer, reference
from test_gpu_range_search import expected, mixed_radii, unit


def header_constants():
    """RANGE_ROW_CHUNK and RANGE_QUERY_BLOCK as csrc/exact_range.h (shipped with the package) states them"""
    with open(os.path.join(gc.ROOT, "duckdb-vss_amd", "csrc", "exact_range.h")) as f:
        text = f.read()
    found = {name: re.search(r"\b%s\s*=\s*(\d+)\b" % name, text) for name in ("RANGE_ROW_CHUNK", "RANGE_QUERY_BLOCK")}
    assert all(found.values()), found
    return int(found["RANGE_ROW_CHUNK"].group(1)), int(found["RANGE_QUERY_BLOCK"].group(1))


CHUNK, BLOCK = header_constants()


def k_steps(dim):
    """K steps of the candidate tiles: 32 floats = eight float4 chunks a step"""
    return -(-(-(-dim // 4)) // 8)


K_STEP_DIMS = [3, 20, 32, 33, 96, 160]
WIDE_DIM = 1536


def prefix(want, n):
    """the answer of the first n queries of a batch"""
    return want[0][:n + 1], want[1][:n]


# ------------------------------------------------------------------------------------------------ (a) query blocks x row chunks
A_DIM, A_ROWS, A_NQ, A_TENANT0_QUERIES = 16, 2 * CHUNK + 5, 2 * BLOCK + 3, BLOCK + 76


class BlocksCase:
    """X, keys (= row ids, so that the label form runs on the same index), the live mask build() leaves, Q, the reference over
    the live rows, the mixed radii and their answer; and the label form: tenant (column 0, 32 bits), lo / hi, the admitted
    live rows per query nearest first, radii and answer."""

    def __init__(self, metric):
        rng = np.random.default_rng(1600 + len(metric))
        X = rng.standard_normal((A_ROWS, A_DIM)).astype(np.float32)
        Q = rng.standard_normal((A_NQ, A_DIM)).astype(np.float32)
        if metric != "l2sq":
            X, Q = unit(X), unit(Q)
        self.metric, self.X, self.Q = metric, X, Q
        self.keys = np.arange(A_ROWS, dtype=np.int64)
        self.live = self.keys % 10 != 3  # test_gpu_range_search.build
        self.ref = gc.ExactReference(metric, X[self.live], self.keys[self.live], None, Q, A_ROWS)
        self.radii = mixed_radii(self.ref, A_NQ)
        self.want = expected(self.ref, self.radii)
        # the label form: tenant 0 owns all live rows but 40; BLOCK + 76 queries on it, the rest interleaved with them
        self.tenant = np.zeros(A_ROWS, np.uint32)
        self.tenant[rng.permutation(self.keys[self.live])[:40]] = np.repeat([2, 3], [31, 9])
        rest = A_NQ - A_TENANT0_QUERIES
        self.kind = rng.permutation(np.repeat(np.arange(5), [A_TENANT0_QUERIES, rest // 4, rest // 4, rest // 4, rest - 3 * (rest // 4)]))
        t_of = np.array([0, 2, 3, 0, ABSENT], np.uint64)[self.kind]
        self.lo, self.hi = t_of[:, None].copy(), t_of[:, None].copy()
        self.lo[self.kind == 3], self.hi[self.kind == 3] = 9, 8  # the empty box
        self.near = reference(self.ref, admitted_mask([self.tenant], [0], self.lo, self.hi))
        self.box_radii, self.box_want = radii_and_answer(self.near)


@functools.lru_cache(maxsize=1)
def blocks_case(metric):
    return BlocksCase(metric)


# ------------------------------------------------------------------------------------------------ (b) full tiles
B_DIM, B_ROWS, B_NQ, B_CORNERS = 96, 256, 256, [0, 127, 128, 255]


class FullTilesCase:
    """256 rows, none removed, keys against slot order; every radius +inf.  Label form: one 32-bit column (row id % 7, set from
    the smallest key on) that both boxes [0, 100] (128 queries) and [0, 200] (32 queries) admit in full."""

    def __init__(self, metric):
        rng = np.random.default_rng(9600 + len(metric))
        self.metric = metric
        self.X, self.Q = unit(rng.standard_normal((B_ROWS, B_DIM))), unit(rng.standard_normal((B_NQ, B_DIM)))
        self.keys = 1_000_000 - np.arange(B_ROWS, dtype=np.int64)
        self.radii = np.full(B_NQ, np.inf, np.float32)
        self.first_rowid = int(self.keys.min())
        self.labels = ((self.first_rowid + np.arange(B_ROWS)) % 7).astype(np.uint32)  # by row id, from first_rowid on
        self.box_nq = 128 + 32
        self.lo = np.zeros((self.box_nq, 1), np.uint64)
        self.hi = np.repeat([100, 200], [128, 32]).astype(np.uint64)[:, None]

    def answers(self, live):
        """(the plain answer over all queries, the label form's over the first 160) with the rows of `live` (a mask by slot)"""
        ref = gc.ExactReference(self.metric, self.X[live], self.keys[live], None, self.Q, B_ROWS)
        return expected(ref, self.radii), expected(ref, self.radii[:self.box_nq])


@functools.lru_cache(maxsize=2)
def full_tiles_case(metric):
    return FullTilesCase(metric)


# ------------------------------------------------------------------------------------------------ (d) mutations
D_DIM, D_ROWS, D_NQ = 20, 3000, 16


class MutationCase:
    """The sequence of test_row_norm_cache_across_mutations with data that makes a stale |x|^2 DROP matching rows: the rows
    removed first are large (l2sq: scaled by 30) or ordinary (cosine: unit), the arrivals that take their slots are copies of
    the queries plus 1e-3 N(0, 1) (cosine: scaled by 0.02 on top) — |x|^2 smaller by a factor of 100 and more, so that with the
    removed row's cached |x|^2 the arrival's score lies far above theta, the tile drops it and the re-score never sees it.
    steps() yields (name, keys removed, (keys, rows) added); the test applies each to its index, the dict `rows` follows."""

    def __init__(self, metric):
        rng = np.random.default_rng(4000 + len(metric))
        n, dim = D_ROWS, D_DIM
        self.metric = metric
        X = rng.standard_normal((n, dim)).astype(np.float32)
        Q = rng.standard_normal((D_NQ, dim)).astype(np.float32)
        if metric == "cosine":
            X, Q = unit(X), unit(Q)
        self.gone = np.sort(rng.choice(n, 100, replace=False)).astype(np.int64)
        if metric == "l2sq":
            X[self.gone] *= np.float32(30)
        self.X, self.Q = X, Q
        self.arrivals = (Q[np.arange(100) % D_NQ] + 1e-3 * rng.standard_normal((100, dim))).astype(np.float32)
        if metric == "cosine":
            self.arrivals *= np.float32(0.02)
        self.more = (0.05 * rng.standard_normal((300, dim))).astype(np.float32)
        self.more[123] = unit(self.more[123]) * np.float32(2 * np.linalg.norm(X, axis=1).max())  # a norm above every one before
        self.drop = np.array([i for i in range(50) if i not in set(self.gone.tolist())], dtype=np.int64)
        self.label_rows = n + 400
        ids = np.arange(self.label_rows, dtype=np.uint64)
        self.column0, self.column1 = (ids % 3).astype(np.uint32), ids << np.uint64(33)
        q3 = (np.arange(D_NQ, dtype=np.uint64) % 3)[:, None]
        self.lo = np.concatenate([q3, np.zeros((D_NQ, 1), np.uint64)], axis=1)
        self.hi = np.concatenate([q3, np.full((D_NQ, 1), 0xFFFFFFFFFFFFFFFF, np.uint64)], axis=1)

    def steps(self):
        n = D_ROWS
        none = np.zeros(0, np.int64)
        yield "build", none, (np.arange(n, dtype=np.int64), self.X)
        yield "remove", self.gone, None
        yield "add into freed slots", none, (np.arange(n, n + 100, dtype=np.int64), self.arrivals)
        yield "reserve and add past the end", none, (np.arange(n + 100, n + 400, dtype=np.int64), self.more)
        yield "save and load", none, None
        yield "remove again", self.drop, None
        yield "compact", none, None

    @staticmethod
    def follow(rows, removed, added):
        for i in removed:
            del rows[int(i)]
        if added is not None:
            rows.update({int(k): v for k, v in zip(*added)})

    def answers(self, rows):
        """radii = the bits of the 3rd-nearest live (admitted) distance; returns (radii, answer) of the plain call and of the
        call under the boxes column 0 == q % 3 and column 1 >= 0"""
        ks = np.array(sorted(rows), dtype=np.int64)
        ref = gc.ExactReference(self.metric, np.stack([rows[int(i)] for i in ks]), ks, None, self.Q, len(ks))
        radii = ref.dist[:, 2].copy()
        near = reference(ref, admitted_mask([self.column0, self.column1], [0, 1], self.lo, self.hi))
        box_radii = np.array([d[2] for _, d in near], np.float32)
        cells = []
        for (ids, d), r in zip(near, box_radii):
            order = np.argsort(ids[d <= r], kind="stable")
            cells.append((ids[d <= r][order], d[d <= r][order]))
        offsets = np.concatenate([[0], np.cumsum([len(k) for k, _ in cells])]).astype(np.uint64)
        return (radii, expected(ref, radii)), (box_radii, (offsets, cells))


# ------------------------------------------------------------------------------------------------ (e) degenerate inputs
E_DIM, E_ROWS, E_NQ = 20, 300, 8
E_ZERO_ROW = 17
# rows i, i + 128 and i + 256 are copies — three tiles of 128 — and none of the three is one build() removes (slot % 10 == 3)
E_DUPLICATED = np.array([i for i in range(44) if i % 10 not in (3, 5, 7) and i != E_ZERO_ROW][:20])


def degenerate_data(metric, what):
    """what: 'duplicates' or 'zero row'.  Returns X, Q, keys (= row ids) and the live mask that build() leaves"""
    rng = np.random.default_rng(500 + len(metric) + len(what))
    X = rng.standard_normal((E_ROWS, E_DIM)).astype(np.float32)
    Q = rng.standard_normal((E_NQ, E_DIM)).astype(np.float32)
    if metric != "l2sq":
        X, Q = unit(X), unit(Q)
    if what == "duplicates":
        X[E_DUPLICATED + 128] = X[E_DUPLICATED]
        X[E_DUPLICATED + 256] = X[E_DUPLICATED]
    else:
        X[E_ZERO_ROW] = 0
    keys = np.arange(E_ROWS, dtype=np.int64)
    return X, Q, keys, keys % 10 != 3


def duplicate_rounds(ref):
    """three batches of radii: query q of round t takes the bits of its distance to triple (8 t + q) % 20.  Yields
    (the triple's three row ids per query, radii at the distance, radii one f32 below)"""
    for t in range(3):
        first = E_DUPLICATED[(E_NQ * t + np.arange(E_NQ)) % len(E_DUPLICATED)]
        at = np.array([ref.dist[q][ref.keys[q] == first[q]][0] for q in range(E_NQ)], np.float32)
        yield np.stack([first, first + 128, first + 256], axis=1), at, np.nextafter(at, np.float32(-np.inf))
