"""-m gpu: the contract of the exact search (vss_search_exact_batch*) on data chosen against its mechanism.

Contract, for finite inputs: the answer is the brute force of the engine's own wave-order f32 metric over the live rows, ordered
by (distance, slot) — keys, distance bits and counts, every query, every cell, ties included.  The reference is
gpu_common.ExactReference (orc_distance_wave over every pair on the CPU); it reads nothing from the index under test.

The engine SELECTS rows by an MFMA ranking score (|x|^2 - 2 q.x, -q.x / |x|, -q.x) and re-scores only the K' = k + 8 survivors.
The cases below are where a score's rounding error exceeds the distance gap between the k-th and the K'-th neighbour — a large
common offset under l2sq (the score cancels catastrophically, the metric does not), groups of near-duplicates larger than K',
bit-identical duplicates — and the plain indexing edges: tiles of 128 rows / queries, chunks of 32768 rows, the folded select,
k against the live rows, tombstones, the cached row norms across mutations.
"""
import numpy as np
import pytest

import gpu_common as gc

pytestmark = pytest.mark.gpu

CHUNK, TILE = 32768, 128


def build(dim, metric, X, keys=None, capacity=None):
    """A cheap graph (only the exact path is under test); slot of row i = i, key of slot s = keys[s]."""
    gpu = gc.gpu_index(dim, metric, 8, 16, 16)
    gpu.reserve(capacity or len(X))
    gpu.set_build_params(32768, 4)
    gpu.add(np.arange(len(X)) if keys is None else keys, X)
    return gpu


def keys_against_slot_order(n):
    """keys that DESCEND with the slot: an answer ordered by (distance, key) instead of (distance, slot) is caught"""
    return 1_000_000 - np.arange(n, dtype=np.int64)


def unit(a):
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------------------------------- (a) a large common offset
@pytest.mark.parametrize("cnorm", [2048.0, 8192.0])
@pytest.mark.parametrize("dim", [64, 100])  # 64: the LDS-DMA tile (k_exact_scores_v4); 100: the register-staged one (_v3)
def test_offset_l2sq(dim, cnorm):
    """rows = c + N(0, 1) with |c| = 2048 / 8192: |x|^2 ~ 4e6 / 7e7 carries an f32 rounding error of 0.25-0.5 / 4-8, the
    squared distances are ~2 dim with gaps of a few units between the 10th and the 18th neighbour.  (A CPU model of the
    selection by score loses 0.65-0.70 of the true top-10 at |c| = 8192 and none at 2048.)"""
    rng = np.random.default_rng(1000 + dim + int(cnorm))
    n = 3000
    c = unit(rng.standard_normal(dim)) * np.float32(cnorm)
    X = (c + rng.standard_normal((n, dim))).astype(np.float32)
    Q = (c + rng.standard_normal((8, dim))).astype(np.float32)
    keys = keys_against_slot_order(n)
    ref = gc.ExactReference("l2sq", X, keys, np.arange(n), Q, 50)
    gpu = build(dim, "l2sq", X, keys)
    for k in (1, 10, 50):
        got = gpu.search_batch(Q, k, exact=True)
        print("offset %g dim %d k %d: %d of %d queries redone" % (cnorm, dim, k, gpu.last_exact_fallbacks(), len(Q)))
        gc.assert_exact_answer(got, ref.top(k), "offset %g dim %d k %d" % (cnorm, dim, k))


# ------------------------------------------------------------------------------------------------- (b) near-duplicate groups
@pytest.mark.parametrize("dim", [64, 100])
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_near_duplicate_groups(metric, dim):
    """4 groups of 60 rows = unit vector + 1e-4 N(0, 1) among 2000 unit rows, shuffled over the slots; queries = other
    perturbations of the groups' bases.  Inside a group the distances differ by ~1e-7 (l2sq: |q - x|^2 ~ 2 dim 1e-8; cosine
    likewise), the scores' rounding error is ~1e-7 per unit of |q| |x|: their order inside the group is noise, and the group is
    larger than K' at k = 10 and 40.  k = 70 spans the group and the background.  (CPU model of the selection by score: 0.18-0.43
    of the true top-10 lost under l2sq and cosine, none under ip, whose distances 1 - q.x differ by ~1e-4 inside a group.)
    Under l2sq and cosine no error bound of an f32 score can separate the group's rows, so k = 10 and 40 must be redone."""
    rng = np.random.default_rng(2000 + dim)
    bases = unit(rng.standard_normal((4, dim)))
    groups = np.concatenate([b + 1e-4 * rng.standard_normal((60, dim)) for b in bases]).astype(np.float32)
    X = np.concatenate([unit(rng.standard_normal((2000, dim))), groups])
    X = np.ascontiguousarray(X[rng.permutation(len(X))])
    Q = np.concatenate([b + 1e-4 * rng.standard_normal((2, dim)) for b in bases]).astype(np.float32)
    n = len(X)
    keys = keys_against_slot_order(n)
    ref = gc.ExactReference(metric, X, keys, np.arange(n), Q, 70)
    gpu = build(dim, metric, X, keys)
    for k in (10, 40, 70):
        got = gpu.search_batch(Q, k, exact=True)
        redone = gpu.last_exact_fallbacks()
        print("groups %s dim %d k %d: %d of %d queries redone" % (metric, dim, k, redone, len(Q)))
        gc.assert_exact_answer(got, ref.top(k), "groups %s dim %d k %d" % (metric, dim, k))
        if metric != "ip" and k < 60:
            assert redone > 0


# ------------------------------------------------------------------------------------------------- (c) bit-identical duplicates
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_identical_duplicates_come_back_in_slot_order(metric):
    """50 copies of one row, each in another 128-row tile; the keys descend with the slots.  Every copy has the same distance
    bits to every query: the lowest SLOTS come back, in slot order (k_exact_rerank)."""
    rng = np.random.default_rng(3000)
    n, dim = 8000, 16
    X = rng.standard_normal((n, dim)).astype(np.float32)
    if metric != "l2sq":
        X = unit(X)
    twins = 7 + 150 * np.arange(50)
    assert len(set(twins // TILE)) == 50 and twins.max() < n
    X[twins] = X[twins[0]]
    Q = np.concatenate([X[twins[:1]], X[twins[:1]] + np.float32(0.01) * rng.standard_normal((2, dim)).astype(np.float32),
                        rng.standard_normal((3, dim)).astype(np.float32)]).astype(np.float32)
    keys = keys_against_slot_order(n)
    ref = gc.ExactReference(metric, X, keys, np.arange(n), Q, 45)
    gpu = build(dim, metric, X, keys)
    for k in (10, 45):
        got = gpu.search_batch(Q, k, exact=True)
        gc.assert_exact_answer(got, ref.top(k), "twins %s k %d" % (metric, k))
        for q in range(3):  # (the queries at and next to the copies: nothing is nearer than a copy)
            assert np.array_equal(got[0][q], keys[twins[:k]])


# ------------------------------------------------------------------------------------------------- (d) chunks and the folded select
def _many_chunk_data(construction, dim):
    rng = np.random.default_rng(4000 + dim)
    n = 70_000
    if construction == "offset":
        c = unit(rng.standard_normal(dim)) * np.float32(8192.0)
        X = (c + rng.standard_normal((n, dim))).astype(np.float32)
        Q = (c + rng.standard_normal((6, dim))).astype(np.float32)
    else:
        X = rng.standard_normal((n, dim)).astype(np.float32)
        twins = 5 + 1399 * np.arange(50)  # in every one of the three 32768-row chunks, each in a tile of its own
        assert set(twins // CHUNK) == {0, 1, 2} and len(set(twins // TILE)) == 50 and twins.max() < n
        X[twins] = X[twins[0]]
        Q = np.concatenate([X[twins[:1]], X[twins[:1]] + np.float32(0.01) * rng.standard_normal((1, dim)).astype(np.float32),
                            rng.standard_normal((4, dim)).astype(np.float32)]).astype(np.float32)
    return X, Q


@pytest.mark.parametrize("dim", [32, 24])  # 32: k_exact_scores_v4 by default; 24: the register-staged _v3
@pytest.mark.parametrize("construction", ["offset", "twins"])
def test_many_chunks_every_kernel_and_select(construction, dim, monkeypatch):
    """70 000 rows = three chunks: the first is selected the plain way, the rest through the select folded into the tile's
    epilogue (k = 10, 200) or plainly (VSS_EXACT_FILTER=0; k = 300, where 8 K' exceeds the survivor buffer).  Every variant —
    VSS_EXACT_FILTER 0 / 1 x VSS_EXACT_KERNEL 2 / 4 / 5, and every query redone in the metric (VSS_EXACT_CERTIFY=2) — gives the
    reference's bits."""
    X, Q = _many_chunk_data(construction, dim)
    n = len(X)
    keys = keys_against_slot_order(n)
    ref = gc.ExactReference("l2sq", X, keys, np.arange(n), Q, 300)
    first = build(dim, "l2sq", X, keys)
    blob = first.save()
    first.close()
    variants = [dict(VSS_EXACT_FILTER=f, VSS_EXACT_KERNEL=kern) for f in "01" for kern in "245"]
    variants.append(dict(VSS_EXACT_CERTIFY="2"))
    for env in variants:
        for name in ("VSS_EXACT_FILTER", "VSS_EXACT_KERNEL", "VSS_EXACT_CERTIFY"):
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        gpu = gc.gpu_index(dim, "l2sq", 8, 16, 16)  # (the knobs are read when the index is created)
        gpu.load(blob)
        for k in (10, 200, 300):
            got = gpu.search_batch(Q, k, exact=True)
            gc.assert_exact_answer(got, ref.top(k), "%s dim %d k %d %r" % (construction, dim, k, env))
        gpu.close()


@pytest.mark.parametrize("qt", [None, 3])
@pytest.mark.parametrize("dim", [20, 768])  # 20: 8 lanes per row, 8 rows side by side, a ragged last chunk; 768: the whole wave per row
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_every_query_redone_in_the_metric(metric, dim, qt, monkeypatch):
    """The redo path (k_exact_metric_scores, every metric's instantiation) on its own: VSS_EXACT_CERTIFY=2 answers every query
    again with the metric as the score — plain data with tombstones, 11 queries (tiles of 8 + 3; of 3 + 3 + 3 + 2 with
    VSS_EXACT_REDO_QT=3, the tiles of rows too wide for eight queries in LDS).  All 11 are counted as redone, and the answer is
    the reference's."""
    n, nq = 3000, 11
    X, Q = gc.make_data(n, dim, metric, 4500 + dim, nq=nq)
    keys = keys_against_slot_order(n)
    dead = np.array([0, 1, 63, 64, 1500, n - 1])
    live = np.setdiff1d(np.arange(n), dead)
    ref = gc.ExactReference(metric, X[live], keys[live], live, Q, 70)
    monkeypatch.setenv("VSS_EXACT_CERTIFY", "2")
    if qt:
        monkeypatch.setenv("VSS_EXACT_REDO_QT", str(qt))
    else:
        monkeypatch.delenv("VSS_EXACT_REDO_QT", raising=False)
    gpu = build(dim, metric, X, keys)
    assert gpu.remove(keys[dead]) == len(dead)
    for k in (10, 70):
        got = gpu.search_batch(Q, k, exact=True)
        assert gpu.last_exact_fallbacks() == nq
        gc.assert_exact_answer(got, ref.top(k), "redo %s dim %d qt %s k %d" % (metric, dim, qt, k))


# ------------------------------------------------------------------------------------------------- (e) shape edges
def _plain(n, dim, seed, nq):
    return gc.make_data(n, dim, "l2sq", seed, nq=nq)


@pytest.mark.parametrize("n", [127, 128, 129, 32767, 32768, 32769, 65537])
def test_row_and_query_counts_at_tile_and_chunk_edges(n):
    """Plain mixture data (no rounding trouble: nothing may be redone), row counts around one tile and around one and two
    chunks, query counts around one query tile.  The whole batch runs; a strided subset of at most 8 queries is compared."""
    dim, k = 16, 10
    X, Qall = _plain(n, dim, 5000 + n, 129)
    keys = keys_against_slot_order(n)
    gpu = build(dim, "l2sq", X, keys)
    for nq in (1, 127, 128, 129):
        Q = Qall[:nq]
        pick = np.unique(np.linspace(0, nq - 1, min(nq, 8)).astype(int))
        ref = gc.ExactReference("l2sq", X, keys, np.arange(n), Q[pick], k)
        gk, gd, gcnt = gpu.search_batch(Q, k, exact=True)
        assert gpu.last_exact_fallbacks() == 0
        gc.assert_exact_answer((gk[pick], gd[pick], gcnt[pick]), ref.top(k), "%d rows %d queries" % (n, nq))
        assert np.all(gcnt == min(k, n)) and np.all(gk[:, :min(k, n)] >= 0)


def test_k_against_the_live_rows():
    """k above the live rows: count < k and a tail of -1 / +inf; k = 4088 (the largest) on 4100 rows; k = 4089 is refused with
    the documented message and the index answers afterwards as before."""
    dim = 16
    X, Q = _plain(4100, dim, 5100, 5)
    keys = keys_against_slot_order(len(X))
    small = build(dim, "l2sq", X[:50], keys[:50])
    ref = gc.ExactReference("l2sq", X[:50], keys[:50], np.arange(50), Q, 64)
    got = small.search_batch(Q, 64, exact=True)
    gc.assert_exact_answer(got, ref.top(64), "50 rows k 64")
    assert np.all(got[2] == 50) and np.all(got[0][:, 50:] == -1) and np.all(np.isposinf(got[1][:, 50:]))
    gpu = build(dim, "l2sq", X, keys)
    ref = gc.ExactReference("l2sq", X, keys, np.arange(len(X)), Q, 4088)
    gc.assert_exact_answer(gpu.search_batch(Q, 4088, exact=True), ref.top(4088), "4100 rows k 4088")
    with pytest.raises(gc.pkg().VssError, match="exact search supports k <= 4088"):
        gpu.search_batch(Q, 4089, exact=True)
    gc.assert_exact_answer(gpu.search_batch(Q, 10, exact=True), ref.top(10), "after the refused call")
    assert gpu.last_exact_fallbacks() == 0


def test_tombstones_at_tile_and_chunk_edges():
    """Tombstones on the first and the last row of a tile and of a chunk, each the nearest row of a query before it was
    removed; then every row but three removed."""
    dim, n = 16, 33_000
    X, _ = _plain(n, dim, 5200, 1)
    keys = keys_against_slot_order(n)
    dead = np.array([0, TILE - 1, TILE, 2 * TILE - 1, CHUNK - 1, CHUNK, n - 1])
    Q = np.ascontiguousarray(X[dead])
    gpu = build(dim, "l2sq", X, keys)
    before = gpu.search_batch(Q, 1, exact=True)
    assert np.array_equal(before[0][:, 0], keys[dead])
    assert gpu.remove(keys[dead]) == len(dead)
    live = np.setdiff1d(np.arange(n), dead)
    ref = gc.ExactReference("l2sq", X[live], keys[live], live, Q, 10)
    got = gpu.search_batch(Q, 10, exact=True)
    gc.assert_exact_answer(got, ref.top(10), "tombstones at the edges")
    assert not np.isin(got[0], keys[dead]).any() and gpu.last_exact_fallbacks() == 0
    gpu.close()
    m = 300
    gpu = build(dim, "l2sq", X[:m], keys[:m])
    left = np.array([0, 131, m - 1])
    assert gpu.remove(np.delete(keys[:m], left)) == m - 3
    ref = gc.ExactReference("l2sq", X[left], keys[left], left, Q, 10)
    got = gpu.search_batch(Q, 10, exact=True)
    gc.assert_exact_answer(got, ref.top(10), "three live rows")
    assert np.all(got[2] == 3)


# ------------------------------------------------------------------------------------------------- (f) the cached row norms
@pytest.mark.parametrize("metric", ["l2sq", "cosine"])
def test_row_norm_cache_across_mutations(metric):
    """The score tiles read |x|^2 from a cache that is refreshed when the index has changed (norms_valid_for != mutations).  One
    index through build / remove / add into the freed slots / add past a reallocating reserve / save + load / compact, an exact
    search after each: the answer is the reference over the rows live at that moment.  The rows that arrive have 30 times the
    norm of the rows they replace: with a stale |x|^2 their l2sq scores would fall far below every honest one and fill the kept set.
    (Slots are not known to the test once they have been re-used or reordered: continuous data, and the reference refuses a
    query with a tie among its first k + 1 distances.)"""
    dim, n, k = 20, 3000, 10
    rng = np.random.default_rng(6000)
    X, Q = gc.make_data(n, dim, metric, 6001, nq=16)
    rows = {int(i): X[i] for i in range(n)}

    def check(index, what, slots_known=False):
        ks = np.array(sorted(rows), dtype=np.int64)
        ref = gc.ExactReference(metric, np.stack([rows[int(i)] for i in ks]), ks, ks if slots_known else None, Q, k)
        gc.assert_exact_answer(index.search_batch(Q, k, exact=True), ref.top(k), "%s after %s" % (metric, what))

    gpu = build(dim, metric, X, capacity=n + 100)
    check(gpu, "build", slots_known=True)
    gone = rng.choice(n, 100, replace=False)
    assert gpu.remove(gone) == 100
    for i in gone:
        del rows[int(i)]
    check(gpu, "remove")
    new = (30.0 * gc.make_data(100, dim, "l2sq", 6002)[0]).astype(np.float32)
    gpu.add(np.arange(n, n + 100), new)  # takes over freed slots (as many as the free ring still names: DESIGN quirk Q11)
    assert n <= gpu.nodes() < n + 100
    rows.update({n + i: new[i] for i in range(100)})
    check(gpu, "add into freed slots")
    at = gpu.nodes()
    gpu.reserve(n + 600)  # reallocates
    more = (0.05 * gc.make_data(300, dim, "l2sq", 6003)[0]).astype(np.float32)
    gpu.add(np.arange(n + 100, n + 400), more)
    assert gpu.nodes() == at + 300
    rows.update({n + 100 + i: more[i] for i in range(300)})
    check(gpu, "add past the end")
    fresh = gc.gpu_index(dim, metric, 8, 16, 16)
    fresh.load(gpu.save())
    check(fresh, "save + load")
    drop = np.array([i for i in range(50) if i in rows], dtype=np.int64)  # (so that compact has tombstones to drop)
    assert fresh.remove(drop) == len(drop) > 0
    for i in drop:
        del rows[int(i)]
    fresh.compact()
    check(fresh, "compact")
