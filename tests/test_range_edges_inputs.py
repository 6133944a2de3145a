"""The inputs of tests/test_gpu_range_edges.py (range_edge_cases.py), built at their real sizes and checked with the oracle alone
(gpu_common.ExactReference): each GPU case reaches what it is for, so none of them can pass vacuously.  No GPU."""
import numpy as np
import pytest

import range_edge_cases as rec
from range_edge_cases import BLOCK, CHUNK


def test_header_constants():
    assert CHUNK > 0 and BLOCK > 0 and rec.A_ROWS == 2 * CHUNK + 5 and rec.A_NQ == 2 * BLOCK + 3
    assert -(-rec.A_ROWS // CHUNK) == 3 and -(-rec.A_NQ // BLOCK) == 3  # more than two row chunks, more than one query block


@pytest.mark.parametrize("metric", ["l2sq", "cosine"])
def test_blocks_case(metric):
    c = rec.blocks_case(metric)
    n_live = int(c.live.sum())
    assert n_live > CHUNK and c.ref.n == n_live
    with np.errstate(invalid="ignore"):
        d0, d4 = c.ref.dist[:, 0], c.ref.dist[:, 4]
        kind = np.select([np.isnan(c.radii), np.isinf(c.radii), c.radii < d0, c.radii == d4, c.radii < d4], [4, 3, 0, 1, 2], -1)
    assert (kind >= 0).all()
    matches = np.diff(c.want[0].astype(np.int64))
    for b in range(3):
        block = slice(b * BLOCK, min((b + 1) * BLOCK, rec.A_NQ))
        # every radius kind in every query block (the third holds three queries: three kinds, NaN, below the nearest, the 5th)
        assert len(set(kind[block].tolist())) == min(5, len(kind[block])), b
        if b:
            assert ((matches[block] > 0) & (matches[block] < n_live)).any(), b  # a match set neither empty nor full
    assert (matches[kind == 1] >= 5).all() and (matches[kind == 2] <= 4).all() and (matches[kind == 3] == n_live).all()
    # the label form: tenant 0's list is longer than a row chunk, its group larger than a query block
    assert int(((c.tenant == 0) & c.live).sum()) > CHUNK
    tenant0 = (c.lo[:, 0] == 0) & (c.hi[:, 0] == 0)
    assert tenant0.sum() == rec.A_TENANT0_QUERIES > BLOCK
    assert not tenant0[:8].all() and not tenant0[-8:].all()  # (interleaved with the other groups)
    admitted = np.array([len(ids) for ids, _ in c.near])
    assert (admitted[tenant0] > CHUNK).all() and (admitted[c.kind == 1] == 31).all() and (admitted[c.kind == 2] == 9).all()
    assert (admitted[c.kind >= 3] == 0).all() and (c.kind == 3).any() and (c.kind == 4).any()
    box_matches = np.diff(c.box_want[0].astype(np.int64))
    assert ((box_matches[tenant0] > 0) & (box_matches[tenant0] < admitted[tenant0])).any()


@pytest.mark.parametrize("metric", ["ip", "cosine"])
def test_full_tiles_case(metric):
    c = rec.full_tiles_case(metric)
    live = np.ones(rec.B_ROWS, bool)
    want, box_want = c.answers(live)
    assert want[0][-1] == 256 * 256 and box_want[0][-1] == (128 + 32) * 256
    live[rec.B_CORNERS] = False
    want, box_want = c.answers(live)
    assert want[0][-1] == 256 * 252 and box_want[0][-1] == (128 + 32) * 252
    assert rec.k_steps(rec.B_DIM) == 3
    # two distinct boxes, both of which admit every row's label
    assert len({(int(a), int(b)) for a, b in zip(c.lo[:, 0], c.hi[:, 0])}) == 2 and c.labels.max() <= c.hi.min() and (c.lo == 0).all()
    assert (np.diff(c.keys) < 0).all()  # keys run against slot order


def test_k_step_counts():
    assert [rec.k_steps(d) for d in rec.K_STEP_DIMS] == [1, 1, 1, 2, 3, 5]
    assert [-(-(-(-d // 4)) // 8) for d in (64, 100, 768)] == [2, 4, 24]  # (what the existing suites run: all even)
    assert -(-33 // 4) - 8 == 1  # dimension 33: the second step holds one live chunk
    assert rec.k_steps(rec.WIDE_DIM) == 48


@pytest.mark.parametrize("metric", ["l2sq", "cosine"])
def test_mutation_case(metric):
    c = rec.MutationCase(metric)
    rows, norm2_max = {}, 0.0
    names = []
    for name, removed, added in c.steps():
        names.append(name)
        before = max((float(np.dot(v, v)) for v in rows.values()), default=0.0)
        norm2_max = max(norm2_max, before)
        c.follow(rows, removed, added)
        if name == "add into freed slots":
            arrivals = set(added[0].tolist())
            (radii, want), (box_radii, box_want) = c.answers(rows)
            for q in range(rec.D_NQ):  # the arrivals are the expected matches, with and without the boxes
                assert arrivals & set(want[1][q][0].tolist()), q
                assert arrivals & set(box_want[1][q][0].tolist()), q
            gone2 = (c.X[c.gone].astype(np.float64) ** 2).sum(axis=1)
            new2 = (c.arrivals.astype(np.float64) ** 2).sum(axis=1)
            assert gone2.min() >= 100 * new2.max(), (gone2.min(), new2.max())  # whichever freed slot an arrival takes
        if name == "reserve and add past the end":
            assert (added[1].astype(np.float64) ** 2).sum(axis=1).max() > norm2_max
    assert names == ["build", "remove", "add into freed slots", "reserve and add past the end", "save and load", "remove again", "compact"]
    assert len(c.drop) > 0 and len(rows) == rec.D_ROWS + 300 - len(c.drop)
    assert c.label_rows > max(rows)


@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_duplicates_case(metric):
    import gpu_common as gc
    X, Q, keys, live = rec.degenerate_data(metric, "duplicates")
    assert len(rec.E_DUPLICATED) == 20 and live[rec.E_DUPLICATED].all() and live[rec.E_DUPLICATED + 128].all() and live[rec.E_DUPLICATED + 256].all()
    assert (rec.E_DUPLICATED < 128).all() and (rec.E_DUPLICATED + 256 < rec.E_ROWS).all()  # one copy in each of three 128-row tiles
    ref = gc.ExactReference(metric, X[live], keys[live], None, Q, rec.E_ROWS)
    by_key = np.argsort(ref.keys, axis=1)
    dist = np.take_along_axis(ref.dist, by_key, axis=1)  # columns = the live keys ascending
    column = {int(k): j for j, k in enumerate(keys[live])}
    for i in rec.E_DUPLICATED:
        a, b, c = (dist[:, column[int(i) + o]].view(np.uint32) for o in (0, 128, 256))
        assert np.array_equal(a, b) and np.array_equal(a, c), i
    seen = set()
    for triples, at, below in rec.duplicate_rounds(ref):
        seen |= set(triples[:, 0].tolist())
        assert (below < at).all()
    assert seen == set(rec.E_DUPLICATED.tolist())


@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_zero_row_case(metric):
    X, Q, keys, live = rec.degenerate_data(metric, "zero row")
    assert live[rec.E_ZERO_ROW] and not X[rec.E_ZERO_ROW].any() and (np.abs(X).sum(axis=1) > 0).sum() == rec.E_ROWS - 1
