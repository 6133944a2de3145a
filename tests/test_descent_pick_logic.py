"""The rule the descent's pre-scoring rests on (hnsw_kernels.h, "THE CONTRACT, FOR THE DESCENT"), in numpy: descend() moves to
the first occurrence of the minimum only if it is STRICTLY smaller than closest_dist, so replacing any subset of the entries
that are >= closest_dist by +inf leaves the pick — whether it moves, where to, the new closest_dist — unchanged."""
import numpy as np

INF = np.float32(np.inf)


def _pick(dist, closest_dist):
    """descend(): (changed, index, bits of the new closest_dist); NaN compares false, as in the kernel"""
    with np.errstate(invalid="ignore"):
        m = np.fmin.reduce(dist)  # (fminf ignores NaN)
        if m < closest_dist:
            return True, int(np.nonzero(dist == m)[0][0]), int(np.float32(m).view(np.uint32))
    return False, -1, int(np.float32(closest_dist).view(np.uint32))


def _filtered(dist, thr, mask):
    """what the scoring waves may hand back: +inf for the rows of `mask`, and only under a bound below +inf"""
    out = dist.copy()
    with np.errstate(invalid="ignore"):
        if thr < INF:
            out[mask] = INF
    return out


def test_rejecting_rows_at_or_beyond_the_threshold_never_changes_the_pick():
    rng = np.random.default_rng(1010)
    for trial in range(4000):
        n = int(rng.integers(1, 65))
        if trial % 2:  # few distinct values: ties among the rows, and rows exactly equal to the threshold
            dist = rng.integers(0, 5, size=n).astype(np.float32)
            thr = np.float32(rng.integers(0, 6))
        else:
            dist = rng.random(n, dtype=np.float32)
            thr = dist[rng.integers(0, n)] if trial % 4 else np.float32(rng.random())  # equal to an entry, or anywhere
        if trial % 7 == 0:
            thr = (INF, np.float32(np.nan), -INF)[trial % 3]
        with np.errstate(invalid="ignore"):
            may = dist >= thr  # a proved bound >= closest_dist implies this (bound <= distance)
        for mask in (may, may & (rng.random(n) < 0.5), np.zeros(n, bool)):
            assert _pick(_filtered(dist, thr, mask), thr) == _pick(dist, thr), (dist, thr, mask)


def test_the_rule_is_tight():
    """+inf for the one row strictly below the threshold does change the pick"""
    dist = np.array([3, 1, 2, 1.5], dtype=np.float32)
    thr = np.float32(1.5)
    assert _pick(dist, thr) == (True, 1, int(np.float32(1).view(np.uint32)))
    assert _pick(_filtered(dist, thr, np.array([False, True, False, False])), thr)[0] is False
    # equality is covered: the row AT the threshold may go, the first occurrence of a tie below it is kept
    tie = np.array([1.5, 1, 1, 7], dtype=np.float32)
    assert _pick(_filtered(tie, thr, tie >= thr), thr) == _pick(tie, thr) == (True, 1, int(np.float32(1).view(np.uint32)))
