"""The row-maxima rules of MH_LINKAGE_ROWMAX (tests/linkage_rowmax_ref.py: what moped_amd/csrc/linkage_rowmax.hip runs)
against the oracle's restatement of the reference's merge loop (orclib.linkage_agglomerate), without a GPU: clusters and
member order equal, no tolerance, on
  - uniform, quarter-valued (ties everywhere), block-structured and NaN-sprinkled matrices of 1 .. 69 rows,
    linkage types 0 / 1 / 2, cutoffs 0.05 / 0.3 / 0.6 (2484 cases),
  - the Gaussian similarity of a point set of 400.
The stale path (a merge won through the just absorbed, still listed index: more merges than points can come of it)
must occur, or the rules for it are untested."""
import numpy as np
import pytest

import linkage_rowmax_ref as rm
import orclib

SIZES = tuple(range(1, 70))
CUTOFFS = (0.05, 0.3, 0.6)
GENERATORS = ("uniform", "quarters", "blocks", "nan")


def symmetric(M):
    return np.ascontiguousarray(np.triu(M) + np.triu(M, 1).T, np.float32)


def matrix(kind, n, seed=0):
    rng = np.random.default_rng([GENERATORS.index(kind), n, seed])
    if kind == "uniform":
        return symmetric(rng.random((n, n)).astype(np.float32))
    if kind == "quarters":
        return symmetric(rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32), (n, n)))
    if kind == "blocks":
        g = rng.integers(0, max(1, n // 8) + 1, n)
        M = np.where(g[:, None] == g[None, :], 0.7, 0.1) + rng.uniform(-0.08, 0.08, (n, n))
        return symmetric(M.astype(np.float32))
    M = symmetric(rng.choice(np.array([0.2, 0.5, 0.8], np.float32), (n, n)))
    hole = np.triu(rng.random((n, n)) < 0.25, 1)
    M[hole | hole.T] = np.nan
    if n > 2:
        k = int(rng.integers(0, n))
        M[k, :] = M[:, k] = np.nan          # a row of nothing but NaN
    return M


def gaussian(n, seed=3):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.normal(c, 0.6, (n // 4, 2)) for c in ((0, 0), (4, 0), (0, 4), (5, 5))])
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    return np.exp(-d2 / 2.0).astype(np.float32)


def same(M, cutoff, ltype, tag):
    got, stats = rm.agglomerate_rowmax(M, cutoff, 0, ltype)
    want = orclib.linkage_agglomerate(M, cutoff, 0, ltype)
    assert got == [c.tolist() for c in want], tag
    return stats


@pytest.mark.parametrize("kind", GENERATORS)
def test_rowmax_rules_equal_the_oracle(kind):
    merges = rescans = stale = 0
    more_merges_than_points = 0
    for n in SIZES:
        M = matrix(kind, n)
        for ltype in (0, 1, 2):
            for cutoff in CUTOFFS:
                st = same(M, cutoff, ltype, (kind, n, ltype, cutoff))
                merges += st["merges"]
                rescans += st["rescans"]
                stale += st["stale"]
                more_merges_than_points += st["merges"] > n
    print(kind, "merges", merges, "rescans per merge %.2f" % (rescans / max(merges, 1)), "stale merges", stale,
          "cases with more merges than points", more_merges_than_points)
    assert merges > 1000
    assert rescans <= 3 * merges            # about two rows per merge, the row of `first` among them


def test_stale_merges_occur():
    """Minimum linkage over equal similarities: the absorbed index wins the next scan through its 1e20 row -- merges with
    S2 = 0, more merges than points -- and the row-maxima rules follow the oracle through it."""
    n = 17
    M = np.full((n, n), 0.5, np.float32)
    st = same(M, 0.3, 0, "all equal")
    assert st["stale"] >= n // 2 - 1 and st["merges"] > n, st
    hits = 0
    for kind in GENERATORS:
        for m in (12, 33, 69):
            st = same(matrix(kind, m, seed=1), 0.05, 0, (kind, m))
            hits += st["merges"] > m
    assert hits >= 1


def test_min_pts_and_size_one():
    assert rm.agglomerate_rowmax(np.ones((1, 1), np.float32), 0.1, 0, 1)[0] == [[0]]
    assert rm.agglomerate_rowmax(np.ones((1, 1), np.float32), 0.1, 1, 1)[0] == []
    M = np.full((7, 7), 0.1, np.float32)
    M[:4, :4] = M[4:, 4:] = 0.9
    for min_pts, sizes in ((2, [4, 3]), (3, [4]), (4, [])):
        got, _ = rm.agglomerate_rowmax(M, 0.5, min_pts, 1)
        assert [len(c) for c in got] == sizes
        assert got == [c.tolist() for c in orclib.linkage_agglomerate(M, 0.5, min_pts, 1)]


def test_gaussian_point_set_of_400():
    M = gaussian(400)
    for ltype, cutoff in ((1, 0.3), (0, 0.05), (2, 0.6)):
        st = same(M, cutoff, ltype, ("gaussian", ltype, cutoff))
        print("gaussian 400", ltype, cutoff, st, "rescans per merge %.2f" % (st["rescans"] / max(st["merges"], 1)))
        assert st["merges"] >= 300
